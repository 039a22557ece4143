"""CPU: tests/aead_spec.py (the checker of the GPU AEAD tests) is pinned to OpenSSL -- through
tests/golden/aead.json, which tests/golden/make_golden_aead.py wrote with the machine's libcrypto, and
directly where a libcrypto loads."""
import json

import numpy as np
import pytest

import aead_spec
from make_golden_aead import AAD_LENS, ALGS, PT_LENS, PUBLISHED, evp_seal, load_libcrypto


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "aead.json").read_text())


def rows(golden, alg):
    return [{k: bytes.fromhex(v) for k, v in r.items()} for r in golden["records"][alg]]


def test_fixture_covers_the_length_sets_and_published_vectors(golden):
    assert golden["openssl"].startswith("OpenSSL ")
    for alg in ALGS:
        recs = rows(golden, alg)
        assert len(recs) >= 64
        assert {len(r["pt"]) for r in recs} >= set(PT_LENS)
        assert {len(r["aad"]) for r in recs} >= set(AAD_LENS)
        assert all(len(r["sealed"]) == len(r["pt"]) + 28 and r["sealed"][:12] == r["nonce"] for r in recs)
        p = PUBLISHED[alg]
        assert recs[0]["key"].hex() == p["key"] and recs[0]["sealed"][-16:].hex() == p["tag"]
    assert rows(golden, "AES-256-GCM")[0]["sealed"][12:28].hex() == "cea7403d4d606b6e074ec5d3baf39d18"


@pytest.mark.parametrize("alg", ALGS)
def test_spec_reproduces_every_record(golden, alg):
    for r in rows(golden, alg):
        assert aead_spec.seal(alg, r["key"], r["nonce"], r["pt"], r["aad"]) == r["sealed"]
        assert aead_spec.open_(alg, r["key"], r["sealed"], r["aad"]) == r["pt"]


def flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


@pytest.mark.parametrize("alg", ALGS)
def test_spec_rejects_one_flipped_bit(golden, alg):
    """One bit in the ciphertext, the tag, the nonce and the aad of each record (the bit position moves
    with the record index; a record without ciphertext or aad bytes skips that part only)."""
    for j, r in enumerate(rows(golden, alg)):
        s, n_ct = r["sealed"], len(r["pt"])
        assert aead_spec.open_(alg, r["key"], flip(s, (12 + n_ct) * 8 + (37 * j) % 128), r["aad"]) is None  # tag
        assert aead_spec.open_(alg, r["key"], flip(s, (11 * j) % 96), r["aad"]) is None  # nonce
        if n_ct:
            assert aead_spec.open_(alg, r["key"], flip(s, 96 + (13 * j) % (8 * n_ct)), r["aad"]) is None
        if r["aad"]:
            assert aead_spec.open_(alg, r["key"], s, flip(r["aad"], (7 * j) % (8 * len(r["aad"])))) is None
        else:
            assert aead_spec.open_(alg, r["key"], s, b"\0") is None
    assert aead_spec.open_(alg, bytes(32), bytes(27)) is None


def test_poly1305_final_reduction_and_wrap():
    """The accumulator values p .. p + 4 and the carry out of h + s (RFC 8439 section 2.5.1's last two steps)."""
    key = (1).to_bytes(16, "little") + b"\xff" * 16
    for k in range(5):
        msg = (1 << 127).to_bytes(16, "little") + ((1 << 127) - 5 + k).to_bytes(16, "little") + bytes(16)
        # r = 1: h = (2^127 + 2^128) + (2^127 - 5 + k + 2^128) + 2^128 = 2^130 - 5 + k = p + k, so the tag
        # is (k + s) mod 2^128 with s = 2^128 - 1
        assert aead_spec.poly1305(key, msg) == ((k - 1) % (1 << 128)).to_bytes(16, "little")


@pytest.mark.parametrize("alg", ALGS)
def test_spec_matches_libcrypto_on_fresh_records(alg):
    lib = load_libcrypto()
    if lib is None:
        pytest.skip("no OpenSSL libcrypto loads on this machine; the committed fixture still pins the spec")
    rng = np.random.default_rng(0xAEAD + len(alg))
    for _ in range(200):
        key, nonce = rng.bytes(32), rng.bytes(12)
        pt, aad = rng.bytes(int(rng.integers(0, 300))), rng.bytes(int(rng.integers(0, 120)))
        assert aead_spec.seal(alg, key, nonce, pt, aad) == evp_seal(lib, alg, key, nonce, pt, aad)


def test_fixture_regenerates_bit_identically(golden_dir):
    from make_golden_aead import generate, openssl_version, render
    lib = load_libcrypto()
    if lib is None:
        pytest.skip("no OpenSSL libcrypto loads on this machine")
    committed = (golden_dir / "aead.json").read_text()
    doc = generate(lib)
    if json.loads(committed)["openssl"] != openssl_version(lib):
        # another OpenSSL than the recorded one must still give the same bytes; only the label differs
        doc["openssl"] = json.loads(committed)["openssl"]
    assert render(doc) == committed
