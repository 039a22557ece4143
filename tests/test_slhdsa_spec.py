"""CPU: tests/slhdsa_spec.py against itself and tests/golden/slhdsa.json -- sizes, sign then verify for the
six names, the two flavours rejecting each other's signatures, every tamper class of the GPU tests, and
the fixture's digests.  (Parity with liboqs or the FIPS 205 KATs is unpinned: see the spec's docstring.)"""
import hashlib
import re

import pytest

import make_golden_slhdsa as gold
import slhdsa_spec as spec

TABLE = {  # n, h, d, h', a, k, len, m, pk, sk, sig
    "128f": (16, 66, 22, 3, 6, 33, 35, 34, 32, 64, 17088),
    "192f": (24, 66, 22, 3, 8, 33, 51, 42, 48, 96, 35664),
    "256f": (32, 68, 17, 4, 9, 35, 67, 49, 64, 128, 49856),
}
NAMES = sorted(spec.PARAMS)


def set_of(name: str) -> str:
    return re.search(r"\d+f", name).group()


def other_flavour(name: str) -> str:
    s = set_of(name)
    return f"SLH-DSA-SHA2-{s}" if name.startswith("SPHINCS+") else f"SPHINCS+-SHA2-{s}-simple"


@pytest.fixture(scope="module")
def fixture():
    return gold.load()


@pytest.fixture(scope="module")
def sigs(fixture):
    return {name: gold.signatures(name, fixture[name]) for name in NAMES}


def test_sizes_equal_the_table():
    assert len(NAMES) == 6
    for name, p in spec.PARAMS.items():
        s = set_of(name)
        assert name in (f"SPHINCS+-SHA2-{s}-simple", f"SLH-DSA-SHA2-{s}")
        assert (p.n, p.h, p.d, p.hp, p.a, p.k, p.len, p.m, p.pk, p.sk, p.sig) == TABLE[s]
        assert p.fips == name.startswith("SLH-DSA") and p.h == p.d * p.hp
        assert p.m == p.md + 8 + 1 and p.sig == p.n * (1 + p.k * (p.a + 1) + p.h + p.d * p.len)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_reproduces_and_verifies(fixture, sigs, name):
    p, f = spec.PARAMS[name], fixture[name]
    assert f["keygen_pk"] == f["pk"] and f["pk"][:p.n] == f["seeds"][2]
    for m, sig, rec in zip(f["msgs"], sigs[name], f["records"]):
        tr = spec.verify_trace(name, f["pk"], m, sig)
        assert tr["flags"] == 0 and spec.verify(name, f["pk"], m, sig) is True
        assert tr["digest"].hex() == rec["digest"] and tr["fors_pk"].hex() == rec["fors_pk"]
        assert hashlib.sha3_256(tr["roots"]).hexdigest() == rec["roots_sha3"]
        assert tr["roots"][-p.n:] == f["pk"][p.n:]


@pytest.mark.parametrize("name", NAMES)
def test_flavours_reject_each_other(fixture, sigs, name):
    f = fixture[name]
    other = other_flavour(name)
    assert spec.PARAMS[other].sig == spec.PARAMS[name].sig
    for m, sig in zip(f["msgs"][:2], sigs[name][:2]):
        assert spec.verify(other, f["pk"], m, sig) is False


def tampers(p, pk: bytes, msg: bytes, sig: bytes):
    """(label, pk, msg, sig, first stage that must change): stage -2 = digest, -1 = fors_pk, j = root of layer j."""
    n = p.n
    fors = p.k * (p.a + 1) * n
    ht = n + fors
    xl = (p.hp + p.len) * n

    def flip(b: bytes, i: int, bit: int = 0) -> bytes:
        return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]

    return [
        ("R", pk, msg, flip(sig, 0), -2),
        ("first FORS secret value", pk, msg, flip(sig, n, 7), -1),
        ("last FORS authentication node", pk, msg, flip(sig, ht - 1), -1),
        ("layer-0 WOTS chain value", pk, msg, flip(sig, ht + 5 * n, 3), 0),
        ("layer-(d-1) WOTS chain value (last chain)", pk, msg, flip(sig, ht + (p.d - 1) * xl + (p.len - 1) * n, 6),
         p.d - 1),
        ("last byte of the signature", pk, msg, flip(sig, p.sig - 1), p.d - 1),
        ("message", pk, flip(msg, len(msg) - 1, 4), sig, -2),
        ("PK.seed", flip(pk, 0), msg, sig, -2),
        ("PK.root", flip(pk, 2 * n - 1, 7), msg, sig, -2),
    ]


def check_divergence(p, clean: dict, got: dict, stage: int, label: str):
    """`got` differs from `clean` from `stage` on and not before."""
    n = p.n
    parts = lambda t: [t["digest"], t["fors_pk"]] + [t["roots"][j * n:(j + 1) * n] for j in range(p.d)]
    for i, (a, b) in enumerate(zip(parts(clean), parts(got))):
        assert (a != b) == (i - 2 >= stage), (label, i - 2)


@pytest.mark.parametrize("name", NAMES)
def test_every_tamper_class_is_rejected(fixture, sigs, name):
    p, f = spec.PARAMS[name], fixture[name]
    m, sig = f["msgs"][1], sigs[name][1]
    clean = spec.verify_trace(name, f["pk"], m, sig)
    for label, tpk, tmsg, tsig, stage in tampers(p, f["pk"], m, sig):
        tr = spec.verify_trace(name, tpk, tmsg, tsig)
        assert tr["flags"] == spec.FLAG_ROOT and spec.verify(name, tpk, tmsg, tsig) is False, label
        check_divergence(p, clean, tr, stage, label)


def test_context_strings():
    name = "SLH-DSA-SHA2-128f"
    f = gold.load()[name]
    sig = spec.sign(name, f["sk"], b"msg", ctx=b"abc")
    assert spec.verify(name, f["pk"], b"msg", sig, ctx=b"abc") and not spec.verify(name, f["pk"], b"msg", sig)
    assert not spec.verify(name, f["pk"], b"msg", sig, ctx=bytes(256))
    with pytest.raises(ValueError, match="no context string"):
        spec.sign("SPHINCS+-SHA2-128f-simple", f["sk"], b"msg", ctx=b"abc")
    assert spec.verify("SPHINCS+-SHA2-128f-simple", f["pk"], b"msg", sig, ctx=b"abc") is False


def test_fors_index_orders():
    """The flavour switch itself: 0x80 is index bit a - 1 of tree 0 in FIPS 205 and bit 7 of the stream in
    round 3.1 (tree 1, bit 1, for a = 6)."""
    md = bytes([0x80]) + bytes(24)
    assert spec._fors_indices(spec.PARAMS["SLH-DSA-SHA2-128f"], md)[:2] == [32, 0]
    assert spec._fors_indices(spec.PARAMS["SPHINCS+-SHA2-128f-simple"], md)[:2] == [0, 2]
