"""CPU: tests/mldsa_spec.py (the FIPS 204 restatement the GPU tests compare with) against
tests/golden/mldsa.json and against its own parts: re-signing, every record, every tamper entry's flag
word, sizes, the derived twiddle table, each malformed-hint class and the norm bound on z."""
import ast
import hashlib
from pathlib import Path

import numpy as np
import pytest

import make_golden_mldsa as gold
import mldsa_spec as spec

SETS = sorted(spec.PARAMS)
SIZES = {"ML-DSA-44": (1312, 2560, 2420), "ML-DSA-65": (1952, 4032, 3309), "ML-DSA-87": (2592, 4896, 4627)}


@pytest.fixture(scope="module")
def fixture():
    return gold.load()


def test_fixture_regenerates_bit_identically_in_shape_and_size(fixture):
    assert sorted(fixture) == SETS
    assert gold.OUT.stat().st_size < 100_000
    for name in SETS:
        assert [r["len"] for r in fixture[name]["records"]] == [0, 70, 71, 2500]
        assert 64 + 2 + 70 == 136  # tr || M' of the second record fills one SHAKE256 block exactly


@pytest.mark.parametrize("name", SETS)
def test_sizes_and_key_from_xi(name, fixture):
    p, f = spec.PARAMS[name], fixture[name]
    assert (p.pk, p.sk, p.sig) == SIZES[name]
    pk, sk = spec.keygen_internal(f["xi"], name)
    assert pk == f["pk"] and (len(pk), len(sk)) == SIZES[name][:2]
    assert all(len(s) == p.sig for s in f["sigs"])


@pytest.mark.parametrize("name", SETS)
def test_spec_resigns_a_record_bit_identically(name, fixture):
    f = fixture[name]
    _, sk = spec.keygen_internal(f["xi"], name)
    assert spec.sign(sk, f["msgs"][2]) == f["sigs"][2]
    assert spec.sign_internal(sk, b"\0\0" + f["msgs"][1], bytes(32)) == f["sigs"][1]  # the ACVP interface
    assert spec.sign(sk, f["msgs"][2], rnd=bytes([1]) * 32) != f["sigs"][2]  # hedged signing differs


@pytest.mark.parametrize("name", SETS)
def test_spec_verifies_every_record_with_the_stored_trace(name, fixture):
    f = fixture[name]
    for msg, sig, rec in zip(f["msgs"], f["sigs"], f["records"]):
        assert spec.verify(f["pk"], msg, sig)
        assert spec.verify_internal(f["pk"], b"\0\0" + msg, sig)
        tr = spec.verify_trace(f["pk"], msg, sig)
        assert tr["flags"] == 0 and tr["mu"].hex() == rec["mu"] and tr["ctilde"].hex() == rec["ctilde"]
        assert hashlib.sha3_256(tr["w1"]).hexdigest() == rec["w1_sha3"]
        assert not spec.verify(f["pk"], msg, sig, ctx=b"x")


@pytest.mark.parametrize("name", SETS)
def test_spec_returns_the_stored_flag_word_for_every_tamper_entry(name, fixture):
    f = fixture[name]
    seen = set()
    for e in f["tampers"]:
        pk, msg, sig = gold.apply_tamper(e, f["pk"], f["msgs"], f["sigs"])
        assert spec.verify_trace(pk, msg, sig)["flags"] == e["flags"] != 0, e["label"]
        assert not spec.verify(pk, msg, sig), e["label"]
        seen.add(e["flags"])
    assert {spec.FLAG_HINT, spec.FLAG_HASH, spec.FLAG_NORM | spec.FLAG_HASH} <= seen


def test_twiddles_are_derived_from_zeta_not_stored():
    z = spec.zetas()
    assert z[0] == 1 and z[1] == pow(1753, 128, spec.Q) == 4808194 and z[255] == pow(1753, 255, spec.Q)
    assert pow(1753, 256, spec.Q) == spec.Q - 1 and pow(1753, 512, spec.Q) == 1  # a primitive 512th root
    assert spec.INV256 == 8347681
    # no long integer table in the source: the largest literal list has a handful of entries
    tree = ast.parse(Path(spec.__file__).read_text())
    assert max((len(n.elts) for n in ast.walk(tree) if isinstance(n, (ast.List, ast.Tuple))), default=0) < 16
    x = np.arange(256) * 32749 % spec.Q
    assert list(spec.ntt(x)) == spec.ntt_slow(x)
    assert np.array_equal(spec.ntt_inv(spec.ntt(x)), x)
    # the NTT is the negacyclic convolution's transform: x * X = x shifted with a sign flip
    shift = np.zeros(256, dtype=np.int64)
    shift[1] = 1
    prod = spec.ntt_inv(spec.ntt(x) * spec.ntt(shift) % spec.Q)
    assert np.array_equal(prod, np.concatenate([[(-x[255]) % spec.Q], x[:255]]))


@pytest.mark.parametrize("name", SETS)
def test_hint_bit_unpack_rejects_each_malformed_class(name):
    p = spec.PARAMS[name]
    h = np.zeros((p.k, 256), dtype=np.int64)
    h[0][[3, 7, 200]] = 1
    h[1][[0, 255]] = 1
    h[p.k - 1][[9]] = 1
    y = spec.hint_bit_pack(p, h)
    assert np.array_equal(spec.hint_bit_unpack(p, y), h)

    def edit(pos, val):
        b = bytearray(y)
        b[pos] = val
        return bytes(b)

    assert spec.hint_bit_unpack(p, edit(1, 3)) is None          # index equal to its predecessor
    assert spec.hint_bit_unpack(p, edit(1, 2)) is None          # index decreasing
    assert spec.hint_bit_unpack(p, edit(3, 1)) is not None      # a new polynomial may start lower
    assert spec.hint_bit_unpack(p, edit(p.omega + 1, 2)) is None        # count decreasing (3, then 2)
    assert spec.hint_bit_unpack(p, edit(p.omega + p.k - 1, p.omega + 1)) is None  # count above omega
    assert spec.hint_bit_unpack(p, edit(6, 1)) is None          # nonzero padding right after the last index
    assert spec.hint_bit_unpack(p, edit(p.omega - 1, 1)) is None        # nonzero padding at the end
    full = np.zeros((p.k, 256), dtype=np.int64)
    full[0][:p.omega] = 1                                        # exactly omega hints is allowed
    assert np.array_equal(spec.hint_bit_unpack(p, spec.hint_bit_pack(p, full)), full)


@pytest.mark.parametrize("name", SETS)
def test_z_norm_bound_is_exact(name, fixture):
    p, f = spec.PARAMS[name], fixture[name]
    bound = p.gamma1 - p.beta
    for value, over in ((bound, True), (-bound, True), (bound - 1, False), (-(bound - 1), False)):
        sig = bytearray(f["sigs"][1])
        for pos, b in gold._z_coeff0(p, f["sigs"][1], value):
            sig[pos] = b
        assert spec.sig_decode(p, bytes(sig))[1][0][0] == value
        flags = spec.verify_trace(f["pk"], f["msgs"][1], bytes(sig))["flags"]
        assert bool(flags & spec.FLAG_NORM) == over, (value, flags)


def test_decompose_and_use_hint_identities():
    r = np.concatenate([np.arange(0, 4096), np.arange(spec.Q - 4096, spec.Q),
                        np.random.default_rng(1).integers(0, spec.Q, 20000)])
    for p in (spec.PARAMS["ML-DSA-44"], spec.PARAMS["ML-DSA-65"]):
        r1, r0 = spec.decompose(p, r)
        m = (spec.Q - 1) // (2 * p.gamma2)
        assert np.all((r1 * 2 * p.gamma2 + r0 - r) % spec.Q == 0)
        assert np.all((0 <= r1) & (r1 < m) & (r0 > -p.gamma2 - 1) & (r0 <= p.gamma2))
        assert np.array_equal(spec.use_hint(p, np.zeros_like(r), r), r1)
        assert np.all(spec.use_hint(p, np.ones_like(r), r) != r1)
