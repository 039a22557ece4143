"""FrodoKEM Decaps at its decision edges (CPU): the fixture's own conditions, and the C oracle against
the fixture and against the pure-Python restatement, before the GPU is compared with either.

tests/golden/frodo_edge.json (tests/golden/make_golden_frodo_edge.py) holds encapsulations under keys
whose decryption noise is known in closed form and sits within a sample of a decoding threshold, so
a row is accepted or rejected by the sign of 0, +-1 or +-2.  tests/frodo_decrypt_cases.py holds the
secret keys whose S^T leaves the range KeyGen writes.  The GPU path is held to the same rows in
tests/test_gpu_frodo_decrypt.py.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import frodo_decrypt_cases as D
import frodo_spec as F
import make_golden_frodo_edge as E
import oracle as orc

GOLD = json.loads((Path(__file__).parent / "golden" / "frodo_edge.json").read_text())
ALGS = list(E.ALGS)


@pytest.fixture(scope="module")
def rebuilt():
    """alg -> per key (pk, sk, mu rows, accept, noise, oracle ct, oracle Encaps ss, oracle Decaps ss), once."""
    out = {}
    for alg in ALGS:
        g = GOLD[alg]
        keys = []
        for t, k in enumerate(g["keys"]):
            pk, sk = E.build_key(alg, bytes.fromhex(g["seedA"]), t, k["i0"], k["j0"], k["delta"])
            mu, accept, noise = E.rows_of(alg, k)
            pks, sks = (np.tile(np.frombuffer(x, np.uint8), (len(mu), 1)) for x in (pk, sk))
            ct, ss = orc.batch_encaps(alg, pks, mu)
            keys.append((pk, sk, mu, accept, noise, ct, ss, orc.batch_decaps(alg, sks, ct)))
        out[alg] = keys
    return out


@pytest.fixture
def memo_gen_a(monkeypatch):
    """frodo_spec.gen_a computed once per (set, seedA): the AES matrix is 51,200 pure-Python blocks."""
    real, memo = F.gen_a, {}

    def gen_a(p, seed_a):
        key = (p["n"], p["prg"], bytes(seed_a))
        if key not in memo:
            memo[key] = real(p, seed_a)
        return memo[key]
    monkeypatch.setattr(F, "gen_a", gen_a)


@pytest.mark.parametrize("alg", ALGS)
def test_fixture_conditions(alg):
    """At most 256 rows over the three keys (i0, j0) = (0, 0), (3, n/4), (7, n-1); at least 16 accepting and
    16 rejecting rows; each exact noise value th-1, th, -th, -th-1 decides a row alone -- every other
    position at least th/8 inside its cell -- and th-1, -th accept while th, -th-1 reject; the accept bit
    is what the stored noise says."""
    p = F.params(alg)
    assert GOLD[alg]["seedA"] == E.derive(alg, b"seedA", 16).hex()
    E.check(alg, GOLD[alg])
    for k in GOLD[alg]["keys"]:
        assert k["delta"] == 1024 and 0 <= k["i0"] < 8 and 0 <= k["j0"] < p["n"]
        assert all(len(bytes.fromhex(r["mu"])) == p["len_mu"] for r in k["rows"])


@pytest.mark.parametrize("alg", ALGS)
def test_c_oracle_reproduces_the_fixture(alg, rebuilt):
    """On every row: Encaps under the crafted pk gives the stored ct and ss digests; Decaps returns the
    Encaps ss exactly where the accept bit is set and H(ct || s) elsewhere; and M = C - B'S computed in
    numpy from the oracle's ciphertext is Encode(mu) plus the stored noise in column i0, |E''| <= 12
    elsewhere (the closed form)."""
    p = F.params(alg)
    n, q, sec = p["n"], 1 << p["logq"], p["sec"]
    for k, (pk, sk, mu, accept, noise, ct, ss, ss_d) in zip(GOLD[alg]["keys"], rebuilt[alg]):
        for i, r in enumerate(k["rows"]):
            assert hashlib.sha256(ct[i].tobytes()).hexdigest() == r["ct"]
            assert hashlib.sha256(ss[i].tobytes()).hexdigest() == r["ss"]
            want = ss[i].tobytes() if accept[i] else E.shake(p, ct[i].tobytes() + sk[:sec], sec)
            assert ss_d[i].tobytes() == want, (alg, k["i0"], i)
        vals = E.unpack_rows(ct, p["logq"])
        Bp, C = vals[:, :8 * n].reshape(-1, 8, n), vals[:, 8 * n:].reshape(-1, 8, 8)
        St = np.zeros((8, n), np.int64)
        St[k["i0"], k["j0"]] = k["delta"]
        enc = np.stack([F.encode(p, m.tobytes()).astype(np.int64) for m in mu])
        e = (C - Bp @ St.T - enc) % q
        e = np.where(e >= q // 2, e - q, e)
        assert np.array_equal(e[:, :, k["i0"]], noise)
        e[:, :, k["i0"]] = 0
        assert np.abs(e).max() <= 12


@pytest.mark.parametrize("alg", ALGS)
def test_spec_agrees_on_the_decided_rows(alg, rebuilt, memo_gen_a):
    """One row per exact value th-1, th, -th, -th-1: frodo_spec's Encaps and Decaps give the C oracle's
    bytes, and frodo_spec.decode of the closed-form M is mu on the accepted two and not on the others."""
    p = F.params(alg)
    T = E.th(p)
    todo = {T - 1, T, -T, -T - 1}
    for k, (pk, sk, mu, accept, noise, ct, ss, ss_d) in zip(GOLD[alg]["keys"], rebuilt[alg]):
        for i in range(len(mu)):
            v = E.decided_by(p, noise[i])
            if v not in todo:
                continue
            todo.discard(v)
            m = mu[i].tobytes()
            assert F.encaps_derand(alg, pk, m) == (ct[i].tobytes(), ss[i].tobytes())
            assert F.decaps(alg, sk, ct[i].tobytes()) == ss_d[i].tobytes()
            M = F.encode(p, m).astype(np.int64)
            M[:, k["i0"]] += noise[i]
            assert (F.decode(p, M) == m) == bool(accept[i]) == (v in (T - 1, -T))
    assert not todo


def test_c_oracle_and_spec_agree_on_the_st_cases(memo_gen_a):
    """The S^T cases of the GPU product test (every entry 0x8000, 0x7FFF, +-12, uniform int16, one entry
    +-1), FrodoKEM-640-SHAKE: the C oracle's Decaps equals frodo_spec.decaps, and frodo_spec.decode of the
    numpy M is what both re-encrypt (every row rejects: ss = H(ct || s))."""
    alg = "FrodoKEM-640-SHAKE"
    p = F.params(alg)
    names, St, Bp, C, M = D.product_cases(alg)
    assert len(names) == 4 * 2 * 2 + 2 * 18 and {n.split(",")[0] for n in names[:16]} == {
        "S^T 0x8000", "S^T 0x7FFF", "S^T +-12", "S^T int16"}
    _, sk = D.honest_key(alg)
    sks, ct = D.with_st(p, sk, St), D.assemble_ct(p, Bp, C)
    got = orc.batch_decaps(alg, sks, ct)
    for i, name in enumerate(names):
        want = F.decaps(alg, sks[i].tobytes(), ct[i].tobytes())
        assert got[i].tobytes() == want, name
        assert want == E.shake(p, ct[i].tobytes() + sk[:p["sec"]], p["sec"]), name
    # the numpy M is the spec's: same Decode input as frodo_spec.decaps builds from the bytes
    i = names.index("S^T int16, B' uniform")
    St_b = np.frombuffer(sks[i].tobytes()[p["sec"] + p["pk"]:][:16 * p["n"]], "<u2").reshape(8, p["n"])
    assert np.array_equal((C[i] - F._mm(Bp[i], St_b.T)) & ((1 << p["logq"]) - 1), M[i])


def test_trace_hook_is_exported_undeclared_and_checks_its_arguments_first():
    """qrk_dbg_frodo_decaps_trace is a test hook: exported, kept out of the public header; a name that is
    no FrodoKEM parameter set, a null context and null buffers are refused before any device work."""
    import ctypes as ct

    import qrkem
    from qrkem._debug import bind
    from test_abi import declared_functions, exported_symbols
    assert "qrk_dbg_frodo_decaps_trace" in exported_symbols()
    assert "qrk_dbg_frodo_decaps_trace" not in declared_functions()
    fn = bind().qrk_dbg_frodo_decaps_trace
    ctx = ct.c_void_p(1)  # never dereferenced: the name and the buffers are checked first
    for alg, msg in ((b"ML-KEM-768", "not a FrodoKEM parameter set"), (b"HQC-128", "not a FrodoKEM parameter set"),
                     (b"FrodoKEM-640", "unsupported KEM")):
        assert fn(ctx, alg, 1, None, None, None, None, None) == -1
        assert msg in qrkem.last_error()
    assert fn(None, b"FrodoKEM-640-SHAKE", 1, None, None, None, None, None) == -1
    assert "null context" in qrkem.last_error()
    assert fn(ctx, b"FrodoKEM-640-SHAKE", 1, None, None, None, None, None) == -1
    assert "null buffer" in qrkem.last_error()
