"""HIP FrodoKEM Decaps decryption (k_fr_dec_m: M = C - B'S, mu' = Decode(M)) at its decision edges.

Honest ciphertexts keep M within a few hundred of a cell centre (half-width 4096 / 4096 / 2048), and on
a tampered ciphertext ss = H(ct || s) whatever Decode returned, so tests/test_gpu_frodo.py and
tests/test_gpu_fullsize.py pass with a mu' that is wrong away from the centre.  Here mu' itself is read
through the test hook qrk_dbg_frodo_decaps_trace (the launches of the public Decaps, then a copy of the
scratch record before it is cleansed), on inputs from tests/frodo_decrypt_cases.py and on the rows of
tests/golden/frodo_edge.json, whose acceptance is decided by a noise value of th-1, th, -th or -th-1:

* Decode over the whole residue ring and both sides of every threshold (B' = 0, so M = C);
* the product with S^T at and beyond the int16 range ends and one-hot S^T against a ramp B';
* Encaps / Decaps through the public entry points on keys with closed-form noise at a threshold;
* Encaps on public keys with B at the ends of its range.

Bar: byte-exact (integer work).  References: numpy int64 mod q for M, frodo_spec.decode for mu',
oracle.batch_decaps / batch_encaps for ss and ct (held to frodo_spec on these inputs in
tests/test_frodo_edge_oracle.py).  No batch is larger than 1024 rows.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SHAKE_ALGS = ["FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE"]
DECAPS_ALGS = SHAKE_ALGS + ["FrodoKEM-640-AES"]  # re-encryption on the AES Gen(A) path
ALL_ALGS = SHAKE_ALGS + ["FrodoKEM-640-AES", "FrodoKEM-976-AES", "FrodoKEM-1344-AES"]
GOLD = json.loads((Path(__file__).parent / "golden" / "frodo_edge.json").read_text())


@pytest.fixture(scope="module")
def engines():
    from qrkem.batch import BatchKEM
    return {a: BatchKEM(a, device=0) for a in ALL_ALGS}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _trace(eng, sk, ct_):
    """(ss [n, ss_len], mu' [n, 32]) of qrk_dbg_frodo_decaps_trace; mu' is pre-filled so missing writes show."""
    from qrkem._debug import bind
    from qrkem._native import last_error
    LIB = bind()
    n = sk.shape[0]
    assert n <= 1024
    sk_d, ct_d = _dev(sk), _dev(ct_)
    ss = torch.full((n, eng.ss_len), 0xA5, dtype=torch.uint8, device="cuda")
    mu = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    rc = LIB.qrk_dbg_frodo_decaps_trace(eng._ctx, eng.alg.encode(), n, ss.data_ptr(), ct_d.data_ptr(),
                                        sk_d.data_ptr(), mu.data_ptr(), eng._stream())
    assert rc == 0, last_error()
    return _host(ss), _host(mu)


def _first_diff(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} of {len(got)} rows differ, first row {bad[0]}: got {got[bad[0]].tobytes().hex()} " \
           f"want {want[bad[0]].tobytes().hex()}" if len(bad) else ""


# ---------------------------------------------------------------- a. Decode over the whole ring
_RING = {}


def _ring(alg):
    """(sk rows, ct rows, mu' wanted, oracle ss, rows of the ring part), ring rows then threshold rows."""
    if alg not in _RING:
        import frodo_decrypt_cases as D
        import frodo_spec as F
        import oracle as orc
        p = F.params(alg)
        ring, thr = D.ring_rows(p), D.threshold_rows(p)
        assert len(ring) == (1 << p["logq"]) // 64 and len(thr) == 4 << p["B"]
        C = np.concatenate([ring, thr])
        ct_ = D.assemble_ct(p, None, C)
        sk = np.tile(np.frombuffer(D.honest_key(alg)[1], np.uint8), (len(C), 1))
        _RING[alg] = (sk, ct_, D.decode_rows(p, C), orc.batch_decaps(alg, sk, ct_), len(ring))
    return _RING[alg]


@pytest.mark.parametrize("alg", DECAPS_ALGS)
def test_decode_over_the_residue_ring(engines, alg):
    """B' = 0, so M = C: every residue 0..q-1 once (q/64 rows, one batch), then T_m + d for every
    threshold T_m and d = -2, -1, 0, +1 at every position (4 2^B rows, a batch on the cooperative
    sponges).  mu' = frodo_spec.decode; every row rejects with the oracle's ss."""
    sk, ct_, want_mu, want_ss, nring = _ring(alg)
    for lo, hi in ((0, nring), (nring, len(sk))):
        ss, mu = _trace(engines[alg], sk[lo:hi], ct_[lo:hi])
        assert not _first_diff(mu, want_mu[lo:hi]), f"{alg} rows {lo}..{hi}"
        assert np.array_equal(ss, want_ss[lo:hi])


def test_trace_across_chunks(engines):
    """A context chunk of 128 splits the 528 ring and threshold rows of FrodoKEM-640 into five chunks with
    a short tail: every chunk's mu' is copied out before that chunk's scratch is cleansed and reused."""
    from qrkem.batch import BatchKEM
    alg = "FrodoKEM-640-SHAKE"
    sk, ct_, want_mu, want_ss, _ = _ring(alg)
    eng = BatchKEM(alg, device=0, chunk=128)
    assert eng.effective_chunk == 128 and len(sk) == 528
    ss, mu = _trace(eng, sk, ct_)
    assert not _first_diff(mu, want_mu)
    assert np.array_equal(ss, want_ss)
    eng.close()


# ---------------------------------------------------------------- b. the product at its extremes
@pytest.mark.parametrize("alg", DECAPS_ALGS)
def test_product_at_its_extremes(engines, alg):
    """S^T every entry 0x8000, 0x7FFF, +-12 alternating, uniform int16 (B' all q-1 and uniform), and one
    entry +-1 at (k, j), k in {0, 7}, j at the ends of a row, of an 8-value group and of the four j
    quarters, against the ramp B'[i][j] = i n + j; C uniform.  mu' = Decode of the numpy M, ss the oracle's."""
    import frodo_decrypt_cases as D
    import frodo_spec as F
    import oracle as orc
    p = F.params(alg)
    names, St, Bp, C, M = D.product_cases(alg)
    sk, ct_ = D.with_st(p, D.honest_key(alg)[1], St), D.assemble_ct(p, Bp, C)
    want_mu, want_ss = D.decode_rows(p, M), orc.batch_decaps(alg, sk, ct_)
    ss, mu = _trace(engines[alg], sk, ct_)
    bad = [names[i] for i in range(len(names)) if mu[i].tobytes() != want_mu[i].tobytes()]
    assert not bad, f"{alg}: mu' differs on {len(bad)} of {len(names)} rows: {bad[:6]}"
    assert np.array_equal(ss, want_ss)
    assert np.array_equal(_host(engines[alg].decaps(_dev(sk), _dev(ct_))), want_ss)


# ---------------------------------------------------------------- c. acceptance decided at a threshold
_EDGE = {}


def _edge(alg):
    """(pk, sk, mu, accept, closed-form mu' [rows, 32], oracle ct, ss of Encaps, ss of Decaps, fixture rows)
    of the three keys of a set in one batch."""
    if alg not in _EDGE:
        import frodo_decrypt_cases as D
        import frodo_spec as F
        import make_golden_frodo_edge as E
        import oracle as orc
        p, g = F.params(alg), GOLD[alg]
        pks, sks, mus, accs, Ms, rows = [], [], [], [], [], []
        for t, k in enumerate(g["keys"]):
            pk, sk = E.build_key(alg, bytes.fromhex(g["seedA"]), t, k["i0"], k["j0"], k["delta"])
            mu, accept, noise = E.rows_of(alg, k)
            M = np.stack([F.encode(p, m.tobytes()).astype(np.int64) for m in mu])
            M[:, :, k["i0"]] += noise
            pks.append(np.tile(np.frombuffer(pk, np.uint8), (len(mu), 1)))
            sks.append(np.tile(np.frombuffer(sk, np.uint8), (len(mu), 1)))
            mus.append(mu), accs.append(accept), Ms.append(M), rows.extend(k["rows"])
        pk, sk, mu, accept, M = (np.concatenate(x) for x in (pks, sks, mus, accs, Ms))
        ct_, ss = orc.batch_encaps(alg, pk, mu)
        _EDGE[alg] = (pk, sk, mu, accept, D.decode_rows(p, M), ct_, ss, orc.batch_decaps(alg, sk, ct_), rows)
    return _EDGE[alg]


@pytest.mark.parametrize("alg", DECAPS_ALGS)
def test_threshold_rows_encaps(engines, alg):
    """Encaps on the crafted pk (seven all-zero columns of B in k_fr_pack's V = S'B): ct and ss are the
    oracle's, their SHA-256 the fixture's."""
    pk, _, mu, _, _, ct_, ss, _, rows = _edge(alg)
    g_ct, g_ss = engines[alg].encaps(_dev(pk), coins=_dev(mu))
    g_ct, g_ss = _host(g_ct), _host(g_ss)
    assert np.array_equal(g_ct, ct_) and np.array_equal(g_ss, ss)
    for i, r in enumerate(rows):
        assert hashlib.sha256(g_ct[i].tobytes()).hexdigest() == r["ct"]
        assert hashlib.sha256(g_ss[i].tobytes()).hexdigest() == r["ss"]


@pytest.mark.parametrize("alg", DECAPS_ALGS)
def test_threshold_rows_decaps(engines, alg):
    """BatchKEM.decaps: the oracle's ss on every row, the Encaps ss exactly where the accept bit is set."""
    _, sk, _, accept, _, ct_, ss, ss_d, rows = _edge(alg)
    assert accept.sum() >= 16 and (~accept).sum() >= 16
    got = _host(engines[alg].decaps(_dev(sk), _dev(ct_)))
    for i, r in enumerate(rows):  # per row first, so a failure names its noise
        assert got[i].tobytes() == ss_d[i].tobytes(), f"{alg} row {i}: accept={r['accept']} noise={r['noise']}"
    assert np.array_equal((got == ss).all(axis=1), accept)


@pytest.mark.parametrize("alg", DECAPS_ALGS)
def test_threshold_rows_mu(engines, alg):
    """The hook: mu' is mu on accepting rows and frodo_spec.decode of the closed-form M on rejecting ones."""
    _, sk, mu, accept, want_mu, ct_, _, ss_d, rows = _edge(alg)
    ss, got = _trace(engines[alg], sk, ct_)
    assert np.array_equal(want_mu[accept][:, :mu.shape[1]], mu[accept]) and not want_mu[:, mu.shape[1]:].any()
    assert not np.any((want_mu[~accept][:, :mu.shape[1]] == mu[~accept]).all(axis=1))
    for i, r in enumerate(rows):
        assert got[i].tobytes() == want_mu[i].tobytes(), f"{alg} row {i}: accept={r['accept']} noise={r['noise']}"
    assert np.array_equal(ss, ss_d)


# ---------------------------------------------------------------- d. Encaps at the edges of B
@pytest.mark.parametrize("alg", ALL_ALGS)
def test_encaps_on_edge_public_keys(engines, alg):
    """pk = honest seedA with B all q-1, all zero, rows alternating 0 and q-1: ct and ss are the oracle's."""
    import frodo_decrypt_cases as D
    import oracle as orc
    pk = D.edge_pks(alg)
    mu = orc.bench_coins(3, engines[alg].enc_coins, seed=0xED6E)
    want_ct, want_ss = orc.batch_encaps(alg, pk, mu)
    g_ct, g_ss = engines[alg].encaps(_dev(pk), coins=_dev(mu))
    assert np.array_equal(_host(g_ct), want_ct)
    assert np.array_equal(_host(g_ss), want_ss)
