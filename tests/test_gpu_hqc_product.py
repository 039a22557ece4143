"""HIP HQC sparse x dense products in F2[X]/(X^n - 1) (build_doubled, build_doubled2_inplace,
sparse_dense, prod_combine in csrc/hqc.hip) at the edges of support and operand, against the
pure-Python spec (oracle/py/hqc_spec.py) and the C oracle.

tests/test_gpu_hqc.py feeds the products pseudo-random operands and tests/test_gpu_hqc_decoder.py
multiplies by u = 0.  Random operands do not reach support position 0 (the only window that lies
wholly in the shifted half of the doubled operand, 1/n per vector), the last operand word
(TOPMASK / NR, the byte mask that cuts the word straddling from u into v) or the stray bits above
X^(n-1); and in Decaps the product leaves the kernel only through a decoder that absorbs dozens
of wrong bits per block.  Here:

* KeyGen (k_hqc_kg_mul) on coins whose y contains position 0 / position n - 1 / a replaced
  duplicate / a position a whole number of words from n (tests/golden/hqc_edge.json);
* Encaps (k_hqc_enc_mul, the two-operand product) on every crafted key pk_seed || s, s a
  dense-edge operand, with coins whose r2 has each of those properties under that key;
* Decaps (k_hqc_decode) on every crafted ciphertext u || v, u a dense-edge operand, with the
  secret keys of the KeyGen records: T = v - u y itself through the test hook
  qrk_dbg_hqc_decaps_trace, the RM symbols and m' of that word, and the public Decaps.

The oracle side of the same records is pinned in tests/test_hqc_edge_oracle.py.
Bar: byte-exact (integer work).
"""
import ctypes as ct
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALGS = ["HQC-128", "HQC-192", "HQC-256"]
GOLD = json.loads((Path(__file__).parent / "golden" / "hqc_edge.json").read_text())
COOP_MAX = 256  # QRK_HQC_COOP_MAX: cooperative sponges up to here, lane kernels above
# neighbouring rows take opposite extremes: a dense s next to a sparse one, all-ones next to zero
ENC_ORDER = ("ones", "zero", "ff", "stray", "aa", "x0", "rand", "xn1", "ones", "x31", "ff", "xw", "aa", "x32",
             "rand", "xw1")


@pytest.fixture(scope="module")
def engines():
    from qrkem.batch import BatchKEM
    return {a: BatchKEM(a, device=0) for a in ALGS}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared references are read-only


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _rows(items):
    return np.stack([np.frombuffer(bytes(b), np.uint8) for b in items])


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


_REF = {}


def _ref(alg):
    """Inputs and expected outputs of one parameter set, computed once and never modified.
    kg: interleaved coins, oracle pk / sk, the rows that are fixture records;
    enc: crafted keys, coins, oracle ct / ss, the fixture digest of every row;
    dec: (sk, ct) rows -- every crafted ciphertext under every sparse-edge secret key -- with the
    spec's T = (v ^ mul_sparse(y, u, n)) & mask, rm_decode_symbol / rs_decode of that word, and
    the oracle's Decaps ss and status."""
    if alg in _REF:
        return _REF[alg]
    import hqc_spec as H
    import make_golden_hqc_edge as E
    import oracle as orc
    p, g = H.params(alg), GOLD[alg]
    s = orc.sizes(alg)
    # KeyGen: ordinary rows between the edge rows
    edge = [bytes.fromhex(r["kp_coins"]) for r in g["kg"]]
    plain = orc.bench_coins(len(edge) + 1, s["keypair_coins"], seed=0xED6E)
    kc = np.stack([plain[i // 2] if i % 2 == 0 else np.frombuffer(edge[i // 2], np.uint8) for i in range(2 * len(edge) + 1)])
    kpk, ksk = orc.batch_keypair(alg, kc)
    kg = dict(coins=kc, pk=kpk, sk=ksk, edge_rows=list(range(1, 2 * len(edge), 2)))
    # Encaps
    digest = {(r["pk"], r["prop"]): r["ct_ss"] for r in g["enc"]}
    labels = [(d, q) for q in E.PROPS for d in ENC_ORDER]
    assert {d for d, _ in labels} == set(E.DENSE)
    epk = _rows(E.edge_pk(alg, d) for d, _ in labels)
    ec = _rows(E.enc_coins(alg, E.theta_class(alg, d), g["enc_counters"][E.theta_class(alg, d)][q]) for d, q in labels)
    ect, ess = orc.batch_encaps(alg, epk, ec)
    enc = dict(labels=labels, pk=epk, coins=ec, ct=ect, ss=ess, digest=[digest[x] for x in labels])
    # Decaps: row = ciphertext-major, so neighbours differ in the secret key
    sks = [ksk[i].tobytes() for i in kg["edge_rows"]]
    ys = [E.secret_y(alg, k) for k in sks]
    cts = [E.edge_ct(alg, u, v) for u, v in E.ct_list(alg)]
    pairs = [(ci, ki) for ci in range(len(cts)) for ki in range(len(sks))]
    t = [E.decode_word(alg, ys[ki], cts[ci]) for ci, ki in pairs]
    span, n1, mult, t2 = p["n2"], p["n1"], p["mult"], 2 * p["delta"]
    memo = {}

    def sym(block):
        if block not in memo:
            memo[block] = H.rm_decode_symbol(block, mult)
        return memo[block]

    syms = [[sym((int.from_bytes(w, "little") >> (span * i)) & ((1 << span) - 1)) for i in range(n1)] for w in t]
    mp = [bytes(H.rs_decode(p, r)[t2:]) for r in syms]
    dsk, dct = _rows(sks[ki] for _, ki in pairs), _rows(cts[ci] for ci, _ in pairs)
    dss, dst = orc.batch_decaps(alg, dsk, dct, with_status=True)
    for ki, d in enumerate(g["decaps"]):  # the fixture's digests, per secret key in ciphertext order
        mine = [i for i, (_, k) in enumerate(pairs) if k == ki]
        assert _sha(b"".join(t[i] for i in mine)) == d["t"] and dst[mine].tolist() == d["status"]
        assert _sha(dss[mine].tobytes()) == d["ss"]
    dec = dict(labels=[(E.ct_list(alg)[ci], E.PROPS[ki]) for ci, ki in pairs], sk=dsk, ct=dct, t=_rows(t),
               syms=np.array(syms, np.uint8), mp=_rows(mp), ss=dss, st=dst)
    for d in (kg, enc, dec):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    _REF[alg] = (kg, enc, dec)
    return _REF[alg]


def _first_bad(got, want, labels):
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    if not bad:
        return ""
    i = bad[0]
    diff = np.flatnonzero(got[i] != want[i])
    return f"{len(bad)} of {len(want)} rows differ, first row {i} {labels[i]}: {len(diff)} bytes from byte {diff[0]}"


# ---------------------------------------------------------------- KeyGen
@pytest.mark.parametrize("alg", ALGS)
def test_keygen_sparse_edges(engines, alg):
    """s = x + y h with y at each sparse edge, between ordinary rows: pk and sk byte-exact against
    the oracle and the fixture's digests; each edge row alone (n = 1) and tiled past
    QRK_HQC_COOP_MAX gives the same bytes."""
    kg, _, _ = _ref(alg)
    eng = engines[alg]
    labels = ["plain" if i % 2 == 0 else GOLD[alg]["kg"][i // 2]["prop"] for i in range(len(kg["coins"]))]
    pk, sk = map(_host, eng.keypair(coins=_dev(kg["coins"])))
    assert not _first_bad(pk, kg["pk"], labels) and not _first_bad(sk, kg["sk"], labels)
    for r, i in zip(GOLD[alg]["kg"], kg["edge_rows"]):
        assert (_sha(pk[i]), _sha(sk[i])) == (r["pk"], r["sk"]), r["prop"]
        pk1, sk1 = map(_host, eng.keypair(coins=_dev(kg["coins"][i:i + 1])))
        assert np.array_equal(pk1[0], kg["pk"][i]) and np.array_equal(sk1[0], kg["sk"][i]), r["prop"]
    idx = np.arange(260) % len(kg["coins"])
    assert len(idx) > COOP_MAX
    pk, sk = map(_host, eng.keypair(coins=_dev(kg["coins"][idx])))
    assert not _first_bad(pk, kg["pk"][idx], [labels[i] for i in idx])
    assert not _first_bad(sk, kg["sk"][idx], [labels[i] for i in idx])


# ---------------------------------------------------------------- Encaps
def _encaps_check(eng, enc, idx):
    ct_, ss = map(_host, eng.encaps(_dev(enc["pk"][idx]), coins=_dev(enc["coins"][idx])))
    labels = [enc["labels"][i] for i in idx]
    assert not _first_bad(ct_, enc["ct"][idx], labels), _first_bad(ct_, enc["ct"][idx], labels)
    assert not _first_bad(ss, enc["ss"][idx], labels), _first_bad(ss, enc["ss"][idx], labels)
    return ct_, ss


@pytest.mark.parametrize("alg", ALGS)
def test_encaps_dense_and_sparse_edges(engines, alg):
    """u = r1 + r2 h, v = mG + r2 s + e for every (dense-edge s, sparse-edge r2): ct and ss
    byte-exact against the oracle and the fixture's digests, neighbouring rows at opposite
    extremes."""
    _, enc, _ = _ref(alg)
    d = [x for x, _ in enc["labels"]]
    assert all(a != b for a, b in zip(d, d[1:])) and ("ones", "zero") in set(zip(d, d[1:]))
    ct_, ss = _encaps_check(engines[alg], enc, np.arange(len(d)))
    for i, want in enumerate(enc["digest"]):
        assert _sha(ct_[i].tobytes() + ss[i].tobytes()) == want, enc["labels"][i]


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("shape", ["one", "ragged", "tiled"])
def test_encaps_batch_shapes(engines, alg, shape):
    """The same records alone (n = 1: every position-0 row and every all-0xFF row), as a ragged
    batch of 61 in another order, and tiled to 260 (the lane-per-handshake sponges)."""
    _, enc, _ = _ref(alg)
    n = len(enc["labels"])
    if shape == "one":
        for i in [i for i, (d, q) in enumerate(enc["labels"]) if q == "pos0" or d == "ff"]:
            _encaps_check(engines[alg], enc, np.array([i]))
    elif shape == "ragged":
        _encaps_check(engines[alg], enc, (np.arange(61) * 37 + 5) % n)
    else:
        _encaps_check(engines[alg], enc, np.arange(260) % n)


# ---------------------------------------------------------------- Decaps
def _trace_check(eng, dec, idx):
    """qrk_dbg_hqc_decaps_trace on the rows idx: T, syms and m' against the spec's, row by row."""
    t, syms, mp = map(_host, eng.hqc_decaps_trace(_dev(dec["sk"][idx]), _dev(dec["ct"][idx])))
    labels = [dec["labels"][i] for i in idx]
    assert not _first_bad(t, dec["t"][idx], labels), _first_bad(t, dec["t"][idx], labels)
    assert not _first_bad(syms, dec["syms"][idx], labels), _first_bad(syms, dec["syms"][idx], labels)
    assert not _first_bad(mp, dec["mp"][idx], labels), _first_bad(mp, dec["mp"][idx], labels)
    return syms, mp


@pytest.mark.parametrize("alg", ALGS)
def test_decaps_product_word(engines, alg):
    """T = v - u y as k_hqc_decode hands it to the RM stage, for every dense-edge u (v zero, all
    0xFF and random; the (ff, zero) / (zero, ff) pair across the u | v cut) under the secret keys
    whose y has each sparse property: t_out equals the spec's word byte for byte, syms and m'
    are rm_decode_symbol / rs_decode of it, and qrk_hqc_code_decode returns the same two."""
    _, _, dec = _ref(alg)
    cut = {(c, k) for c, k in dec["labels"] if c in (("ff", "zero"), ("zero", "ff"))}
    assert len(cut) == 8
    idx = np.arange(len(dec["labels"]))
    syms, mp = _trace_check(engines[alg], dec, idx)
    s2, m2 = map(_host, engines[alg].hqc_code_decode(_dev(dec["sk"]), _dev(dec["ct"])))
    assert np.array_equal(s2, syms) and np.array_equal(m2, mp)


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("shape", ["one", "ragged", "tiled"])
def test_decaps_trace_batch_shapes(engines, alg, shape):
    """A row's trace does not depend on the batch around it: every fifth row alone (n = 1), a
    ragged batch of 71 in another order, the list tiled to 260."""
    _, _, dec = _ref(alg)
    n = len(dec["labels"])
    if shape == "one":
        for i in range(0, n, 5):
            _trace_check(engines[alg], dec, np.array([i]))
    elif shape == "ragged":
        _trace_check(engines[alg], dec, (np.arange(71) * 29 + 3) % n)
    else:
        idx = np.arange(260) % n
        assert len(idx) > COOP_MAX
        _trace_check(engines[alg], dec, idx)


@pytest.mark.parametrize("alg", ALGS)
def test_decaps_public_path(engines, alg):
    """Plain Decaps on the same rows, as they are and tiled to 260: the oracle's ss and status
    (the re-encryption under these keys rejects, so ss = K(sigma || u || v))."""
    _, _, dec = _ref(alg)
    for idx in (np.arange(len(dec["labels"])), np.arange(260) % len(dec["labels"])):
        ss, st = map(_host, engines[alg].decaps(_dev(dec["sk"][idx]), _dev(dec["ct"][idx]), return_status=True))
        assert np.array_equal(st, dec["st"][idx])
        labels = [dec["labels"][i] for i in idx]
        assert not _first_bad(ss, dec["ss"][idx], labels), _first_bad(ss, dec["ss"][idx], labels)


@pytest.mark.parametrize("alg", ALGS)
def test_chunk_below_batch(alg):
    """A context chunk of 64 under ragged batches of 70: KeyGen, Encaps and Decaps run in two
    chunks and give the same bytes."""
    from qrkem.batch import BatchKEM
    kg, enc, dec = _ref(alg)
    eng = BatchKEM(alg, device=0, chunk=64)
    chunk = eng.effective_chunk
    assert chunk < 70
    idx = np.arange(70) % len(kg["coins"])
    pk, sk = map(_host, eng.keypair(coins=_dev(kg["coins"][idx])))
    assert np.array_equal(pk, kg["pk"][idx]) and np.array_equal(sk, kg["sk"][idx])
    _encaps_check(eng, enc, (np.arange(70) * 11) % len(enc["labels"]))
    idx = (np.arange(70) * 13) % len(dec["labels"])
    ss, st = map(_host, eng.decaps(_dev(dec["sk"][idx]), _dev(dec["ct"][idx]), return_status=True))
    assert np.array_equal(st, dec["st"][idx]) and np.array_equal(ss, dec["ss"][idx])
    _trace_check(eng, dec, idx[:chunk])  # the hook itself takes one chunk at most


# ---------------------------------------------------------------- the hook's argument checks
def test_trace_rejects_oversize_batch_and_unknown_algorithm():
    """More records than the context chunk, a name that is no parameter set and a parameter set
    that is not HQC are errors, and nothing is launched: the outputs keep their fill."""
    from qrkem._debug import bind
    from qrkem._native import last_error
    from qrkem.batch import BatchKEM
    LIB = bind()
    eng = BatchKEM("HQC-128", device=0, chunk=64)
    n = eng.effective_chunk + 1
    sk = torch.zeros((n, eng.sk_len), dtype=torch.uint8, device="cuda")
    c = torch.zeros((n, eng.ct_len), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="chunk"):
        eng.hqc_decaps_trace(sk, c)
    outs = [torch.full((n, w), 0xA5, dtype=torch.uint8, device="cuda") for w in (2208, 46, 16)]
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(alg, rows):
        return LIB.qrk_dbg_hqc_decaps_trace(eng._ctx, alg, rows, sk.data_ptr(), c.data_ptr(), outs[0].data_ptr(),
                                            outs[1].data_ptr(), outs[2].data_ptr(), stream)

    assert call(b"HQC-128", n) == -1 and "chunk" in last_error()
    assert call(b"HQC-512", 1) == -1
    assert call(b"ML-KEM-768", 1) == -1 and "not an HQC parameter set" in last_error()
    assert LIB.qrk_dbg_hqc_decaps_trace(eng._ctx, b"HQC-128", 1, sk.data_ptr(), c.data_ptr(), None, outs[1].data_ptr(),
                                        outs[2].data_ptr(), stream) == -1 and "null buffer" in last_error()
    assert all(bool((_host(o) == 0xA5).all()) for o in outs)
    assert call(b"HQC-128", 1) == 0, last_error()  # the same call within the chunk runs
    assert not (_host(outs[0])[0] == 0xA5).all() and (_host(outs[0])[1:] == 0xA5).all()
