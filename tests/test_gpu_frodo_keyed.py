"""HIP FrodoKEM key sets (csrc/frodo_keyed.hip) against the per-row calls, the C oracle and a plain-arithmetic model.

* Parity: keyed Encaps (ct, ss) and keyed Decaps (ss, status) are byte for byte BatchKEM.encaps / decaps on the
  gathered key rows with the same mu, for all six variants, sets of 1, 2 and 17 keys, the row counts of
  frodo_keyed_cases.ROW_COUNTS (the cooperative-sponge switch at 256, the product kernel's tile of 16) in chunks of
  128, and every index pattern; and the oracle's bytes on the rows of the `mod` pattern.
* Tampered ciphertexts, refused rows, the set's lifecycle, and independence from what the context's buffers held.
* The limb split, the stored layout and the product kernel on chosen matrices and samples, through a probe built from
  the kernels' own header (tests/frodo_keyed_probe.hip -> tests/libfrodo_keyed_probe.so, never part of libqrkem.so).

Bar: byte-exact (integer work).  Outputs the library allocates are compared whole; outputs the tests allocate are
pre-filled with 0xA5, so a missing store shows.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import frodo_keyed_cases as K
import frodo_spec as F
import oracle as orc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FILL = 0xA5
GMAX, NMAX = max(K.SET_SIZES), max(K.ROW_COUNTS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ptr(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _idx(a):
    return _dev(np.asarray(a, np.uint32).view(np.int32))


@functools.lru_cache(maxsize=None)
def keys(alg):
    """17 key pairs from the oracle on fixed seeds, and mu for 257 rows."""
    p = F.params(alg)
    pk, sk = orc.batch_keypair(alg, orc.bench_coins(GMAX, p["keypair_coins"], seed=0xF20D0 + p["n"]))
    return pk, sk, orc.bench_coins(NMAX, p["len_mu"], seed=0xF20D1 + p["n"])


@functools.lru_cache(maxsize=None)
def reference(alg):
    """The per-row calls on every (key, row) pair: ct, ss [17][257] from BatchKEM.encaps with row i's mu, and the
    per-row Decaps of those ciphertexts.  Row i under key k of any keyed call must return entry [k][i]."""
    from qrkem.batch import BatchKEM
    pk, sk, mu = keys(alg)
    eng = BatchKEM(alg, device=0)
    try:
        kk, ii = np.repeat(np.arange(GMAX), NMAX), np.tile(np.arange(NMAX), GMAX)
        c, ss = eng.encaps(_dev(pk[kk]), coins=_dev(mu[ii]))
        dss, st = eng.decaps(_dev(sk[kk]), c, return_status=True)
        c, ss, dss, st = (_host(t) for t in (c, ss, dss, st))
    finally:
        eng.close()
    assert np.array_equal(ss, dss) and not st.any()
    shape = (GMAX, NMAX, -1)
    return c.reshape(shape), ss.reshape(shape)


@pytest.fixture(scope="module")
def engines():
    from qrkem.batch import FrodoBatchKEM
    engs = {a: FrodoBatchKEM(a, device=0, chunk=128) for a in K.ALGS}
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def lib():
    from qrkem._debug import bind
    return bind()


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("g", K.SET_SIZES)
@pytest.mark.parametrize("alg", K.ALGS)
def test_parity_with_the_per_row_calls(engines, alg, g):
    eng = engines[alg]
    pk, sk, mu = keys(alg)
    rct, rss = reference(alg)
    with eng.load_public_keys(pk[:g]) as pub, eng.load_secret_keys(_dev(sk[:g])) as sec:
        for n in K.ROW_COUNTS:
            pats = K.index_patterns(g, n)
            if g == 1:
                pats["NULL"] = None
            rows = np.arange(n)
            for name, idx in pats.items():
                where = f"{alg} g={g} n={n} {name}"
                kk = np.zeros(n, np.int64) if idx is None else idx.astype(np.int64)
                di = None if idx is None else _idx(idx)
                c, ss, st = eng.encaps_keyed(pub, di, n=n, coins=_dev(mu[:n]), return_status=True)
                c_h, ss_h, st_h = _host(c), _host(ss), _host(st)
                assert np.array_equal(c_h, rct[kk, rows]), where + ": Encaps ct"
                assert np.array_equal(ss_h, rss[kk, rows]), where + ": Encaps ss"
                assert not st_h.any(), where + ": Encaps status"
                dss, dst = eng.decaps_keyed(sec, c, di, return_status=True)
                assert np.array_equal(_host(dss), rss[kk, rows]), where + ": Decaps ss"
                assert not _host(dst).any(), where + ": Decaps status"


@pytest.mark.parametrize("alg", K.ALGS)
def test_reference_rows_are_the_oracles(alg):
    """The per-row results the parity test compares with are the oracle's, on the rows of the `mod` pattern for
    17 keys and for one key: every row of the three smallest and the three largest row counts."""
    pk, sk, mu = keys(alg)
    rct, rss = reference(alg)
    rows = np.arange(NMAX)
    for g in (GMAX, 1):
        kk = rows % g
        oc, oss = orc.batch_encaps(alg, pk[kk], mu)
        assert np.array_equal(oc, rct[kk, rows]) and np.array_equal(oss, rss[kk, rows]), f"{alg} g={g}"
        assert np.array_equal(orc.batch_decaps(alg, sk[kk], oc), oss), f"{alg} g={g}"


# ---------------------------------------------------------------- tampered and refused rows
@pytest.mark.parametrize("alg", K.ALGS)
def test_decaps_of_tampered_rows(engines, alg):
    """One bit flipped in B', in C and in the last ct word: the rejection secret built from the set's s."""
    from qrkem.batch import BatchKEM
    eng, p = engines[alg], F.params(alg)
    pk, sk, mu = keys(alg)
    rct, rss = reference(alg)
    g, n = 2, 24
    idx = K.index_patterns(g, n)["mod"]
    kk, rows = idx.astype(np.int64), np.arange(n)
    c = rct[kk, rows].copy()
    lenb = p["logq"] * p["n"]  # bytes of Pack(B')
    flips = {0: (5, 0x10), 1: (lenb + 3, 0x01), 2: (p["ct"] - 1, 0x80)}  # row % 4 -> (byte, bit); row % 4 == 3: valid
    for r in rows:
        if r % 4 in flips:
            c[r, flips[r % 4][0]] ^= flips[r % 4][1]
    per_row = BatchKEM(alg, device=0)
    try:
        want = _host(per_row.decaps(_dev(sk[kk]), _dev(c)))
    finally:
        per_row.close()
    with eng.load_secret_keys(sk[:g]) as sec:
        ss, st = eng.decaps_keyed(sec, _dev(c), _idx(idx), return_status=True)
        ss, st = _host(ss), _host(st)
    assert np.array_equal(ss, want) and not st.any()
    valid = rows % 4 == 3
    assert np.array_equal(ss[valid], rss[kk, rows][valid])
    assert not (ss[~valid] == rss[kk, rows][~valid]).all(axis=1).any()
    assert np.array_equal(want, orc.batch_decaps(alg, sk[kk], c))


@pytest.mark.parametrize("g", [2, 1])
@pytest.mark.parametrize("alg", K.ALGS)
def test_refused_rows(engines, alg, g):
    """Out-of-set indices at the first row, the last row and a tile border: status -1 and zero rows there, every
    other row unchanged.  The outputs are the caller's, pre-filled, through the C calls."""
    from qrkem._native import LIB, last_error
    eng, p = engines[alg], F.params(alg)
    pk, sk, mu = keys(alg)
    rct, rss = reference(alg)
    n = 65
    idx = K.index_patterns(g, n)["zeros"].copy()
    idx[40:] = g - 1  # a set of one key takes the grouping's path without a sort
    bad = [0, K.TILE - 1, K.TILE, n - 1]
    idx[bad] = [g, K.REFUSED, g + 5, 1 << 31]
    kk, rows = np.where(idx < g, idx, 0).astype(np.int64), np.arange(n)
    good = idx < g
    with eng.load_public_keys(pk[:g]) as pub, eng.load_secret_keys(sk[:g]) as sec:
        c = torch.full((n, p["ct"]), FILL, dtype=torch.uint8, device="cuda")
        ss = torch.full((n, p["ss"]), FILL, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
        idx_d, mu_d = _idx(idx), _dev(mu[:n])  # named: a temporary would be freed before the call ran
        rc = LIB.qrk_frodo_encaps_keyed_batch(eng._ctx, pub._handle, n, _ptr(idx_d), _ptr(c), _ptr(ss), _ptr(mu_d),
                                              _ptr(st), eng._stream())
        assert rc == 0, last_error()
        c_h, ss_h, st_h = _host(c), _host(ss), _host(st)
        assert st_h.tolist() == [0 if ok else -1 for ok in good]
        assert not c_h[~good].any() and not ss_h[~good].any()
        assert np.array_equal(c_h[good], rct[kk, rows][good]) and np.array_equal(ss_h[good], rss[kk, rows][good])
        cin = _dev(rct[kk, rows])
        ss.fill_(FILL), st.fill_(FILL)
        rc = LIB.qrk_frodo_decaps_keyed_batch(eng._ctx, sec._handle, n, _ptr(idx_d), _ptr(ss), _ptr(cin), _ptr(st),
                                              eng._stream())
        assert rc == 0, last_error()
        ss_h, st_h = _host(ss), _host(st)
        assert st_h.tolist() == [0 if ok else -1 for ok in good]
        assert not ss_h[~good].any() and np.array_equal(ss_h[good], rss[kk, rows][good])
        assert np.array_equal(_host(cin), rct[kk, rows])  # the input is untouched


# ---------------------------------------------------------------- limbs and layout, through the probe
@pytest.fixture(scope="module")
def probe():
    from pathlib import Path
    path = Path(__file__).resolve().parent / "libfrodo_keyed_probe.so"
    assert path.exists(), f"{path} is missing: build() makes it"
    lib = ct.CDLL(str(path))
    P, SZ = ct.c_void_p, ct.c_size_t
    lib.frk_probe_encrypt.restype = ct.c_int
    lib.frk_probe_encrypt.argtypes = [ct.c_int, SZ, P, P, SZ, P, P, P, P, P, P, ct.c_int]
    lib.frk_probe_tile_rows.restype = ct.c_int
    assert lib.frk_probe_tile_rows() == K.TILE  # the model's tile is the kernel's
    return lib


@pytest.mark.parametrize("alg", K.SHAKE)
def test_limb_and_layout_edges(probe, alg):
    """Chosen A (limb-edge values: constant, one-hot at the corners, on the borders of every tile of the kernel),
    chosen S' (all +max, all -max, alternating, one-hot at the first and last column), every matrix a key of one set
    and neighbouring rows under different keys, two refused rows among them: ct is the plain-arithmetic model's,
    whatever the scratch held."""
    p = F.params(alg)
    rows = K.edge_rows(alg)
    g, n = len(rows["matrices"]), len(rows["labels"])
    index = rows["key_index"].copy()
    refused = [K.TILE, n - 1]
    index[refused] = [g, K.REFUSED]
    pk_d, mat_d, idx_d = _dev(rows["pk"]), _dev(rows["matrices"].view(np.int16)), _idx(index)
    s8_d, e16_d, epp_d, mu_d = (_dev(rows[k]) for k in ("s8", "e16", "epp16", "mu"))
    torch.cuda.synchronize()
    want = None
    for fill in (0xFF, 0x00):
        out = torch.full((n, p["ct"]), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = probe.frk_probe_encrypt(p["n"], g, _ptr(pk_d), _ptr(mat_d), n, _ptr(idx_d), _ptr(s8_d), _ptr(e16_d),
                                     _ptr(epp_d), _ptr(mu_d), _ptr(out), fill)
        assert rc == 0, f"{alg}: hipError_t {rc}"
        got = _host(out)
        if want is None:
            want = [bytes(p["ct"]) if i in refused else
                    K.expected_ct(alg, rows["matrices"][int(index[i])], rows["pk"][int(index[i])].tobytes(),
                                  rows["s8"][i], rows["e16"][i], rows["epp16"][i], rows["mu"][i].tobytes())
                    for i in range(n)]
        for i, label in enumerate(rows["labels"]):
            assert got[i].tobytes() == want[i], f"{alg} fill {fill:#x} row {i}: {label}"
    # a sample outside the sampler's range, or a nonzero pad column, is refused before any launch
    for where, v in (((0, 3, 7), K.SMAX[p["n"]] + 1), ((0, 0, p["n"]), 1)):
        if where[2] >= K.pitch(p["n"]):
            continue  # FrodoKEM-640 has no pad columns
        bad = rows["s8"][:1].copy()
        bad[where] = v
        bad_d, out = _dev(bad), torch.full((1, p["ct"]), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = probe.frk_probe_encrypt(p["n"], g, _ptr(pk_d), _ptr(mat_d), 1, _ptr(idx_d), _ptr(bad_d), _ptr(e16_d),
                                     _ptr(epp_d), _ptr(mu_d), _ptr(out), 0)
        assert rc == -2 and (_host(out) == FILL).all(), (alg, where)


# ---------------------------------------------------------------- lifecycle
@pytest.mark.parametrize("alg", K.ALGS)
def test_set_lifecycle(engines, alg):
    from qrkem._native import LIB, last_error
    eng, p = engines[alg], F.params(alg)
    pk, sk, mu = keys(alg)
    rct, rss = reference(alg)
    n = 9
    rows = np.arange(n)
    a = eng.load_public_keys(pk[:2])            # host keys
    b = eng.load_public_keys(_dev(pk[1:4]))     # device keys; two sets alive at once
    s = eng.load_secret_keys(sk[:2])
    try:
        for ks, g, sec in ((a, 2, False), (b, 3, False), (s, 2, True)):
            assert ks.device_bytes == K.set_bytes(p["n"], sec, g), (alg, g, sec)
            out = (ct.c_size_t * 4)()
            assert LIB.qrk_frodo_keyset_info(ks._handle, out) == 0
            assert list(out) == [g, K.ALGS.index(alg) % 3 * 2 + (1 if alg.endswith("AES") else 0), int(sec),
                                 K.set_bytes(p["n"], sec, g)]
        ia, ib = np.ones(n, np.uint32), np.zeros(n, np.uint32)  # key 1 of a is key 0 of b
        ca, sa = eng.encaps_keyed(a, _idx(ia), coins=_dev(mu[:n]))
        cb, sb = eng.encaps_keyed(b, _idx(ib), coins=_dev(mu[:n]))
        assert np.array_equal(_host(ca), _host(cb)) and np.array_equal(_host(sa), _host(sb))
        assert np.array_equal(_host(ca), rct[1, rows]) and np.array_equal(_host(sa), rss[1, rows])
        # the wrong kind of set, then a closed one: refused by the library and by the wrapper
        buf, ia_d = _dev(np.zeros((n, max(p["ct"], p["ss"])), np.uint8)), _idx(ia)
        rc = LIB.qrk_frodo_encaps_keyed_batch(eng._ctx, s._handle, n, _ptr(ia_d), _ptr(buf), _ptr(buf), None, None,
                                              eng._stream())
        assert rc == -1 and "secret key set cannot encapsulate" in last_error()
        rc = LIB.qrk_frodo_decaps_keyed_batch(eng._ctx, a._handle, n, _ptr(ia_d), _ptr(buf), _ptr(buf), None,
                                              eng._stream())
        assert rc == -1 and "public key set cannot decapsulate" in last_error()
        rc = LIB.qrk_frodo_encaps_keyed_batch(eng._ctx, a._handle, n, None, _ptr(buf), _ptr(buf), None, None,
                                              eng._stream())
        assert rc == -1 and "only for a key set of one key" in last_error()
        assert LIB.qrk_frodo_encaps_keyed_batch(eng._ctx, a._handle, 0, None, None, None, None, None, None) == 0
        with pytest.raises(ValueError, match="secret key set cannot encapsulate"):
            eng.encaps_keyed(s, _idx(ia))
        with pytest.raises(ValueError, match="public key set cannot decapsulate"):
            eng.decaps_keyed(a, ca, _idx(ia))
        b.close()
        assert b.closed and b.device_bytes == 0
        with pytest.raises(ValueError, match="the key set is closed"):
            eng.encaps_keyed(b, _idx(ib))
        # the other sets are as they were
        dss = eng.decaps_keyed(s, ca, _idx(ia))
        assert np.array_equal(_host(dss), rss[1, rows])
    finally:
        for ks in (a, b, s):
            ks.close()


# ---------------------------------------------------------------- independence from prior buffer contents
@pytest.mark.parametrize("alg", ["FrodoKEM-640-SHAKE", "FrodoKEM-976-AES", "FrodoKEM-1344-SHAKE"])
def test_results_do_not_depend_on_what_the_buffers_held(lib, alg):
    """One Encaps and one Decaps on a context whose buffers were filled with 0xFF and then with 0x00 (the scratch is
    sized by a first run, so the fill covers all of it): the reference's bytes each time.  200 rows in chunks of 128:
    a tail chunk that leaves most of the scratch's rows unwritten."""
    from qrkem._native import last_error
    from qrkem.batch import FrodoBatchKEM
    pk, sk, mu = keys(alg)
    rct, rss = reference(alg)
    g, n = 3, 200
    idx = K.index_patterns(g, n)["random"]
    idx[[3, 150]] = g  # refused rows, too
    kk, rows, good = np.where(idx < g, idx, 0).astype(np.int64), np.arange(n), idx < g
    want_c = np.where(good[:, None], rct[kk, rows], 0)
    want_s = np.where(good[:, None], rss[kk, rows], 0)
    eng = FrodoBatchKEM(alg, device=0, chunk=128)
    try:
        with eng.load_public_keys(pk[:g]) as pub, eng.load_secret_keys(sk[:g]) as sec:
            for fill in (None, 0xFF, 0x00):
                if fill is not None:
                    torch.cuda.synchronize()
                    assert lib.qrk_dbg_ctx_fill(eng._ctx, fill) == 0, last_error()
                c, ss, st = eng.encaps_keyed(pub, _idx(idx), coins=_dev(mu[:n]), return_status=True)
                assert np.array_equal(_host(c), want_c) and np.array_equal(_host(ss), want_s), (alg, fill)
                assert np.array_equal(_host(st) == 0, good), (alg, fill)
                if fill is not None:
                    torch.cuda.synchronize()
                    assert lib.qrk_dbg_ctx_fill(eng._ctx, fill) == 0, last_error()
                dss, dst = eng.decaps_keyed(sec, _dev(rct[kk, rows]), _idx(idx), return_status=True)
                assert np.array_equal(_host(dss), want_s) and np.array_equal(_host(dst) == 0, good), (alg, fill)
    finally:
        eng.close()
