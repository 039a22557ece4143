"""HIP FrodoKEM forward path (KeyGen, Encaps and the same kernels inside Decaps' re-encryption) at its edges.

Every other GPU test reaches these kernels with honest keys and hash-derived samples, and looks at the final bytes.
Here (inputs and references: tests/frodo_forward_cases.py, held to the specification on the CPU by
tests/test_frodo_forward_cases.py):

* k_fr_sample alone, through qrk_dbg_frodo_sample: every 16-bit word, and the words on both sides of every CDF table
  entry placed at the first and last index of every output region, for the three tables in both instantiations;
* Gen(A) fused with S'A / A S, k_fr_pack and k_fr_kg_pack on crafted sample matrices, through
  qrk_dbg_frodo_from_samples: every entry at the sampler's extreme, alternating signs, one-hot at the tile borders;
* Encaps on attacker-chosen public keys and Decaps on secret keys with S^T at the int16 ends and ciphertext fields
  all-zero / all-ones, through the public calls, against the C oracle.

Bar: byte-exact (integer work).  The hooks' outputs are pre-filled, so a missing store shows.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import frodo_forward_cases as W
import frodo_spec as F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FILL = 0xA5
SHAKE = [a for a in W.ALGS if a.endswith("SHAKE")]
TILED = {640: 257, 976: 70, 1344: 70}  # 257: past the 256-handshake cooperative sponges and the Gen(A) sub-chunk


@pytest.fixture(scope="module")
def lib():
    from qrkem._debug import bind
    return bind()


@pytest.fixture(scope="module")
def engines():
    from qrkem.batch import BatchKEM
    engs = {a: BatchKEM(a, device=0) for a in W.ALGS}
    yield engs
    for e in engs.values():
        e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _out(shape, dtype):
    return torch.full(shape, FILL, dtype=dtype, device="cuda")  # int8: 0xA5 wraps; int16: 0x00A5 -- neither is a sample


def _ptr(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def run_sample(lib, eng, kg, words_d, dirty=False):
    """qrk_dbg_frodo_sample on device words [rows, words_per_row] -> device (s8, e16, epp16 or None).  dirty: every
    buffer of the context is filled with 0xFF first, so a pad column the sampler did not zero is not zero by luck."""
    from qrkem._native import last_error
    p = F.params(eng.alg)
    rows = words_d.shape[0]
    if dirty:
        assert lib.qrk_dbg_ctx_fill(eng._ctx, 0xFF) == 0, last_error()
    s8 = torch.full((rows, 8, W.pitch(p["n"])), -91, dtype=torch.int8, device="cuda")
    e16, epp = _out((rows, 8 * p["n"]), torch.int16), (None if kg else _out((rows, 64), torch.int16))
    rc = lib.qrk_dbg_frodo_sample(eng._ctx, eng.alg.encode(), int(kg), rows, _ptr(words_d), _ptr(s8), _ptr(e16),
                                  _ptr(epp), eng._stream())
    assert rc == 0, last_error()
    return s8, e16, epp


def run_from_samples(lib, eng, kg, inp, idx):
    """qrk_dbg_frodo_from_samples on the cases idx of from_samples_inputs -> host rows (Encaps: ct; KeyGen: pk, sk)."""
    from qrkem._native import last_error
    p = F.params(eng.alg)
    n = len(idx)
    s8, e16 = _dev(inp["s8"][idx]), _dev(inp["e16"][idx])
    if kg:
        src, epp, mu = _dev(inp["seedA"][idx]), None, None
        out, sk = _out((n, p["pk"]), torch.uint8), _out((n, p["sk"]), torch.uint8)
    else:
        src, epp, mu = _dev(inp["pk"][idx]), _dev(inp["epp16"][idx]), _dev(inp["mu"][idx])
        out, sk = _out((n, p["ct"]), torch.uint8), None
    rc = lib.qrk_dbg_frodo_from_samples(eng._ctx, eng.alg.encode(), int(kg), n, _ptr(s8), _ptr(e16), _ptr(epp),
                                        _ptr(src), _ptr(mu), _ptr(out), _ptr(sk), eng._stream())
    assert rc == 0, last_error()
    return (_host(out), _host(sk)) if kg else _host(out)


# ---------------------------------------------------------------- 1. the sampler alone
def _sampler_mismatch(p, kg, got, want, row_label=lambda r: f"row {r}"):
    """'' or a message naming the first differing region and entry."""
    for name, g, w in zip(("S" if not kg else "S^T", "E'" if not kg else "E", "E''"), got, want):
        if w is None:
            continue
        g = _host(g).reshape(w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            pad = name.startswith("S") and len(bad) == 3 and bad[2] >= p["n"]
            return (f"{row_label(bad[0])}: region {name}{' pad column' if pad else ''} index {tuple(int(b) for b in bad[1:])}: "
                    f"got {int(g[tuple(bad)])} want {int(w[tuple(bad)])}")
    return ""


@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
@pytest.mark.parametrize("kg", [False, True], ids=["encaps", "keygen"])
@pytest.mark.parametrize("alg", SHAKE)
def test_sampler_on_every_word(lib, engines, alg, kg, shuffled):
    """All 65,536 words over 7 / 5 / 4 rows: S' (pad columns included), E' and E'' are frodo_spec.sample's."""
    p = F.params(alg)
    words = W.every_word_rows(p, kg, shuffled)
    words_d = _dev(words.view(np.int16))
    run_sample(lib, engines[alg], kg, words_d)  # sizes the scratch, which the fill below then covers
    got = run_sample(lib, engines[alg], kg, words_d, dirty=True)
    msg = _sampler_mismatch(p, kg, got, W.sampler_expected(p, kg, words))
    assert not msg, f"{alg}: {msg}"


@pytest.mark.parametrize("kg", [False, True], ids=["encaps", "keygen"])
@pytest.mark.parametrize("alg", SHAKE)
def test_sampler_at_every_table_boundary(lib, engines, alg, kg):
    """2T[j] .. 2T[j]+3 for every table entry and 0, 1, 0xFFFE, 0xFFFF, each alone in a zero stream at the first and
    last index of every region: at n = 1, and as row 1 and the last row of a batch of 3 behind a zero row."""
    p = F.params(alg)
    words, meta = W.boundary_streams(p, kg)
    want = W.sampler_expected(p, kg, words)
    # the table says what the spec's sampler gives at the placed word, and zero elsewhere
    flat = np.concatenate([want[0][:, :, :p["n"]].reshape(len(meta), -1).astype(np.int64), want[1].astype(np.int64)]
                          + ([] if kg else [want[2].astype(np.int64)]), axis=1)
    for i, (label, region, idx, v) in enumerate(meta):
        assert flat[i, idx] == v and np.count_nonzero(flat[i]) == (v != 0), (label, region)
    words_d = _dev(np.concatenate([np.zeros((1, words.shape[1]), np.uint16), words]).view(np.int16))  # row 0: zeros
    M = len(meta)

    def label(i):
        return f"{meta[i][0]} at {meta[i][1]} (sample {meta[i][3]})"

    run_sample(lib, engines[alg], kg, words_d[:3])  # sizes the scratch for both shapes
    for i in range(M):
        got = run_sample(lib, engines[alg], kg, words_d[1 + i:2 + i], dirty=i == 0)
        msg = _sampler_mismatch(p, kg, got, [None if w is None else w[i:i + 1] for w in want])
        assert not msg, f"{alg} n=1, {label(i)}: {msg}"
    zero = [None if w is None else np.zeros_like(w[:1]) for w in want]
    for i in range(M):
        j = (i + 1) % M
        rows = torch.tensor([0, 1 + i, 1 + j], device="cuda")
        got = run_sample(lib, engines[alg], kg, words_d[rows].contiguous(), dirty=i == 0)
        exp = [None if w is None else np.concatenate([z, w[i:i + 1], w[j:j + 1]]) for z, w in zip(zero, want)]
        msg = _sampler_mismatch(p, kg, got, exp, lambda r: ("zero row", label(i), label(j))[r] + f" (row {r} of 3)")
        assert not msg, f"{alg} n=3: {msg}"


# ---------------------------------------------------------------- 2. products and packing from crafted samples
@functools.lru_cache(maxsize=None)
def _gold():
    import make_golden_frodo_forward as G
    return G.load()


def _expected(alg, kg):
    """(names, digests of the expected rows from the fixture, the rows themselves where A is cheap: the SHAKE names)."""
    inp = W.from_samples_inputs(alg, kg)
    d = _gold()[alg]["keygen" if kg else "encaps"]
    assert list(d) == inp["names"] and _gold()[alg]["seedA"] == W.seed_a(alg).hex()
    rows = W.from_samples_expected(alg, kg) if alg.endswith("SHAKE") else None
    if rows is not None:
        assert W.digests(rows) == list(d.values())
    return inp, list(d.values()), rows


def _check_rows(alg, kg, what, inp, want_digest, want_rows, idx, got):
    for r, i in enumerate(idx):
        if want_rows is not None and not np.array_equal(got[r], want_rows[i]):
            bad = np.nonzero(got[r] != want_rows[i])[0]
            raise AssertionError(f"{alg} {'keygen' if kg else 'encaps'} {what} row {r}, case {inp['names'][i]}: "
                                 f"{len(bad)} bytes differ, first at {bad[0]} of {len(got[r])}")
    assert W.digests(got) == [want_digest[i] for i in idx], \
        (alg, what, [inp["names"][i] for r, i in enumerate(idx) if W.digests(got[r:r + 1])[0] != want_digest[i]][:6])


def _check_sk(alg, inp, idx, pk, sk):
    """KeyGen mode: k_fr_kg_pack's part of sk is the pk copy and S^T as int16; s and pkh keep the fill."""
    p = F.params(alg)
    sec, n = p["sec"], p["n"]
    assert np.array_equal(sk[:, sec:sec + p["pk"]], pk)
    assert np.array_equal(sk[:, sec + p["pk"]:sec + p["pk"] + 16 * n], W.keygen_sk_part(alg)[idx])
    assert (sk[:, :sec] == FILL).all() and (sk[:, -sec:] == FILL).all()


@pytest.mark.parametrize("kg", [False, True], ids=["encaps", "keygen"])
@pytest.mark.parametrize("alg", W.ALGS)
def test_from_samples_each_case_alone(lib, engines, alg, kg):
    inp, dig, rows = _expected(alg, kg)
    for i in range(len(dig)):
        got = run_from_samples(lib, engines[alg], kg, inp, [i])
        if kg:
            _check_sk(alg, inp, [i], *got)
            got = got[0]
        _check_rows(alg, kg, "n=1", inp, dig, rows, [i], got)


@pytest.mark.parametrize("kg", [False, True], ids=["encaps", "keygen"])
@pytest.mark.parametrize("alg", W.ALGS)
def test_from_samples_batches(lib, engines, alg, kg):
    """All cases in one ragged batch (39 rows, neighbours at opposite extremes), then tiled to 257 / 70 rows."""
    inp, dig, rows = _expected(alg, kg)
    for total in (len(dig), TILED[F.params(alg)["n"]]):
        idx = W.tiled(len(dig), total)
        got = run_from_samples(lib, engines[alg], kg, inp, idx)
        if kg:
            _check_sk(alg, inp, idx, *got)
            got = got[0]
        _check_rows(alg, kg, f"n={total}", inp, dig, rows, idx, got)


def test_hooks_check_their_arguments_before_any_launch(lib, engines):
    """Unknown name, a name of another family, n above the context chunk, a null buffer, a sample outside the
    sampler's range, a nonzero pad column: -1, and the outputs keep their fill."""
    import qrkem
    from qrkem.batch import BatchKEM
    alg = "FrodoKEM-976-SHAKE"
    p, eng = F.params(alg), BatchKEM("FrodoKEM-976-SHAKE", device=0, chunk=64)
    inp = W.from_samples_inputs(alg, False)
    n = 65
    idx = W.tiled(len(inp["names"]), n)
    words = _dev(np.zeros((n, W.words_per_row(p, False)), np.int16))
    s8, e16, epp = _dev(inp["s8"][idx]), _dev(inp["e16"][idx]), _dev(inp["epp16"][idx])
    pk, mu = _dev(inp["pk"][idx]), _dev(inp["mu"][idx])
    o8 = torch.full((n, 8, W.pitch(p["n"])), -91, dtype=torch.int8, device="cuda")
    o16, opp, out = _out((n, 8 * p["n"]), torch.int16), _out((n, 64), torch.int16), _out((n, p["ct"]), torch.uint8)
    st = eng._stream()

    def sample(name, rows, w=words, a=o8):
        return lib.qrk_dbg_frodo_sample(eng._ctx, name, 0, rows, _ptr(w), _ptr(a), _ptr(o16), _ptr(opp), st)

    def from_samples(name, rows, s=s8, o=out):
        return lib.qrk_dbg_frodo_from_samples(eng._ctx, name, 0, rows, _ptr(s), _ptr(e16), _ptr(epp), _ptr(pk), _ptr(mu),
                                              _ptr(o), None, st)

    a = alg.encode()
    for call in (sample, from_samples):
        for name, rows, kw, msg in ((b"FrodoKEM-976", 1, {}, "unsupported KEM"),
                                    (b"ML-KEM-768", 1, {}, "not a FrodoKEM parameter set"),
                                    (b"HQC-128", 1, {}, "not a FrodoKEM parameter set"),
                                    (a, n, {}, "n exceeds the context chunk")):
            assert call(name, rows, **kw) == -1
            assert msg in qrkem.last_error()
    assert sample(a, 1, a=None) == -1 and "null buffer" in qrkem.last_error()
    assert from_samples(a, 1, o=None) == -1 and "null buffer" in qrkem.last_error()
    for where, v in (((0, 0, 0), W.smax(p) + 1), ((0, 7, p["n"] - 1), -W.smax(p) - 1), ((0, 3, p["n"]), 1)):
        bad = inp["s8"][idx[:2]].copy()
        bad[where] = v
        assert from_samples(a, 2, s=_dev(bad)) == -1 and "sampler range" in qrkem.last_error()
    torch.cuda.synchronize()
    assert (_host(o8) == -91).all() and (_host(o16) == FILL).all() and (_host(opp) == FILL).all()
    assert (_host(out) == FILL).all()
    # and within the chunk both run
    assert sample(a, 64) == 0 and from_samples(a, 64) == 0, qrkem.last_error()
    assert np.array_equal(_host(out)[:64], W.from_samples_expected(alg, False)[idx[:64]])
    eng.close()


# ---------------------------------------------------------------- 3. crafted keys through the public calls
@functools.lru_cache(maxsize=None)
def _encaps_ref(alg):
    import oracle as orc
    r = W.encaps_rows(alg)
    return r, orc.batch_encaps(alg, r["pk"], r["mu"])


@functools.lru_cache(maxsize=None)
def _decaps_ref(alg):
    import oracle as orc
    r = W.decaps_rows(alg)
    ss, st = orc.batch_decaps(alg, r["sk"], r["ct"], with_status=True)
    accepted = (ss == r["ss_enc"]).all(axis=1)
    tampered = np.array([b != "honest" or c != "honest" for _, _, b, c in r["plan"]])
    assert accepted[0] and not accepted[tampered].any()  # pinned against frodo_spec in test_frodo_forward_cases.py
    return r, ss, st


def _batches(alg, count):
    n = F.params(alg)["n"]
    return [W.tiled(count, 70)] + ([W.tiled(count, 257)] if n == 640 else [])


@pytest.mark.parametrize("alg", W.ALGS)
def test_encaps_on_crafted_public_keys(engines, alg):
    """B all 0, all q-1, all q/2, striped by row and by column, 0x5555 / 0x2AAA, one-hot q-1 at three corners, random,
    an honest key after each: ct and ss are the C oracle's, each row alone, 70 ragged and 257 for the 640 sets."""
    r, (want_ct, want_ss) = _encaps_ref(alg)
    for idx in [[i] for i in range(len(r["names"]))] + _batches(alg, len(r["names"])):
        idx = np.asarray(idx)
        g_ct, g_ss = engines[alg].encaps(_dev(r["pk"][idx]), coins=_dev(r["mu"][idx]))
        g_ct, g_ss = _host(g_ct), _host(g_ss)
        bad = [r["names"][i] for k, i in enumerate(idx) if not np.array_equal(g_ct[k], want_ct[i])]
        assert not bad, f"{alg} n={len(idx)}: ct differs under {bad[:6]}"
        assert np.array_equal(g_ss, want_ss[idx]), f"{alg} n={len(idx)}"


@pytest.mark.parametrize("alg", W.ALGS)
def test_decaps_on_crafted_secret_keys(engines, alg):
    """sk = s || crafted pk || S^T || H(pk) with S^T honest / 0x7FFF / 0x8000 / 0xFFFF; the honest Encaps under the
    crafted pk and ciphertexts whose B' and / or C are all-zero or all-ones: ss and status are the C oracle's."""
    r, want_ss, want_st = _decaps_ref(alg)
    for idx in [[i] for i in range(len(r["names"]))] + _batches(alg, len(r["names"])):
        idx = np.asarray(idx)
        ss, st = engines[alg].decaps(_dev(r["sk"][idx]), _dev(r["ct"][idx]), return_status=True)
        ss, st = _host(ss), _host(st)
        bad = [r["names"][i] for k, i in enumerate(idx) if not np.array_equal(ss[k], want_ss[i])]
        assert not bad, f"{alg} n={len(idx)}: ss differs on {bad[:6]}"
        assert np.array_equal(st, want_st[idx])


@pytest.mark.parametrize("alg", ["FrodoKEM-976-SHAKE", "FrodoKEM-640-AES"])
def test_crafted_keys_across_chunks(alg):
    """BatchKEM(alg, chunk=64) on 70 rows: two chunks of one call, the second of six rows."""
    from qrkem.batch import BatchKEM
    eng = BatchKEM(alg, device=0, chunk=64)
    assert eng.effective_chunk == 64
    r, (want_ct, want_ss) = _encaps_ref(alg)
    idx = W.tiled(len(r["names"]), 70)
    g_ct, g_ss = eng.encaps(_dev(r["pk"][idx]), coins=_dev(r["mu"][idx]))
    assert np.array_equal(_host(g_ct), want_ct[idx]) and np.array_equal(_host(g_ss), want_ss[idx])
    d, d_ss, d_st = _decaps_ref(alg)
    idx = W.tiled(len(d["names"]), 70)
    ss, st = eng.decaps(_dev(d["sk"][idx]), _dev(d["ct"][idx]), return_status=True)
    assert np.array_equal(_host(ss), d_ss[idx]) and np.array_equal(_host(st), d_st[idx])
    eng.close()
