"""HIP FrodoKEM / HQC Decaps: the re-encryption compare, hit at every word of the ciphertext.

Decaps decrypts, re-encrypts and compares with the received ciphertext; for a one-bit change that the
decryption absorbs, that compare (step 4 of k_fr_pack<N, 1>; the REENC branch of k_hqc_enc_mul: the
register / LDS paths of u, the masked word that u and v share, v's unaligned words) is the only thing
that rejects.  The rows of tests/fo_compare_cases.py flip one bit in every 64-bit word of a FrodoKEM
ciphertext (`silent`: absorbed by Decode; `cycle`: every bit position of the word; `ends`: every bit of
the first / last words of Pack(B') and Pack(C)) and in every 32-bit word of HQC's u and v (`word`), every
bit around the u | v and v | salt boundaries (`edge`) and every salt byte (`salt`);
tests/test_fo_compare_cases.py holds those rows to the specs and the C oracle.

Per parameter set and family, on device tensors, sk tiled, in calls of at most 1024 rows, the first of
at most 256 (cooperative sponges; the later ones run the lane kernels), each call with the honest
ciphertext as its first, middle and last row:
* every tampered row is rejected with the closed-form secret -- FrodoKEM ss = SHAKE(ct_bad || s), HQC
  status -1 and ss = K(sigma || u || v) of the tampered ciphertext (hashlib) -- which is also
  oracle.batch_decaps' on every 16th row and on all `ends` / `edge` / `salt` rows;
* no tampered row returns the honest ss, and the three honest rows do (HQC: status 0);
* the decryption did absorb the flip: mu' (qrk_dbg_frodo_decaps_trace) is the honest mu on every
  `silent` row, m' (qrk_hqc_code_decode) the honest m on every HQC row.
Bar: byte-exact.  A failure names the family, the byte, the bit and the compare unit.
"""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fo_compare_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

CALL = 1024   # rows per call at most
COOP = 256    # QRK_FR_COOP_MAX = QRK_HQC_COOP_MAX: cooperative sponges up to here
ORACLE_STRIDE = 16
CASES = [(a, f) for a in K.FRODO_ALGS + K.HQC_ALGS for f in K.FAMILIES[a]]


@pytest.fixture(scope="module")
def engines():
    from qrkem.batch import BatchKEM
    return {a: BatchKEM(a, device=0) for a in K.FRODO_ALGS + K.HQC_ALGS}


_SK = {}


def _sk_dev(alg, n):
    """The honest sk tiled to n <= CALL rows on the device (one upload per parameter set)."""
    if alg not in _SK:
        _SK[alg] = torch.from_numpy(np.tile(np.frombuffer(K.honest(alg)["sk"], np.uint8), (CALL, 1))).cuda()
    return _SK[alg][:n]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _calls(nbad):
    """[lo, hi) of the tampered rows of each call: three honest rows go with them, so COOP - 3 in the
    first call and at most CALL - 3 in the others."""
    cuts = [0, min(nbad, COOP - 3)]
    while cuts[-1] < nbad:
        cuts.append(min(nbad, cuts[-1] + CALL - 3))
    return list(zip(cuts, cuts[1:]))


def _with_honest(alg, bad):
    """(ct rows, index of the tampered rows in them): honest | first half | honest | second half | honest."""
    ct = np.frombuffer(K.honest(alg)["ct"], np.uint8)[None]
    h = len(bad) // 2
    idx = np.r_[1:1 + h, 2 + h:2 + len(bad)]
    return np.concatenate([ct, bad[:h], ct, bad[h:], ct]), idx


def _closed_form(alg, bad):
    """The rejection secret of every tampered row, from hashlib alone."""
    sk = K.honest(alg)["sk"]
    if alg.startswith("Frodo"):
        p = K.F.params(alg)
        xof = hashlib.shake_128 if p["n"] == 640 else hashlib.shake_256
        s = sk[:p["sec"]]
        return np.stack([np.frombuffer(xof(r.tobytes() + s).digest(p["ss"]), np.uint8) for r in bad])
    p = K.H.params(alg)
    sigma = sk[K.H.SEED_BYTES:K.H.SEED_BYTES + p["k"]]
    uv = p["nb"] + p["vb"]
    return np.stack([np.frombuffer(K.H.shake_ds(sigma + r[:uv].tobytes(), K.H.D_K), np.uint8) for r in bad])


def _frodo_trace(eng, sk_d, ct_d):
    """(ss, mu') of qrk_dbg_frodo_decaps_trace, outputs pre-filled so a missing store shows."""
    from qrkem._debug import bind
    from qrkem._native import last_error
    n = sk_d.shape[0]
    ss = torch.full((n, eng.ss_len), 0xA5, dtype=torch.uint8, device="cuda")
    mu = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    rc = bind().qrk_dbg_frodo_decaps_trace(eng._ctx, eng.alg.encode(), n, ss.data_ptr(), ct_d.data_ptr(),
                                           sk_d.data_ptr(), mu.data_ptr(), eng._stream())
    assert rc == 0, last_error()
    return _host(ss), _host(mu)


def _first(names, wrong):
    w = np.nonzero(wrong)[0]
    return f"{len(w)} of {len(wrong)} rows, first: {[names[i] for i in w[:4]]}"


@pytest.mark.parametrize("alg,family", CASES)
def test_one_bit_flips_are_rejected_by_the_compare(engines, alg, family):
    import oracle as orc
    eng, h = engines[alg], K.honest(alg)
    frodo = alg.startswith("Frodo")
    names, bad = K.rows(alg, family)
    want = _closed_form(alg, bad)
    honest_ss = np.frombuffer(h["ss"], np.uint8)
    msg = np.frombuffer(h["msg"], np.uint8)
    assert not (want == honest_ss).all(axis=1).any()
    calls = _calls(len(bad))
    assert calls[0][1] + 3 <= COOP
    if family in ("silent", "cycle", "word"):  # one call per set on the lane kernels as well
        assert any(hi - lo + 3 > COOP for lo, hi in calls)
    for lo, hi in calls:
        ct, idx = _with_honest(alg, bad[lo:hi])
        nm = names[lo:hi]
        n = len(ct)
        assert n <= CALL
        hon = np.setdiff1d(np.arange(n), idx)
        assert list(hon) == [0, 1 + (hi - lo) // 2, n - 1]
        sk_d, ct_d = _sk_dev(alg, n), _dev(ct)
        ss, st = eng.decaps(sk_d, ct_d, return_status=True)
        ss, st = _host(ss), _host(st)
        where = f"{alg} {family} rows {lo}..{hi}"
        # rejection, with the closed-form secret, on every tampered row
        assert not (ss[idx] == honest_ss).all(axis=1).any(), \
            f"{where}: ACCEPTED with the honest ss: {_first(nm, (ss[idx] == honest_ss).all(axis=1))}"
        if not frodo:
            assert (st[idx] == -1).all(), f"{where}: status 0 on {_first(nm, st[idx] != -1)}"
        assert np.array_equal(ss[idx], want[lo:hi]), f"{where}: ss differs on {_first(nm, (ss[idx] != want[lo:hi]).any(axis=1))}"
        # the honest rows between them are accepted
        assert (ss[hon] == honest_ss).all(), f"{where}: honest rows {hon[(ss[hon] != honest_ss).any(axis=1)]} rejected"
        assert (st[hon] == 0).all() and (not frodo or (st == 0).all())
        # the decryption absorbed the flip: the compare is what rejected
        if frodo and family == "silent":
            ss2, mu = _frodo_trace(eng, sk_d, ct_d)
            assert np.array_equal(ss2, ss), f"{where}: the traced Decaps differs from the public one"
            assert not mu[:, len(msg):].any()
            wrong = (mu[:, :len(msg)] != msg).any(axis=1)
            assert not wrong[idx].any(), f"{where}: mu' != mu on {_first(nm, wrong[idx])}"
            assert not wrong[hon].any()
        if not frodo:
            _, mp = eng.hqc_code_decode(sk_d, ct_d)
            wrong = (_host(mp) != msg).any(axis=1)
            assert not wrong[idx].any(), f"{where}: m' != m on {_first(nm, wrong[idx])}"
            assert not wrong[hon].any()
    # the closed form is the reference's: every 16th row, and every row of the small families
    pick = np.arange(len(bad)) if family in ("ends", "edge", "salt") else np.arange(0, len(bad), ORACLE_STRIDE)
    sk = np.tile(np.frombuffer(h["sk"], np.uint8), (len(pick), 1))
    o_ss, o_st = orc.batch_decaps(alg, sk, bad[pick], with_status=True)
    assert np.array_equal(o_ss, want[pick]), f"{alg} {family}: oracle differs on {_first([names[i] for i in pick], (o_ss != want[pick]).any(axis=1))}"
    assert (o_st == (0 if frodo else -1)).all()
