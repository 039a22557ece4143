"""GPU: a rejected kernel launch fails the ABI call that made it, whichever entry point that is.

The launchers record a failed launch in one thread-local channel (csrc/qrkem_internal.h: launch_begin,
launch_status) and return it; every ABI call opens with launch_begin().  The test hook
qrk_dbg_fail_launch makes launch_begin() record hipErrorLaunchFailure, as if the call's first launch
had been rejected.  No kernel misbehaves while it is on: each is launched as usual on valid buffers
or, on ML-KEM's stop-at-first-failure paths, not at all.

Every case: the call with the hook off returns 0; with the hook on it returns -1 and qrk_last_error()
carries HIP's text for hipErrorLaunchFailure; with the hook off again it returns 0 and writes the same
bytes as the first time (ML-KEM Encaps / Decaps: the fix-up counters' re-zero after a failed chunk;
host-pointer KeyGen: the flag words' re-zero).

Before the launch-error channel had a single owner, the middle call returned 0 for
qrk_hkdf_sha256_batch, qrk_digest_rows, qrk_base64_encode_batch, qrk_base64_decode_batch,
qrk_hqc_supports, qrk_bench_coins, qrk_tamper, qrk_dbg_poly1305_batch and qrk_dbg_ghash_batch (and
for a handshake whose HKDF or key comparison was rejected): the launchers' own return value could not
see the failure, and those entry points never looked at the channel.  That is the defect pinned here.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LAUNCH_FAILURE = "unspecified launch failure"  # hipGetErrorString(hipErrorLaunchFailure)
P, SZ = ct.c_void_p, ct.c_size_t
FILL = 0xA5


@pytest.fixture(scope="module")
def lib():
    from qrkem._debug import bind
    return bind()


@pytest.fixture
def ctx(lib):
    h = ct.c_void_p()
    assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
    yield h
    lib.qrk_ctx_destroy(h)


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: np.frombuffer views are read-only


def _out(*shape, dtype=torch.uint8):
    return torch.full(shape, FILL, dtype=dtype, device="cuda")


def _offsets(n, row):
    return _dev((np.arange(n + 1, dtype=np.uint64) * row).view(np.int64))


def _sizes(lib, alg):
    out = (SZ * 6)()
    assert lib.qrk_kem_sizes(alg.encode(), out) == 0
    return dict(zip(("pk", "sk", "ct", "ss", "kp", "enc"), out))


def _kem_chain(lib, ctx, alg, n):
    """Inputs of the three operations, made with the hook off: (sizes, kp coins, enc coins, pk, sk, ct)."""
    s, a = _sizes(lib, alg), alg.encode()
    kc, ec = _dev(_rand(11, n, s["kp"])), _dev(_rand(12, n, s["enc"]))
    pk, sk, c, ss = _out(n, s["pk"]), _out(n, s["sk"]), _out(n, s["ct"]), _out(n, s["ss"])
    assert lib.qrk_kem_keypair_batch(ctx, a, n, pk.data_ptr(), sk.data_ptr(), kc.data_ptr(), _stream()) == 0
    assert lib.qrk_kem_encaps_batch(ctx, a, n, c.data_ptr(), ss.data_ptr(), pk.data_ptr(), ec.data_ptr(), None,
                                    _stream()) == 0
    torch.cuda.synchronize()
    return s, kc, ec, pk, sk, c


# Each case builds its inputs with the hook off and returns (call, outputs): `call()` makes the ABI call
# and returns its status, `outputs` are the buffers it writes (device tensors or host arrays).  Inputs
# are kept alive by the closure.
def kem_device(alg, n, op):
    def build(lib, ctx):
        s, kc, ec, pk, sk, c = _kem_chain(lib, ctx, alg, n)
        a = alg.encode()
        if op == "keypair":
            o1, o2 = _out(n, s["pk"]), _out(n, s["sk"])
            return lambda: lib.qrk_kem_keypair_batch(ctx, a, n, o1.data_ptr(), o2.data_ptr(), kc.data_ptr(),
                                                     _stream()), [o1, o2]
        if op == "encaps":
            o1, o2, st = _out(n, s["ct"]), _out(n, s["ss"]), _out(n, dtype=torch.int32)
            return lambda: lib.qrk_kem_encaps_batch(ctx, a, n, o1.data_ptr(), o2.data_ptr(), pk.data_ptr(),
                                                    ec.data_ptr(), st.data_ptr(), _stream()), [o1, o2, st]
        o1 = _out(n, s["ss"])
        return lambda: lib.qrk_kem_decaps_batch(ctx, a, n, o1.data_ptr(), c.data_ptr(), sk.data_ptr(),
                                                _stream()), [o1]
    return build


def kem_host(alg, op):
    """n = 1 through the host-pointer entry points: the single-shot ticket path, and for KeyGen the
    pipelined kernel with its error word."""
    def build(lib, ctx):
        s, kc, ec, pk, sk, c = (x if isinstance(x, dict) else x.cpu().numpy() for x in _kem_chain(lib, ctx, alg, 1))
        a = alg.encode()

        def ptr(x):
            return x.ctypes.data

        def host(k):
            return np.full((1, s[k]), FILL, np.uint8)

        if op == "keypair":
            o1, o2 = host("pk"), host("sk")
            return lambda: lib.qrk_kem_keypair_batch_host(ctx, a, 1, ptr(o1), ptr(o2), ptr(kc)), [o1, o2]
        if op == "encaps":
            o1, o2, st = host("ct"), host("ss"), np.full(1, FILL, np.int32)
            return lambda: lib.qrk_kem_encaps_batch_host(ctx, a, 1, ptr(o1), ptr(o2), ptr(pk), ptr(ec),
                                                         ptr(st)), [o1, o2, st]
        o1 = host("ss")
        return lambda: lib.qrk_kem_decaps_batch_host(ctx, a, 1, ptr(o1), ptr(c), ptr(sk)), [o1]
    return build


def handshake(lib, ctx):
    alg, n, key_len = "ML-KEM-512", 64, 32
    s = _sizes(lib, alg)
    ci, cr, ce = _dev(_rand(21, n, s["kp"])), _dev(_rand(22, n, s["kp"])), _dev(_rand(23, n, s["enc"]))
    outs = [_out(n, s["pk"]), _out(n, s["pk"]), _out(n, s["ct"]), _out(n, key_len), _out(n, key_len),
            _out(n, dtype=torch.int32)]
    return lambda: lib.qrk_handshake_batch(ctx, alg.encode(), n, ci.data_ptr(), cr.data_ptr(), ce.data_ptr(), None,
                                           None, 0, key_len, *[o.data_ptr() for o in outs], _stream()), outs


def hkdf(lib, ctx):
    n, ikm, okm = 64, _dev(_rand(31, 64, 32)), _out(64, 32)
    return lambda: lib.qrk_hkdf_sha256_batch(ctx, n, ikm.data_ptr(), 32, None, 0, None, None, 0, okm.data_ptr(), 32,
                                             _stream()), [okm]


def digest_rows(lib, ctx):
    n, a, out = 64, _dev(_rand(32, 64, 32)), _out(64, 32)
    return lambda: lib.qrk_digest_rows(ctx, n, a.data_ptr(), 32, None, 0, out.data_ptr(), _stream()), [out]


def base64_encode(lib, ctx):
    n, raw, txt = 64, _dev(_rand(33, 64, 3)), _out(64, 4)
    return lambda: lib.qrk_base64_encode_batch(ctx, n, raw.data_ptr(), 3, txt.data_ptr(), _stream()), [txt]


def base64_decode(lib, ctx):
    import base64
    n, raw = 64, _rand(33, 64, 3)
    txt = _dev(np.frombuffer(b"".join(base64.b64encode(r.tobytes()) for r in raw), np.uint8).reshape(n, 4))
    back, st = _out(n, 3), _out(n, dtype=torch.int32)
    return lambda: lib.qrk_base64_decode_batch(ctx, n, txt.data_ptr(), 3, back.data_ptr(), st.data_ptr(),
                                               _stream()), [back, st]


def hqc_supports(lib, ctx):
    import hqc_spec as H
    n, w = 64, H.params("HQC-128")["w"]
    r = _dev(np.random.default_rng(41).integers(0, 1 << 32, (n, w), dtype=np.uint64).astype(np.uint32).view(np.int32))
    sup = _out(n, w, dtype=torch.int32)
    return lambda: lib.qrk_hqc_supports(ctx, b"HQC-128", 0, n, r.data_ptr(), sup.data_ptr(), _stream()), [sup]


def hqc_code_decode(lib, ctx):
    import hqc_spec as H
    n, p = 64, H.params("HQC-128")
    _, _, _, _, sk, c = _kem_chain(lib, ctx, "HQC-128", n)
    syms, mp = _out(n, p["n1"]), _out(n, p["k"])
    return lambda: lib.qrk_hqc_code_decode(ctx, b"HQC-128", n, sk.data_ptr(), c.data_ptr(), syms.data_ptr(),
                                           mp.data_ptr(), _stream()), [syms, mp]


def hqc_decaps_trace(lib, ctx):
    import hqc_spec as H
    n, p = 64, H.params("HQC-128")
    _, _, _, _, sk, c = _kem_chain(lib, ctx, "HQC-128", n)
    t, syms, mp = _out(n, p["vb"]), _out(n, p["n1"]), _out(n, p["k"])
    return lambda: lib.qrk_dbg_hqc_decaps_trace(ctx, b"HQC-128", n, sk.data_ptr(), c.data_ptr(), t.data_ptr(),
                                                syms.data_ptr(), mp.data_ptr(), _stream()), [t, syms, mp]


def bench_coins(lib, ctx):
    n, out = 64, _out(64, 96)
    return lambda: lib.qrk_bench_coins(ctx, n, 96, 0x5EED, 7, out.data_ptr(), _stream()), [out]


def tamper(lib, ctx):
    n, c = 64, _dev(_rand(51, 64, 768))  # flipped in place: the test restores it before every call
    return lambda: lib.qrk_tamper(ctx, n, 768, 0x5EED, 2, c.data_ptr(), _stream()), [c]


def aead_seal(alg):
    def build(lib, ctx):
        n = 64
        keys, nonces, pt, off = _dev(_rand(61, n, 32)), _dev(_rand(62, n, 12)), _dev(_rand(63, n, 16)), _offsets(n, 16)
        sealed = _out(n, 44)
        return lambda: lib.qrk_aead_seal_batch(ctx, alg.encode(), n, keys.data_ptr(), nonces.data_ptr(), pt.data_ptr(),
                                               off.data_ptr(), None, None, 0, sealed.data_ptr(), _stream()), [sealed]
    return build


def aead_open(alg):
    def build(lib, ctx):
        n = 64
        keys = _dev(_rand(61, n, 32))
        seal, (sealed,) = aead_seal(alg)(lib, ctx)
        assert seal() == 0
        off, pt, st = _offsets(n, 44), _out(n, 16), _out(n, dtype=torch.int32)
        return lambda: lib.qrk_aead_open_batch(ctx, alg.encode(), n, keys.data_ptr(), sealed.data_ptr(), off.data_ptr(),
                                               None, None, 0, pt.data_ptr(), st.data_ptr(), _stream()), [pt, st]
    return build


def sig_verify(lib, ctx):
    import make_golden_mldsa as gold
    f = gold.load()["ML-DSA-44"]
    n = len(f["sigs"])
    pk = _dev(np.frombuffer(f["pk"] * n, np.uint8))
    sig = _dev(np.frombuffer(b"".join(f["sigs"]), np.uint8))
    msg = _dev(np.frombuffer(b"".join(f["msgs"]), np.uint8))
    off = _dev(np.cumsum([0] + [len(m) for m in f["msgs"]]).astype(np.uint64).view(np.int64))
    st = _out(n, dtype=torch.int32)
    return lambda: lib.qrk_sig_verify_batch(ctx, b"ML-DSA-44", n, pk.data_ptr(), msg.data_ptr(), off.data_ptr(),
                                            sig.data_ptr(), None, 0, st.data_ptr(), _stream()), [st]


SLH, SLH_ROWS = "SLH-DSA-SHA2-128f", 2  # the cheapest set; one partly filled front workgroup, one core workgroup


@functools.lru_cache(maxsize=None)
def _slh_gold():
    """tests/golden/slhdsa.json, loaded once for the three cases (the load rebuilds every key with the spec)."""
    import make_golden_slhdsa as gold
    return gold, gold.load()[SLH]


def _slh_fixture():
    """The key of tests/golden/slhdsa.json and its first SLH_ROWS messages (0 and 8 bytes), ragged."""
    gold, f = _slh_gold()
    msgs = f["msgs"][:SLH_ROWS]
    msg = _dev(np.frombuffer(b"".join(msgs), np.uint8))
    off = _dev(np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64).view(np.int64))
    return gold, f, msg, off


def slh_verify(lib, ctx):
    gold, f, msg, off = _slh_fixture()
    n = SLH_ROWS
    sigs = gold.signatures(SLH, {**f, "msgs": f["msgs"][:n], "records": f["records"][:n]})
    pk = _dev(np.frombuffer(f["pk"] * n, np.uint8))
    sig = _dev(np.frombuffer(b"".join(sigs), np.uint8))
    st = _out(n, dtype=torch.int32)
    return lambda: lib.qrk_sig_verify_batch(ctx, SLH.encode(), n, pk.data_ptr(), msg.data_ptr(), off.data_ptr(),
                                            sig.data_ptr(), None, 0, st.data_ptr(), _stream()), [st]


def slh_keypair(lib, ctx):
    gold, f, _, _ = _slh_fixture()
    n = SLH_ROWS
    seeds = np.frombuffer(b"".join(f["seeds"]), np.uint8)  # row 0: the fixture key; the rest: fixed random seeds
    seeds = _dev(np.stack([seeds] + [_rand(81 + i, seeds.size) for i in range(1, n)]))
    pk, sk = _out(n, len(f["pk"])), _out(n, len(f["sk"]))
    return lambda: lib.qrk_sig_keypair_batch(ctx, SLH.encode(), n, seeds.data_ptr(), pk.data_ptr(), sk.data_ptr(),
                                             _stream()), [pk, sk]


def slh_sign(lib, ctx):
    gold, f, msg, off = _slh_fixture()
    n = SLH_ROWS
    sk = _dev(np.frombuffer(f["sk"] * n, np.uint8))
    size = (SZ * 3)()
    assert lib.qrk_sig_sizes(SLH.encode(), size) == 0
    sig, st = _out(n, size[2]), _out(n, dtype=torch.int32)
    return lambda: lib.qrk_sig_sign_batch(ctx, SLH.encode(), n, sk.data_ptr(), msg.data_ptr(), off.data_ptr(), None,
                                          None, 0, sig.data_ptr(), st.data_ptr(), _stream()), [sig, st]


def frodo_decaps_trace(lib, ctx):
    alg, n = "FrodoKEM-640-SHAKE", 64
    s, _, _, _, sk, c = _kem_chain(lib, ctx, alg, n)
    ss, mu = _out(n, s["ss"]), _out(n, 32)
    return lambda: lib.qrk_dbg_frodo_decaps_trace(ctx, alg.encode(), n, ss.data_ptr(), c.data_ptr(), sk.data_ptr(),
                                                  mu.data_ptr(), _stream()), [ss, mu]


def frodo_sample(kg):
    def build(lib, ctx):
        import frodo_forward_cases as W
        import frodo_spec as F
        alg, n = "FrodoKEM-640-SHAKE", 64
        p = F.params(alg)
        words = _dev(np.resize(W.every_word_rows(p, kg, True), (n, W.words_per_row(p, kg))).view(np.int16))
        outs = [_out(n, 8, W.pitch(p["n"])), _out(n, 8 * p["n"], dtype=torch.int16)]  # int8 samples as bytes
        outs += [] if kg else [_out(n, 64, dtype=torch.int16)]
        epp = None if kg else outs[2].data_ptr()
        return lambda: lib.qrk_dbg_frodo_sample(ctx, alg.encode(), int(kg), n, words.data_ptr(), outs[0].data_ptr(),
                                                outs[1].data_ptr(), epp, _stream()), outs
    return build


def frodo_from_samples(alg, kg):
    def build(lib, ctx):
        import frodo_forward_cases as W
        import frodo_spec as F
        n, p, inp = 64, F.params(alg), W.from_samples_inputs(alg, kg)
        idx = W.tiled(len(inp["names"]), n)
        s8, e16 = _dev(inp["s8"][idx]), _dev(inp["e16"][idx])
        if kg:
            src, outs = _dev(inp["seedA"][idx]), [_out(n, p["pk"]), _out(n, p["sk"])]
            return lambda: lib.qrk_dbg_frodo_from_samples(ctx, alg.encode(), 1, n, s8.data_ptr(), e16.data_ptr(), None,
                                                          src.data_ptr(), None, outs[0].data_ptr(), outs[1].data_ptr(),
                                                          _stream()), outs
        epp, pk, mu, outs = _dev(inp["epp16"][idx]), _dev(inp["pk"][idx]), _dev(inp["mu"][idx]), [_out(n, p["ct"])]
        return lambda: lib.qrk_dbg_frodo_from_samples(ctx, alg.encode(), 0, n, s8.data_ptr(), e16.data_ptr(),
                                                      epp.data_ptr(), pk.data_ptr(), mu.data_ptr(), outs[0].data_ptr(),
                                                      None, _stream()), outs
    return build


def dbg_hook(name, fixed_len):
    def build(lib, ctx):
        n = 64
        fixed, data, off, out = _dev(_rand(71, n, fixed_len)), _dev(_rand(72, n, 16)), _offsets(n, 16), _out(n, 16)
        fn = getattr(lib, name)
        return lambda: fn(n, fixed.data_ptr(), data.data_ptr(), off.data_ptr(), out.data_ptr(), _stream()), [out]
    return build


CASES = {f"{op}-{alg}-{n}": kem_device(alg, n, op)
         for alg, n in (("ML-KEM-512", 64), ("ML-KEM-512", 1088), ("FrodoKEM-640-SHAKE", 64), ("HQC-128", 64))
         for op in ("keypair", "encaps", "decaps")}
CASES.update({f"{op}-host-ML-KEM-512-1": kem_host("ML-KEM-512", op) for op in ("keypair", "encaps", "decaps")})
CASES.update({
    "handshake-ML-KEM-512-64": handshake, "hkdf": hkdf, "digest_rows": digest_rows, "base64_encode": base64_encode,
    "base64_decode": base64_decode, "hqc_supports": hqc_supports, "hqc_code_decode": hqc_code_decode,
    "dbg_hqc_decaps_trace": hqc_decaps_trace,
    "bench_coins": bench_coins, "tamper": tamper, "sig_verify-ML-DSA-44": sig_verify,
    f"sig_verify-{SLH}-{SLH_ROWS}": slh_verify, f"sig_keypair-{SLH}-{SLH_ROWS}": slh_keypair,
    f"sig_sign-{SLH}-{SLH_ROWS}": slh_sign,
    "dbg_poly1305": dbg_hook("qrk_dbg_poly1305_batch", 32), "dbg_ghash": dbg_hook("qrk_dbg_ghash_batch", 16),
    "dbg_frodo_decaps_trace-FrodoKEM-640-SHAKE-64": frodo_decaps_trace,
    "dbg_frodo_sample-encaps-FrodoKEM-640-SHAKE-64": frodo_sample(False),
    "dbg_frodo_sample-keygen-FrodoKEM-640-SHAKE-64": frodo_sample(True),
    "dbg_frodo_from_samples-encaps-FrodoKEM-640-SHAKE-64": frodo_from_samples("FrodoKEM-640-SHAKE", False),
    "dbg_frodo_from_samples-keygen-FrodoKEM-640-SHAKE-64": frodo_from_samples("FrodoKEM-640-SHAKE", True),
    "dbg_frodo_from_samples-encaps-FrodoKEM-640-AES-64": frodo_from_samples("FrodoKEM-640-AES", False),
    "dbg_frodo_from_samples-keygen-FrodoKEM-640-AES-64": frodo_from_samples("FrodoKEM-640-AES", True),
})
for _alg in ("AES-256-GCM", "ChaCha20-Poly1305"):
    CASES[f"aead_seal-{_alg}"] = aead_seal(_alg)
    CASES[f"aead_open-{_alg}"] = aead_open(_alg)


def _copy(b):
    return b.clone() if torch.is_tensor(b) else b.copy()


def _restore(bufs, init):
    for b, i in zip(bufs, init):
        if torch.is_tensor(b):
            b.copy_(i)
        else:
            b[...] = i


def _bytes(bufs):
    torch.cuda.synchronize()
    return [(b.cpu().numpy() if torch.is_tensor(b) else b).tobytes() for b in bufs]


@pytest.mark.parametrize("case", sorted(CASES))
def test_rejected_launch_fails_the_call_and_the_next_call_is_exact(lib, ctx, case):
    from qrkem._native import last_error
    call, outs = CASES[case](lib, ctx)
    init = [_copy(b) for b in outs]
    assert call() == 0, last_error()
    first = _bytes(outs)
    assert first != _bytes(init), "the call wrote nothing"
    _restore(outs, init)
    try:
        assert lib.qrk_dbg_fail_launch(1) == 0
        rc, err = call(), last_error()
        torch.cuda.synchronize()
    finally:
        lib.qrk_dbg_fail_launch(0)
    assert rc == -1, "a rejected launch was reported as success"
    assert LAUNCH_FAILURE in err, err
    _restore(outs, init)
    assert call() == 0, last_error()
    assert _bytes(outs) == first
