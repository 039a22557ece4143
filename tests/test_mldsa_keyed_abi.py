"""CPU: the ML-DSA key-set calls (qrk_mldsa_pubkeys_load .. qrk_mldsa_sign_keyed_batch) are exported, declared and
bound, check their arguments in the documented order before any device work and say which argument they refuse;
MLDSAKeySet and the keyed methods have the stated surface, raise ValueError on a mismatched set before any GPU call
and need a device for everything else."""
import ctypes as ct
import inspect

import pytest

from test_abi import HEADER, declared_functions, exported_symbols

NAMES = ("ML-DSA-44", "ML-DSA-65", "ML-DSA-87")
CTX = ct.c_void_p(1)  # never dereferenced: every check below comes before the context is used
BUF = ct.c_void_p(8)  # a non-null buffer, never dereferenced either
PUBLIC = {"qrk_mldsa_pubkeys_load": 6, "qrk_mldsa_seckeys_load": 6, "qrk_mldsa_keyset_info": 2,
          "qrk_mldsa_keyset_free": 1, "qrk_mldsa_verify_keyed_batch": 11, "qrk_mldsa_sign_keyed_batch": 12}
HOOKS = ("qrk_dbg_mldsa_verify_keyed_trace", "qrk_dbg_mldsa_sign_keyed_trace")


def load(which, ctx, alg, g, keys=None, out=True):
    from qrkem._native import LIB
    h = ct.c_void_p()
    rc = getattr(LIB, which)(ctx, alg, g, keys, ct.byref(h) if out else None, None)
    assert not h.value  # no handle comes back from a refused load
    return rc


def verify(ctx, ks, n, ctx_len=0, bufs=None, ctx_str=None, index=None):
    from qrkem._native import LIB
    return LIB.qrk_mldsa_verify_keyed_batch(ctx, ks, n, index, bufs, bufs, bufs, ctx_str, ctx_len, bufs, None)


def sign(ctx, ks, n, ctx_len=0, bufs=None, ctx_str=None, index=None):
    from qrkem._native import LIB
    return LIB.qrk_mldsa_sign_keyed_batch(ctx, ks, n, index, bufs, bufs, None, ctx_str, ctx_len, bufs, bufs, None)


def test_symbols_are_exported_declared_and_bound():
    from qrkem._native import LIB
    exported = exported_symbols()
    declared = declared_functions()
    for name, nargs in PUBLIC.items():
        assert name in exported and name in declared and len(getattr(LIB, name).argtypes) == nargs, name
    for name in HOOKS:
        assert name in exported and name not in declared
    assert "typedef struct qrk_mldsa_keyset qrk_mldsa_keyset;" in HEADER.read_text()


def test_loaders_check_order_and_messages():
    import qrkem
    for which in ("qrk_mldsa_pubkeys_load", "qrk_mldsa_seckeys_load"):
        for alg in NAMES:
            a = alg.encode()
            # 1. null context, even with everything else wrong too
            assert load(which, None, a, 0) == -1 and "null context" in qrkem.last_error()
            assert load(which, None, b"nonsense", 0, out=False) == -1 and "null context" in qrkem.last_error()
            # 3. g == 0, before the pointers
            assert load(which, CTX, a, 0) == -1 and "at least one key" in qrkem.last_error()
            assert load(which, CTX, a, 0, BUF) == -1 and "at least one key" in qrkem.last_error()
            # 4. null pointers
            assert load(which, CTX, a, 1) == -1 and "null buffer" in qrkem.last_error()
            assert load(which, CTX, a, 1, BUF, out=False) == -1 and "null buffer" in qrkem.last_error()
            # 5. more keys than one allocation may hold under the scratch budget rule
            assert load(which, CTX, a, 1 << 40, BUF) == -1
            assert "scratch budget" in qrkem.last_error() and alg in qrkem.last_error()
        # 2. the name, before g: an ML-KEM, SLH-DSA or unknown name gets the signature calls' message
        for a in (b"ML-KEM-768", b"SLH-DSA-SHA2-128f", b"SPHINCS+-SHA2-128f-simple", b"ML-DSA-45", b""):
            assert load(which, CTX, a, 0) == -1
            assert "unsupported signature algorithm" in qrkem.last_error()
        assert load(which, CTX, None, 1, BUF) == -1 and "unsupported signature algorithm" in qrkem.last_error()


def test_keyed_calls_check_order_and_messages():
    import qrkem
    for call in (verify, sign):
        # 1. null context first, whatever else is wrong
        assert call(None, None, 1, 256) == -1 and "null context" in qrkem.last_error()
        assert call(None, BUF, 0) == -1 and "null context" in qrkem.last_error()
        # 2. then the key set: a null one is named, before ctx_len, before n == 0 and before the buffers
        for n, ctx_len in ((0, 0), (0, 256), (1, 256), (1, 0)):
            assert call(CTX, None, n, ctx_len, bufs=BUF) == -1 and "null key set" in qrkem.last_error()


def test_trace_hooks_check_like_the_calls():
    import qrkem
    from qrkem._debug import bind
    LIB = bind()
    v, s = LIB.qrk_dbg_mldsa_verify_keyed_trace, LIB.qrk_dbg_mldsa_sign_keyed_trace
    assert v(None, None, 0, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert "null context" in qrkem.last_error()
    assert v(CTX, None, 0, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert "null key set" in qrkem.last_error()
    assert v(CTX, None, 1, None, BUF, BUF, BUF, None, 0, BUF, None, None, None, None, None) == -1
    assert "null trace buffer" in qrkem.last_error()
    assert s(None, None, 0, None, None, None, None, None, 0, None, None, 814, None, None, None) == -1
    assert "null context" in qrkem.last_error()
    assert s(CTX, None, 1, None, BUF, BUF, None, None, 256, BUF, BUF, 814, BUF, BUF, None) == -1
    assert "null key set" in qrkem.last_error()


def test_info_and_free_take_null():
    import qrkem
    from qrkem._native import LIB
    out = (ct.c_size_t * 4)(7, 7, 7, 7)
    assert LIB.qrk_mldsa_keyset_info(None, out) == -1 and "null key set" in qrkem.last_error()
    assert list(out) == [7, 7, 7, 7]
    assert LIB.qrk_mldsa_keyset_info(None, None) == -1
    LIB.qrk_mldsa_keyset_free(None)  # a no-op
    # the existing calls and the empty registry are as they were
    assert LIB.OQS_SIG_alg_count() == 0
    assert LIB.qrk_sig_sign_batch(CTX, b"ML-DSA-65", 0, None, None, None, None, None, 0, None, None, None) == -1
    assert "qrk_mldsa_sign_batch" in qrkem.last_error()


def test_surface():
    import qrkem
    ks = qrkem.MLDSAKeySet(None, "ML-DSA-65", 3, True)
    assert (ks.g, ks.secret, ks.variant, ks.device, ks.closed, ks.device_bytes) == (3, True, "ML-DSA-65", 0, True, 0)
    for attr in ("close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(ks, attr))
    with ks as inner:
        assert inner is ks
    ks.close()  # closing twice is harmless
    assert qrkem.signatures.MLDSAKeySet is qrkem.MLDSAKeySet

    def params(f):
        return list(inspect.signature(f).parameters)
    v, s = qrkem.MLDSASignature, qrkem.MLDSASigner
    assert params(v.load_public_keys) == ["self", "public_keys"]
    assert params(v.verify_keyed) == params(v.verify_keyed_status) == [
        "self", "keyset", "messages", "signatures", "key_index", "offsets"]
    assert params(s.load_secret_keys) == ["self", "private_keys"]
    assert params(s.sign_keyed) == ["self", "keyset", "messages", "key_index", "offsets", "rnd", "return_status"]
    for f in (v.verify_keyed, v.verify_keyed_status, s.sign_keyed):
        defaults = {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not p.empty}
        assert defaults.pop("return_status", False) is False and set(defaults.values()) == {None}
    # the signer verifies too; the verify-only class still has no signing half
    assert s.verify_keyed is v.verify_keyed and s.load_public_keys is v.load_public_keys
    assert not hasattr(v, "sign_keyed") and not hasattr(v, "load_secret_keys") and not hasattr(v, "sign_batch")


def test_mismatched_sets_are_value_errors_before_any_gpu_call():
    import qrkem
    signer, verifier = qrkem.MLDSASigner(3, deterministic=True), qrkem.MLDSASignature(3)
    pub = qrkem.MLDSAKeySet(None, "ML-DSA-65", 1, False)
    sec = qrkem.MLDSAKeySet(None, "ML-DSA-65", 1, True)
    with pytest.raises(ValueError, match="holds ML-DSA-44 keys, this object is ML-DSA-65"):
        verifier.verify_keyed(qrkem.MLDSAKeySet(None, "ML-DSA-44", 1, False), [b"m"], [bytes(3309)])
    with pytest.raises(ValueError, match="holds ML-DSA-87 keys"):
        signer.sign_keyed(qrkem.MLDSAKeySet(None, "ML-DSA-87", 1, True), [b"m"])
    with pytest.raises(ValueError, match="secret key set cannot verify"):
        verifier.verify_keyed(sec, [b"m"], [bytes(3309)])
    with pytest.raises(ValueError, match="secret key set cannot verify"):
        signer.verify_keyed_status(sec, [b"m"], [bytes(3309)])
    with pytest.raises(ValueError, match="public key set cannot sign"):
        signer.sign_keyed(pub, [b"m"])
    with pytest.raises(ValueError, match="must be an MLDSAKeySet"):
        signer.sign_keyed(object(), [b"m"])
    with pytest.raises(ValueError, match="only for a key set of one key"):
        verifier.verify_keyed(qrkem.MLDSAKeySet(None, "ML-DSA-65", 2, False), [b"m"], [bytes(3309)])
    with pytest.raises(ValueError, match="only for a key set of one key"):
        signer.sign_keyed(qrkem.MLDSAKeySet(None, "ML-DSA-65", 2, True), [b"m"])
    with pytest.raises(ValueError, match="on device 1"):
        verifier.verify_keyed(qrkem.MLDSAKeySet(None, "ML-DSA-65", 1, False, device=1), [b"m"], [bytes(3309)])
    assert signer._ctx is None and verifier._ctx is None  # none of them reached the device


def test_keyed_methods_need_a_device():
    import qrkem
    if qrkem.device_count() > 0:
        pytest.skip("GPU present")
    for det in (False, True):
        s = qrkem.MLDSASigner(2, deterministic=det)
        pub = qrkem.MLDSAKeySet(None, "ML-DSA-44", 1, False)
        sec = qrkem.MLDSAKeySet(None, "ML-DSA-44", 1, True)
        for call in (lambda: s.load_public_keys([bytes(1312)]), lambda: s.load_secret_keys([bytes(2560)]),
                     lambda: s.load_public_keys([]), lambda: s.load_secret_keys([b"short"]),
                     lambda: s.verify_keyed(pub, [b"m"], [bytes(2420)]),
                     lambda: s.verify_keyed_status(pub, [b"m"], [bytes(2420)], key_index=[0]),
                     lambda: s.sign_keyed(sec, [b"m"]), lambda: s.sign_keyed(sec, [b"m"], [0], return_status=True)):
            with pytest.raises(RuntimeError, match="cannot create a context"):
                call()
    v = qrkem.MLDSASignature(5)
    with pytest.raises(RuntimeError, match="cannot create a context"):
        v.load_public_keys([bytes(2592)])
