"""CPU: qrk_mldsa_keypair_batch and qrk_mldsa_sign_batch are exported, declared and bound, check their arguments
in the documented order before any device work, refuse hash-based names by name; MLDSASigner has the reference's
surface and needs a device for every signing call, while MLDSASignature stays verification-only."""
import ctypes as ct

import pytest

from test_abi import declared_functions, exported_symbols

NAMES = ("ML-DSA-44", "ML-DSA-65", "ML-DSA-87")
SIZES = {2: (1312, 2560, 2420), 3: (1952, 4032, 3309), 5: (2592, 4896, 4627)}
CTX = ct.c_void_p(1)  # never dereferenced: every check below comes before the context is used
BUF = ct.c_void_p(8)  # a non-null buffer, never dereferenced either


def keypair(ctx, alg, n, bufs=None):
    from qrkem._native import LIB
    return LIB.qrk_mldsa_keypair_batch(ctx, alg, n, bufs, bufs, bufs, None)


def sign(ctx, alg, n, ctx_len=0, bufs=None, ctx_str=None):
    from qrkem._native import LIB
    return LIB.qrk_mldsa_sign_batch(ctx, alg, n, bufs, bufs, bufs, None, ctx_str, ctx_len, bufs, bufs, None)


def test_symbols_are_exported_declared_and_bound():
    from qrkem._native import LIB
    exported = exported_symbols()
    declared = declared_functions()
    for name, nargs in (("qrk_mldsa_keypair_batch", 7), ("qrk_mldsa_sign_batch", 12)):
        assert name in exported and name in declared and len(getattr(LIB, name).argtypes) == nargs
    assert "qrk_dbg_mldsa_sign_trace" in exported and "qrk_dbg_mldsa_sign_trace" not in declared


def test_check_order_and_messages():
    import qrkem
    for alg in NAMES:
        a = alg.encode()
        # 1. null context, even with everything else wrong too
        assert keypair(None, a, 1) == -1 and "null context" in qrkem.last_error()
        assert sign(None, a, 1, 256) == -1 and "null context" in qrkem.last_error()
        assert sign(None, b"nonsense", 0, 256) == -1 and "null context" in qrkem.last_error()
        # 3. ctx_len > 255, before n == 0 and before the buffers
        assert sign(CTX, a, 0, 256) == -1 and "255" in qrkem.last_error()
        assert sign(CTX, a, 1, 256) == -1 and "255" in qrkem.last_error()
        # 4. n == 0 is a success once the arguments are accepted, whatever the buffers
        assert sign(CTX, a, 0) == 0 and sign(CTX, a, 0, 255) == 0 and keypair(CTX, a, 0) == 0
        # 5. null buffers, last
        assert keypair(CTX, a, 1) == -1 and "null buffer" in qrkem.last_error()
        assert sign(CTX, a, 1) == -1 and "null buffer" in qrkem.last_error()
        assert sign(CTX, a, 1, 1, bufs=BUF) == -1 and "null buffer" in qrkem.last_error()  # ctx_len without ctx_str
    # 2. the name, before ctx_len: a hash-based name is refused by name and pointed at its own calls
    for a in (b"SPHINCS+-SHA2-128f-simple", b"SLH-DSA-SHA2-256f"):
        for rc in (keypair(CTX, a, 0), sign(CTX, a, 0), sign(CTX, a, 1, 256)):
            assert rc == -1
            assert a.decode() in qrkem.last_error() and "qrk_sig_sign_batch" in qrkem.last_error()
    for a in (b"ML-DSA-45", b"SLH-DSA-SHAKE-128f", b"ML-KEM-768", b""):
        for rc in (keypair(CTX, a, 0), sign(CTX, a, 0), sign(CTX, a, 1, 256)):
            assert rc == -1 and "unsupported signature algorithm" in qrkem.last_error()


def test_trace_hook_checks_like_the_call():
    import qrkem
    from qrkem._debug import bind
    LIB = bind()
    none = [None] * 5
    assert LIB.qrk_dbg_mldsa_sign_trace(None, b"ML-DSA-65", 0, *none, 0, None, None, 814, None, None, None) == -1
    assert "null context" in qrkem.last_error()
    assert LIB.qrk_dbg_mldsa_sign_trace(CTX, b"SLH-DSA-SHA2-128f", 0, *none, 0, None, None, 814, None, None, None) == -1
    assert LIB.qrk_dbg_mldsa_sign_trace(CTX, b"ML-DSA-65", 0, *none, 256, None, None, 814, None, None, None) == -1
    assert LIB.qrk_dbg_mldsa_sign_trace(CTX, b"ML-DSA-65", 0, *none, 0, None, None, 814, None, None, None) == 0
    # the trace buffers are required buffers
    assert LIB.qrk_dbg_mldsa_sign_trace(CTX, b"ML-DSA-65", 1, BUF, BUF, BUF, None, None, 0, BUF, BUF, 814, None, None,
                                        None) == -1
    assert "null buffer" in qrkem.last_error()


def test_generic_pair_still_refuses_and_points_here():
    import qrkem
    from qrkem._native import LIB
    for a in (n.encode() for n in NAMES):
        assert LIB.qrk_sig_sign_batch(CTX, a, 0, None, None, None, None, None, 0, None, None, None) == -1
        err = qrkem.last_error()
        assert a.decode() in err and "no ML-DSA KeyGen or Sign" in err and "qrk_mldsa_sign_batch" in err
    assert LIB.OQS_SIG_alg_count() == 0


def test_signer_surface():
    import qrkem
    with pytest.raises(ValueError, match="Invalid security level"):
        qrkem.MLDSASigner(1)
    for level, (pk, sk, sig) in SIZES.items():
        s = qrkem.MLDSASigner(level)
        assert isinstance(s, qrkem.MLDSASignature) and isinstance(s, qrkem.SignatureAlgorithm)
        assert s.variant == qrkem.MLDSASignature.VARIANTS[level] and s.deterministic is False
        assert (s.public_key_size, s.secret_key_size, s.signature_size) == (pk, sk, sig)
        assert s.name == s.display_name == f"ML-DSA (Level {level})" and "lattice-based" in s.description
        assert s._ctx is None  # no device work at construction
    s = qrkem.MLDSASigner()
    assert s.security_level == 3 and s.device == 0
    assert qrkem.MLDSASigner(5, 0, True).deterministic is True
    for method in ("generate_keypair", "sign", "verify", "generate_keypair_batch", "sign_batch", "verify_batch"):
        assert callable(getattr(s, method))
    # the verify-only class is untouched
    m = qrkem.MLDSASignature()
    assert not hasattr(m, "sign_batch") and not hasattr(m, "generate_keypair_batch")
    with pytest.raises(NotImplementedError, match="verifies ML-DSA signatures only"):
        m.sign(b"", b"m")


def test_signing_needs_a_device():
    import qrkem
    if qrkem.device_count() > 0:
        pytest.skip("GPU present")
    for det in (False, True):
        s = qrkem.MLDSASigner(2, deterministic=det)
        for call in (s.generate_keypair, lambda: s.sign(bytes(2560), b"m"), lambda: s.sign(b"short", b"m"),
                     lambda: s.generate_keypair_batch(2), lambda: s.sign_batch([bytes(2560)], [b"m"]),
                     lambda: s.sign_batch([bytes(2560)], [b"m"], return_status=True)):
            with pytest.raises(RuntimeError, match="cannot create a context"):
                call()
