"""CPU: qrk_sig_keypair_batch and qrk_sig_sign_batch are exported and declared, check their arguments in the
documented order before any device work, refuse ML-DSA names by name; SPHINCSSignature keeps raising
NotImplementedError by default and, with signing=True, needs a device for every signing call."""
import ctypes as ct

import pytest

from test_abi import declared_functions, exported_symbols

SETS = ("128f", "192f", "256f")
NAMES = [f"SPHINCS+-SHA2-{s}-simple" for s in SETS] + [f"SLH-DSA-SHA2-{s}" for s in SETS]
CTX = ct.c_void_p(1)  # never dereferenced: every check below comes before the context is used


def keypair(ctx, alg, n):
    from qrkem._native import LIB
    return LIB.qrk_sig_keypair_batch(ctx, alg, n, None, None, None, None)


def sign(ctx, alg, n, ctx_len=0):
    from qrkem._native import LIB
    return LIB.qrk_sig_sign_batch(ctx, alg, n, None, None, None, None, None, ctx_len, None, None, None)


def test_symbols_are_exported_and_declared():
    from qrkem._native import LIB
    exported = exported_symbols()
    declared = declared_functions()
    for name, nargs in (("qrk_sig_keypair_batch", 7), ("qrk_sig_sign_batch", 12)):
        assert name in exported and name in declared and len(getattr(LIB, name).argtypes) == nargs


def test_check_order_and_messages():
    import qrkem
    for alg in NAMES:
        a = alg.encode()
        # 1. null context, even with everything else wrong too
        assert keypair(None, a, 1) == -1 and "null context" in qrkem.last_error()
        assert sign(None, a, 1, 256) == -1 and "null context" in qrkem.last_error()
        assert sign(None, b"nonsense", 0, 256) == -1 and "null context" in qrkem.last_error()
        # 3. ctx_len > 255, before the flavour rule and before n == 0
        assert sign(CTX, a, 0, 256) == -1 and "255" in qrkem.last_error()
        # 4. a context under a SPHINCS+ name
        if alg.startswith("SPHINCS+"):
            assert sign(CTX, a, 0, 1) == -1
            assert "no context string" in qrkem.last_error() and alg in qrkem.last_error()
        else:
            assert sign(CTX, a, 0, 255) == 0
        # n == 0 is a success once the arguments are accepted
        assert sign(CTX, a, 0) == 0 and keypair(CTX, a, 0) == 0
    # 2. the name, before ctx_len
    for a in (b"ML-DSA-44", b"ML-DSA-65", b"ML-DSA-87"):
        for rc in (keypair(CTX, a, 0), sign(CTX, a, 0), sign(CTX, a, 1, 256)):
            assert rc == -1
            assert a.decode() in qrkem.last_error() and "no ML-DSA KeyGen or Sign" in qrkem.last_error()
    for a in (b"SPHINCS+-SHA2-128s-simple", b"SLH-DSA-SHAKE-128f", b"ML-KEM-768", b""):
        for rc in (keypair(CTX, a, 0), sign(CTX, a, 0), sign(CTX, a, 1, 256)):
            assert rc == -1 and "unsupported signature algorithm" in qrkem.last_error()


def test_registry_stays_empty_and_sizes_unchanged():
    from qrkem._native import LIB
    assert LIB.OQS_SIG_alg_count() == 0
    out = (ct.c_size_t * 3)()
    assert LIB.qrk_sig_sizes(b"SLH-DSA-SHA2-256f", out) == 0 and tuple(out) == (64, 128, 49856)


def test_default_classes_still_raise():
    import qrkem
    s = qrkem.SPHINCSSignature()
    assert s.signing is False and s.deterministic is False
    with pytest.raises(NotImplementedError, match="qrkem verifies SPHINCS\\+ signatures only: key generation stays"):
        s.generate_keypair()
    with pytest.raises(NotImplementedError, match="qrkem verifies SPHINCS\\+ signatures only: signing stays"):
        s.sign(bytes(s.secret_key_size), b"m")
    with pytest.raises(NotImplementedError, match="qrkem verifies SPHINCS\\+ signatures only: "):
        s.generate_keypair_batch(1)
    with pytest.raises(NotImplementedError, match="qrkem verifies SPHINCS\\+ signatures only: "):
        s.sign_batch([bytes(s.secret_key_size)], [b"m"])
    assert s._ctx is None
    m = qrkem.MLDSASignature()
    with pytest.raises(NotImplementedError, match="qrkem verifies ML-DSA signatures only: "):
        m.generate_keypair()
    with pytest.raises(NotImplementedError, match="qrkem verifies ML-DSA signatures only: "):
        m.sign(b"", b"m")
    assert not hasattr(m, "sign_batch")
    with pytest.raises(TypeError):
        qrkem.MLDSASignature(signing=True)


def test_signing_needs_a_device():
    import qrkem
    if qrkem.device_count() > 0:
        pytest.skip("GPU present")
    for fips in (False, True):
        s = qrkem.SPHINCSSignature(1, fips205=fips, signing=True, deterministic=True)
        assert s.signing and s.deterministic and s.n_bytes == 16
        for call in (s.generate_keypair, lambda: s.sign(bytes(64), b"m"), lambda: s.generate_keypair_batch(2),
                     lambda: s.sign_batch([bytes(64)], [b"m"]),
                     lambda: s.sign_batch([bytes(64)], [b"m"], return_status=True)):
            with pytest.raises(RuntimeError, match="cannot create a context"):
                call()
