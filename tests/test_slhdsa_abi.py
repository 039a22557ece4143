"""CPU: the signature entry points answer the SLH-DSA / SPHINCS+ names, refuse every other name and the
context-string misuses before any device work, keep the OQS_SIG registry empty, export the test hook
without declaring it, and SPHINCSSignature checks its arguments without a GPU."""
import ctypes as ct

import pytest

from test_abi import declared_functions, exported_symbols

SIZES = {"128f": (32, 64, 17088), "192f": (48, 96, 35664), "256f": (64, 128, 49856)}
NAMES = {f(s): SIZES[s] for s in SIZES for f in (lambda s: f"SPHINCS+-SHA2-{s}-simple", lambda s: f"SLH-DSA-SHA2-{s}")}
LEVEL = {1: "128f", 3: "192f", 5: "256f"}


def test_sig_sizes():
    import qrkem
    from qrkem._native import LIB
    out = (ct.c_size_t * 3)()
    assert len(NAMES) == 6
    for alg, sizes in NAMES.items():
        assert LIB.qrk_sig_sizes(alg.encode(), out) == 0 and tuple(out) == sizes, alg
    for alg in (b"ML-KEM-768", b"SPHINCS+-SHA2-128s-simple", b"SPHINCS+-SHAKE-128f-simple", b"sphincs+-sha2-128f-simple",
                b""):
        assert LIB.qrk_sig_sizes(alg, out) == -1
        assert "unsupported signature algorithm" in qrkem.last_error()
    assert LIB.qrk_sig_sizes(b"ML-DSA-65", out) == 0 and tuple(out) == (1952, 4032, 3309)


def test_context_rules_are_checked_before_any_device_work():
    import qrkem
    from qrkem._native import LIB
    ctx = ct.c_void_p(1)  # never dereferenced: name and ctx_len are checked first
    for alg in NAMES:
        if alg.startswith("SPHINCS+"):
            assert LIB.qrk_sig_verify_batch(ctx, alg.encode(), 1, None, None, None, None, None, 1, None, None) == -1
            assert "no context string" in qrkem.last_error() and alg in qrkem.last_error()
        else:
            assert LIB.qrk_sig_verify_batch(ctx, alg.encode(), 1, None, None, None, None, None, 256, None, None) == -1
            assert "255" in qrkem.last_error()
            assert LIB.qrk_sig_verify_batch(ctx, alg.encode(), 0, None, None, None, None, None, 255, None, None) == 0
        assert LIB.qrk_sig_verify_batch(ctx, alg.encode(), 0, None, None, None, None, None, 0, None, None) == 0
        assert LIB.qrk_sig_verify_batch(None, alg.encode(), 1, None, None, None, None, None, 0, None, None) == -1
        assert "null context" in qrkem.last_error()
    for alg in (b"SPHINCS+-SHA2-128s-simple", b"SLH-DSA-SHAKE-128f", b"SLH-DSA-SHA2-128f-simple"):
        assert LIB.qrk_sig_verify_batch(ctx, alg, 1, None, None, None, None, None, 0, None, None) == -1
        assert "unsupported signature algorithm" in qrkem.last_error()


def test_trace_hook_is_exported_and_not_declared():
    import qrkem
    from qrkem._debug import bind
    LIB = bind()
    exported = exported_symbols()
    declared = declared_functions()
    assert "qrk_dbg_slhdsa_verify_trace" in exported and "qrk_dbg_slhdsa_verify_trace" not in declared
    for name, nargs in (("qrk_sig_sizes", 2), ("qrk_sig_verify_batch", 11)):
        assert name in exported and name in declared and len(getattr(LIB, name).argtypes) == nargs
    # each family's hook refuses the other family's names
    args = [None, None, None, None, None, 0, None, None, None, None, None, None]
    assert LIB.qrk_dbg_slhdsa_verify_trace(ct.c_void_p(1), b"ML-DSA-65", 0, *args) == -1
    assert "unsupported signature algorithm" in qrkem.last_error()
    assert LIB.qrk_dbg_slhdsa_verify_trace(ct.c_void_p(1), b"SLH-DSA-SHA2-192f", 0, *args) == 0


def test_oqs_sig_registry_stays_empty():
    from qrkem._native import LIB
    assert LIB.OQS_SIG_alg_count() == 0
    assert LIB.OQS_SIG_alg_is_enabled(b"SPHINCS+-SHA2-128f-simple") == 0


def test_class_keeps_the_reference_surface_and_argument_errors():
    import qrkem
    from qrkem.signatures import MLDSASignature, SignatureAlgorithm, SPHINCSSignature
    assert qrkem.SPHINCSSignature is SPHINCSSignature
    assert SPHINCSSignature().variant == "SPHINCS+-SHA2-192f-simple"
    # one shared base, not a copy: both classes run the same batch code
    assert SPHINCSSignature.verify_status is MLDSASignature.verify_status
    assert SPHINCSSignature.verify is MLDSASignature.verify
    for fips in (False, True):
        for level, s_ in LEVEL.items():
            variant = f"SLH-DSA-SHA2-{s_}" if fips else f"SPHINCS+-SHA2-{s_}-simple"
            s = SPHINCSSignature(security_level=level, fips205=fips)
            assert isinstance(s, SignatureAlgorithm) and isinstance(s, qrkem.CryptoAlgorithm)
            assert s.name == s.display_name == f"SPHINCS+ (Level {level})"
            assert s.variant == s.actual_variant == variant
            assert s.description == ("SPHINCS+ is a stateless hash-based digital signature scheme. "
                                     "Its security relies only on the security of the underlying hash functions.")
            assert s.is_using_mock is False and s.get_security_info()["security_level"] == level
            assert (s.public_key_size, s.secret_key_size, s.signature_size) == SIZES[s_]
            with pytest.raises(NotImplementedError, match="qrkem verifies SPHINCS\\+ signatures only: "):
                s.generate_keypair()
            with pytest.raises(NotImplementedError, match="qrkem verifies SPHINCS\\+ signatures only: "):
                s.sign(bytes(s.secret_key_size), b"m")
            # wrong lengths: False with no GPU call (a context is never created)
            assert s.verify(bytes(s.public_key_size - 1), b"m", bytes(s.signature_size)) is False
            assert s.verify(bytes(s.public_key_size), b"m", bytes(s.signature_size + 1)) is False
            assert s.verify(b"", b"", b"") is False
            assert s._ctx is None
    for level in (2, 4, 0, "3"):
        with pytest.raises(ValueError, match=f"Invalid security level: {level}. Must be 1, 3, or 5."):
            SPHINCSSignature(security_level=level)


def test_verify_never_raises_without_a_gpu():
    import qrkem
    if qrkem.device_count() > 0:
        pytest.skip("GPU present")
    s = qrkem.SPHINCSSignature(1)
    assert s.verify(bytes(32), b"m", bytes(17088)) is False  # logged, as the reference's except -> False
    with pytest.raises(RuntimeError, match="cannot create a context"):
        s.verify_batch([bytes(32)], [b"m"], [bytes(17088)])
