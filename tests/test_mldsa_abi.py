"""CPU: the ML-DSA verification entry points are exported, declared and bound, answer the size query,
refuse bad names and over-long context strings before any device work, leave the OQS_SIG registry
empty, and the reference-shaped class checks its arguments without a GPU."""
import ctypes as ct

import pytest

from test_abi import declared_functions, exported_symbols

SIZES = {"ML-DSA-44": (1312, 2560, 2420), "ML-DSA-65": (1952, 4032, 3309), "ML-DSA-87": (2592, 4896, 4627)}


def test_sig_symbols_exported_declared_and_bound():
    from qrkem._native import LIB
    exported = exported_symbols()
    declared = declared_functions()
    for name, nargs in (("qrk_sig_sizes", 2), ("qrk_sig_verify_batch", 11)):
        assert name in exported and name in declared
        assert len(getattr(LIB, name).argtypes) == nargs
    assert "qrk_dbg_mldsa_verify_trace" in exported and "qrk_dbg_mldsa_verify_trace" not in declared


def test_sig_sizes():
    import qrkem
    from qrkem._native import LIB
    out = (ct.c_size_t * 3)()
    for alg, sizes in SIZES.items():
        assert LIB.qrk_sig_sizes(alg.encode(), out) == 0 and tuple(out) == sizes
    for alg in (b"ML-DSA-45", b"ML-KEM-768", b"Dilithium3", b"ml-dsa-65", b""):
        assert LIB.qrk_sig_sizes(alg, out) == -1
        assert "unsupported signature algorithm" in qrkem.last_error()
    assert LIB.qrk_sig_sizes(None, out) == -1


def test_bad_name_and_long_context_are_refused_before_any_device_work():
    import qrkem
    from qrkem._native import LIB
    ctx = ct.c_void_p(1)  # never dereferenced: name and ctx_len are checked first
    for alg in (b"ML-KEM-768", b"ML-DSA", b""):
        assert LIB.qrk_sig_verify_batch(ctx, alg, 1, None, None, None, None, None, 0, None, None) == -1
        assert "unsupported signature algorithm" in qrkem.last_error()
    assert LIB.qrk_sig_verify_batch(ctx, b"ML-DSA-65", 1, None, None, None, None, None, 256, None, None) == -1
    assert "255" in qrkem.last_error()
    assert LIB.qrk_sig_verify_batch(None, b"ML-DSA-65", 1, None, None, None, None, None, 0, None, None) == -1
    assert "null context" in qrkem.last_error()
    assert LIB.qrk_sig_verify_batch(ctx, b"ML-DSA-65", 0, None, None, None, None, None, 255, None, None) == 0


def test_oqs_sig_registry_stays_empty():
    from qrkem._native import LIB
    assert LIB.OQS_SIG_alg_count() == 0
    assert LIB.OQS_SIG_alg_is_enabled(b"ML-DSA-65") == 0


def test_class_keeps_the_reference_surface_and_argument_errors():
    import qrkem
    from qrkem.signatures import MLDSASignature, SignatureAlgorithm
    assert qrkem.MLDSASignature is MLDSASignature and qrkem.SignatureAlgorithm is SignatureAlgorithm
    assert sorted(SignatureAlgorithm.__abstractmethods__) == ["description", "generate_keypair", "name", "sign",
                                                              "verify"]
    assert MLDSASignature().variant == "ML-DSA-65"
    for level, variant in ((2, "ML-DSA-44"), (3, "ML-DSA-65"), (5, "ML-DSA-87")):
        s = MLDSASignature(security_level=level)
        assert isinstance(s, SignatureAlgorithm) and isinstance(s, qrkem.CryptoAlgorithm)
        assert s.name == s.display_name == f"ML-DSA (Level {level})" and s.variant == s.actual_variant == variant
        assert s.description == ("ML-DSA is a lattice-based digital signature scheme. "
                                 "It is one of the NIST post-quantum cryptography standards.")
        assert s.is_using_mock is False and s.get_security_info()["security_level"] == level
        assert (s.public_key_size, s.secret_key_size, s.signature_size) == SIZES[variant]
        with pytest.raises(NotImplementedError, match="verifies ML-DSA signatures only"):
            s.generate_keypair()
        with pytest.raises(NotImplementedError, match="verifies ML-DSA signatures only"):
            s.sign(bytes(s.secret_key_size), b"m")
        # wrong lengths: False with no GPU call (a context is never created)
        assert s.verify(bytes(s.public_key_size - 1), b"m", bytes(s.signature_size)) is False
        assert s.verify(bytes(s.public_key_size), b"m", bytes(s.signature_size + 1)) is False
        assert s.verify(b"", b"", b"") is False
        assert s._ctx is None
    for level in (1, 4, 0, "3"):
        with pytest.raises(ValueError, match=f"Invalid security level: {level}. Must be 2, 3, or 5."):
            MLDSASignature(security_level=level)


def test_verify_never_raises_without_a_gpu():
    import qrkem
    if qrkem.device_count() > 0:
        pytest.skip("GPU present")
    s = qrkem.MLDSASignature(3)
    assert s.verify(bytes(1952), b"m", bytes(3309)) is False  # logged, as the reference's except -> False
    with pytest.raises(RuntimeError, match="cannot create a context"):
        s.verify_batch([bytes(1952)], [b"m"], [bytes(3309)])
