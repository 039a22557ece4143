"""CPU: the AEAD entry points are exported, declared and bound, refuse unknown algorithm names, and the
reference-shaped classes check their arguments before any GPU work."""
import ctypes as ct

import pytest

from test_abi import declared_functions, exported_symbols

AEAD_SYMBOLS = ("qrk_aead_seal_batch", "qrk_aead_open_batch")
HOOKS = ("qrk_dbg_poly1305_batch", "qrk_dbg_ghash_batch")


def test_aead_symbols_exported_declared_and_bound():
    from qrkem._native import LIB
    exported = exported_symbols()
    declared = declared_functions()
    for name in AEAD_SYMBOLS:
        assert name in exported and name in declared
        assert getattr(LIB, name).argtypes is not None and len(getattr(LIB, name).argtypes) == 12
    for name in HOOKS:  # test hooks: exported, kept out of the public header
        assert name in exported and name not in declared


def test_unknown_aead_name_is_refused_before_any_device_work():
    import qrkem
    from qrkem._native import LIB
    ctx = ct.c_void_p(1)  # never dereferenced: the name is checked first
    for alg in (b"AES-128-GCM", b"aes-256-gcm", b"ChaCha20", b""):
        assert LIB.qrk_aead_seal_batch(ctx, alg, 1, None, None, None, None, None, None, 0, None, None) == -1
        assert "unsupported AEAD" in qrkem.last_error()
        assert LIB.qrk_aead_open_batch(ctx, alg, 1, None, None, None, None, None, 0, None, None, None) == -1
        assert "unsupported AEAD" in qrkem.last_error()
    assert LIB.qrk_aead_seal_batch(None, b"AES-256-GCM", 1, None, None, None, None, None, None, 0, None, None) == -1
    assert "null context" in qrkem.last_error()


def test_classes_keep_the_reference_surface_and_argument_errors():
    import qrkem
    from qrkem.handshake import SYMMETRIC_KEY_SIZE
    from qrkem.symmetric import BY_NAME, SymmetricAlgorithm
    assert sorted(BY_NAME) == sorted(SYMMETRIC_KEY_SIZE)
    assert qrkem.AES256GCM is BY_NAME["AES-256-GCM"] and qrkem.ChaCha20Poly1305 is BY_NAME["ChaCha20-Poly1305"]
    assert sorted(SymmetricAlgorithm.__abstractmethods__) == ["decrypt", "description", "encrypt", "generate_key",
                                                              "key_size", "name"]
    for name, cls in BY_NAME.items():
        a = cls()
        assert isinstance(a, SymmetricAlgorithm) and isinstance(a, qrkem.CryptoAlgorithm)
        assert a.name == a.display_name == name and a.key_size == SYMMETRIC_KEY_SIZE[name] == 32
        assert a.is_using_mock is False and a.description
        assert a.get_security_info() == {"name": name, "mock_implementation": False, "description": a.description}
        key = a.generate_key()
        assert len(key) == 32 and key != a.generate_key()
        with pytest.raises(ValueError, match="Key must be 32 bytes, got 31"):
            a.encrypt(bytes(31), b"x")
        with pytest.raises(ValueError, match="Key must be 32 bytes, got 33"):
            a.decrypt(bytes(33), bytes(40))
        with pytest.raises(ValueError, match="Ciphertext too short: 11 bytes"):
            a.decrypt(key, bytes(11))


def test_no_cpu_fallback_for_aead():
    import qrkem
    if qrkem.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="cannot create a context"):
        qrkem.AES256GCM().encrypt(bytes(32), b"hello")
