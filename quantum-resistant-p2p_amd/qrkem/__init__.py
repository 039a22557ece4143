"""qrkem -- MI355X-native batched post-quantum key exchange.

Host-side mirror of the reference's KEM path (``quantum_resistant_p2p/crypto/
key_exchange.py`` + ``vendor/oqs.py``) over ``libqrkem.so`` (hand-written HIP
for gfx950).  Importing this package loads the library and raises
``RuntimeError`` if it is missing: there is no CPU fallback.
"""
from ._native import LIB, LIB_PATH, last_error  # noqa: F401
from . import oqs  # noqa: F401
from .algorithm_base import CryptoAlgorithm  # noqa: F401
from .key_exchange import (  # noqa: F401
    FrodoKEMKeyExchange,
    HQCKeyExchange,
    KeyExchangeAlgorithm,
    KyberKeyExchange,
    MLKEMKeyExchange,
)


# The symmetric layer (crypto/symmetric.py's surface over aead.hip) is re-exported on first use:
# its module needs torch for device buffers, which `import qrkem` alone does not load.
_SYMMETRIC = ("SymmetricAlgorithm", "AES256GCM", "ChaCha20Poly1305")
# ... and so is the signature layer (crypto/signatures.py's surface over mldsa.hip, mldsa_sign.hip,
# mldsa_keyed.hip, slhdsa.hip and slhdsa_sign.hip)
_SIGNATURES = ("SignatureAlgorithm", "MLDSASignature", "MLDSASigner", "MLDSAKeySet", "SPHINCSSignature")


# ML-KEM key sets (batch.py over mlkem_keyed.hip): BatchKEM.load_public_keys / encaps_keyed and their secret halves
# ... and FrodoKEM key sets (frodo_keyed.hip): FrodoBatchKEM, a BatchKEM whose keyed methods take a FrodoKeySet
_BATCH = ("BatchKEM", "MLKEMKeySet", "FrodoBatchKEM", "FrodoKeySet")


def __getattr__(name: str):
    if name in _BATCH or name == "batch":
        import importlib
        mod = importlib.import_module(".batch", __name__)
        return mod if name == "batch" else getattr(mod, name)
    if name in _SYMMETRIC or name == "symmetric":
        import importlib
        mod = importlib.import_module(".symmetric", __name__)
        return mod if name == "symmetric" else getattr(mod, name)
    if name in _SIGNATURES or name == "signatures":
        import importlib
        mod = importlib.import_module(".signatures", __name__)
        return mod if name == "signatures" else getattr(mod, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def device_count() -> int:
    return int(LIB.qrk_device_count())
