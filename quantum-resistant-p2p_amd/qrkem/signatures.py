"""Signatures on the GPU -- the reference's ``crypto/signatures.py``: verification for ML-DSA and SPHINCS+ /
SLH-DSA, and for the hash-based family key generation and signing as well.

``SignatureAlgorithm`` keeps the three abstract methods of ``quantum_resistant_p2p/crypto/signatures.py:
18-55``, ``MLDSASignature`` the names, strings and errors of ``:58-188`` and ``SPHINCSSignature`` those of
``:191-314``.  Only ``verify`` is implemented (``qrk_sig_verify_batch``; mldsa.hip: FIPS 204 pure ML-DSA
with the empty context string, what liboqs's ``OQS_SIG_sign`` produces; slhdsa.hip: the round-3.1
``SPHINCS+-SHA2-*f-simple`` sets liboqs ships, or FIPS 205 pure SLH-DSA with ``fips205=True``);
``generate_keypair`` and ``sign`` raise ``NotImplementedError``: a node keeps signing with liboqs and
verifies the messages it receives here, in batches (:meth:`verify_batch`).  That is every default constructor.

``SPHINCSSignature(signing=True)`` implements the other half too (``qrk_sig_keypair_batch`` /
``qrk_sig_sign_batch``, slhdsa_sign.hip: FIPS 205 Algorithms 18 and 19): ``generate_keypair`` and ``sign`` as
the reference calls them, :meth:`SPHINCSSignature.generate_keypair_batch` and
:meth:`SPHINCSSignature.sign_batch` over device tensors.  Signing is hedged (a fresh ``opt_rand`` per
signature) unless ``deterministic=True``.  A node on the SPHINCS+ path then needs no liboqs.

``MLDSASigner`` does the same for ML-DSA, the reference's default signature: a subclass of ``MLDSASignature``
with ``generate_keypair`` / ``sign`` and their ``*_batch`` forms over ``qrk_mldsa_keypair_batch`` /
``qrk_mldsa_sign_batch`` (mldsa_sign.hip: FIPS 204 Algorithms 6 and 2, hedged unless ``deterministic=True``).
``MLDSASignature`` itself and the generic ``qrk_sig_keypair_batch`` / ``qrk_sig_sign_batch`` deliberately keep
refusing ML-DSA signing, so code written against the verify-only class keeps its errors.  With ``MLDSASigner``
a default node needs no liboqs for signatures either.  Like ``_native.py`` there is no CPU fallback.

A node signs with one identity key and verifies each peer's messages against that peer's one key, so both ML-DSA
classes also work on key sets (``MLDSAKeySet``, mldsa_keyed.hip): ``load_public_keys`` / ``load_secret_keys`` expand
g keys once, and ``verify_keyed`` / ``sign_keyed`` take a key index per row and return what ``verify_batch`` /
``sign_batch`` return for the same keys.
"""
from __future__ import annotations

import abc
import ctypes as ct
import logging
import os
import threading
from typing import Tuple

import numpy as np

from ._native import LIB, last_error
from .algorithm_base import CryptoAlgorithm
from .batch import _as_host, _check_dev, _is_dev
from .handshake import _dev, _ptr, pack_infos

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

logger = logging.getLogger(__name__)

VERIFY_ONLY = ("qrkem verifies ML-DSA signatures only: {} stays with liboqs "
               "(libqrkem has no ML-DSA KeyGen or Sign)")
SPHINCS_VERIFY_ONLY = ("qrkem verifies SPHINCS+ signatures only: {} stays with liboqs "
                       "(libqrkem has no SPHINCS+ / SLH-DSA KeyGen or Sign)")


class SignatureAlgorithm(CryptoAlgorithm):
    """Same abstract surface as crypto/signatures.py:18-55."""

    @abc.abstractmethod
    def generate_keypair(self) -> Tuple[bytes, bytes]:
        ...

    @abc.abstractmethod
    def sign(self, private_key: bytes, message: bytes) -> bytes:
        ...

    @abc.abstractmethod
    def verify(self, public_key: bytes, message: bytes, signature: bytes) -> bool:
        ...


def sig_sizes(variant: str) -> Tuple[int, int, int]:
    """(public key, secret key, signature) bytes of an ML-DSA or SLH-DSA / SPHINCS+ parameter set."""
    out = (ct.c_size_t * 3)()
    if LIB.qrk_sig_sizes(variant.encode(), out) != 0:
        raise ValueError(last_error())
    return int(out[0]), int(out[1]), int(out[2])


class _BatchVerifier(SignatureAlgorithm):
    """What the verifying classes share: sizes from the library, the lazily created context, scalar
    ``verify`` and the batch calls.  A subclass sets ``FAMILY`` (the name used in messages), ``VERIFY_ONLY``
    and ``variant`` before calling :meth:`_setup`."""

    FAMILY = ""
    VERIFY_ONLY = ""

    def _setup(self, device: int) -> None:
        self.device = device
        self.public_key_size, self.secret_key_size, self.signature_size = sig_sizes(self.variant)
        self._ctx = None
        self._ctx_lock = threading.Lock()

    def _context(self):
        # one context per object, whichever thread asks first: ctypes drops the GIL inside qrk_ctx_create, so
        # without the lock two first calls would each create one and the loser's would never be destroyed
        with self._ctx_lock:
            if self._ctx is None:
                h = ct.c_void_p()
                if LIB.qrk_ctx_create(ct.byref(h), self.device) != 0:
                    raise RuntimeError(f"qrkem: cannot create a context on device {self.device}: {last_error()}")
                self._ctx = h
            return self._ctx

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            LIB.qrk_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ragged(self, messages, offsets):
        """``(messages, offsets)`` as the batch methods accept them -> the validated device tensors and n."""
        if offsets is None:
            data, off = pack_infos([bytes(m) for m in messages])
            messages, offsets = _dev(data, self.device), _dev(off.view(np.int64), self.device)
        n = offsets.numel() - 1
        if not (_is_dev(messages) and messages.dtype == torch.uint8 and messages.dim() == 1 and
                messages.is_contiguous()):
            raise ValueError("messages must be a contiguous 1-D uint8 device tensor")
        if not (_is_dev(offsets) and offsets.dtype in (torch.int64, torch.uint64) and offsets.dim() == 1 and
                n >= 0 and offsets.is_contiguous()):
            raise ValueError("offsets must be a contiguous 64-bit device tensor of n + 1 entries")
        return messages, offsets, n

    # ------------------------------------------------------------------ the reference's single calls
    def generate_keypair(self) -> Tuple[bytes, bytes]:
        raise NotImplementedError(self.VERIFY_ONLY.format("key generation"))

    def sign(self, private_key: bytes, message: bytes) -> bytes:
        raise NotImplementedError(self.VERIFY_ONLY.format("signing"))

    def verify(self, public_key: bytes, message: bytes, signature: bytes) -> bool:
        """True if the signature is valid.  Never raises: a wrong-length key or signature is False
        without any GPU work, and so is any error (logged), as in the reference (signatures.py:186-188)."""
        try:
            if len(public_key) != self.public_key_size or len(signature) != self.signature_size:
                return False
            return bool(self.verify_batch([bytes(public_key)], [bytes(message)], [bytes(signature)])[0])
        except Exception as exc:
            logger.error(f"Error verifying {self.FAMILY} signature: {exc}")
            return False

    # ------------------------------------------------------------------ batches
    def verify_batch(self, public_keys, messages, signatures, offsets=None):
        """valid[i] = Verify(public_keys[i], messages[i], signatures[i]): a numpy bool array [n].

        ``public_keys`` / ``signatures``: [n, pk bytes] / [n, signature bytes] uint8 (device tensors,
        numpy arrays or lists of bytes).  ``messages``: a list of byte strings, or a 1-D uint8 device
        tensor of the messages back to back with ``offsets``, an int64 or uint64 [n + 1] device
        tensor (message i = messages[offsets[i]:offsets[i + 1]]).  Use :meth:`verify_status` to keep
        the result on the device."""
        return self.verify_status(public_keys, messages, signatures, offsets).cpu().numpy() == 0

    def verify_status(self, public_keys, messages, signatures, offsets=None):
        """As :meth:`verify_batch`, returning the int32 [n] device tensor of the C ABI: 0 valid, -1 not."""
        ctx = self._context()  # first: without a device this is the error to raise
        messages, offsets, n = self._ragged(messages, offsets)
        if not _is_dev(public_keys):
            public_keys = _dev(_as_host(public_keys, self.public_key_size), self.device)
        if not _is_dev(signatures):
            signatures = _dev(_as_host(signatures, self.signature_size), self.device)
        _check_dev(public_keys, self.public_key_size, f"{self.FAMILY} public keys", n)
        _check_dev(signatures, self.signature_size, f"{self.FAMILY} signatures", n)
        status = torch.empty((n,), dtype=torch.int32, device=messages.device)
        rc = LIB.qrk_sig_verify_batch(ctx, self.variant.encode(), n, _ptr(public_keys), _ptr(messages), _ptr(offsets),
                                      _ptr(signatures), None, 0, _ptr(status), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} verify failed ({self.variant}): {last_error()}")
        return status


class MLDSAKeySet:
    """g ML-DSA keys expanded once on the device (``qrk_mldsa_pubkeys_load`` / ``qrk_mldsa_seckeys_load``,
    mldsa_keyed.hip): what :meth:`MLDSASignature.verify_keyed` and :meth:`MLDSASigner.sign_keyed` index into.
    Made by :meth:`MLDSASignature.load_public_keys` / :meth:`MLDSASigner.load_secret_keys`; owns the handle and
    is a context manager.  A secret set holds secret-derived bytes in device memory until :meth:`close`, which
    zeroes them (the library synchronises the device first)."""

    def __init__(self, handle, variant: str, g: int, secret: bool, device: int = 0):
        self._handle = handle
        self.variant = variant
        self.g = int(g)
        self.secret = bool(secret)
        self.device = device

    @property
    def closed(self) -> bool:
        return not self._handle

    @property
    def device_bytes(self) -> int:
        """Bytes of device memory the set holds (``qrk_mldsa_keyset_info``); 0 once closed."""
        if self.closed:
            return 0
        out = (ct.c_size_t * 4)()
        if LIB.qrk_mldsa_keyset_info(self._handle, out) != 0:
            raise RuntimeError(last_error())
        return int(out[3])

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            LIB.qrk_mldsa_keyset_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self) -> str:
        kind = "secret" if self.secret else "public"
        return f"<MLDSAKeySet {self.variant} {kind} g={self.g}{' closed' if self.closed else ''}>"


class MLDSASignature(_BatchVerifier):
    """ML-DSA (FIPS 204) verification on one device.  The context is created on first use, so
    constructing the object (as the reference does at start-up, messaging.py:128) needs no GPU.

    A node that hears from a handful of peers verifies many signatures under few keys:
    :meth:`load_public_keys` expands the keys once and :meth:`verify_keyed` takes a key index per row."""

    VARIANTS = {2: "ML-DSA-44", 3: "ML-DSA-65", 5: "ML-DSA-87"}
    FAMILY = "ML-DSA"
    VERIFY_ONLY = VERIFY_ONLY

    def __init__(self, security_level: int = 3, device: int = 0):
        if security_level not in self.VARIANTS:
            raise ValueError(f"Invalid security level: {security_level}. Must be 2, 3, or 5.")
        self.security_level = security_level
        self.variant = self.VARIANTS[security_level]
        self._setup(device)

    # ------------------------------------------------------------------ key sets
    def _load_keys(self, keys, width: int, secret: bool) -> MLDSAKeySet:
        ctx = self._context()  # first: without a device this is the error to raise
        what = "secret" if secret else "public"
        if not _is_dev(keys):
            keys = _dev(_as_host(keys, width), self.device)
        _check_dev(keys, width, f"{self.FAMILY} {what} keys")
        g = keys.shape[0]
        if g == 0:
            raise ValueError(f"a key set holds at least one {what} key")
        h = ct.c_void_p()
        load = LIB.qrk_mldsa_seckeys_load if secret else LIB.qrk_mldsa_pubkeys_load
        if load(ctx, self.variant.encode(), g, _ptr(keys), ct.byref(h), self._stream()) != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} key set load failed ({self.variant}): {last_error()}")
        torch.cuda.current_stream(self.device).synchronize()  # the set is ready on every stream; `keys` may go
        return MLDSAKeySet(h, self.variant, g, secret, self.device)

    def _keyed_args(self, keyset, secret: bool, messages, offsets, key_index):
        """The checks that need no device first (ValueError), then the context, then the device tensors."""
        if not isinstance(keyset, MLDSAKeySet):
            raise ValueError("keyset must be an MLDSAKeySet")
        if keyset.variant != self.variant:
            raise ValueError(f"the key set holds {keyset.variant} keys, this object is {self.variant}")
        if keyset.secret and not secret:
            raise ValueError("a secret key set cannot verify: load the public keys with load_public_keys")
        if secret and not keyset.secret:
            raise ValueError("a public key set cannot sign: load the secret keys with load_secret_keys")
        if keyset.device != self.device:
            raise ValueError(f"the key set is on device {keyset.device}, this object on device {self.device}")
        if key_index is None and keyset.g != 1:
            raise ValueError(f"key_index may be None only for a key set of one key, this one has {keyset.g}")
        ctx = self._context()
        if keyset.closed:
            raise ValueError("the key set is closed")
        messages, offsets, n = self._ragged(messages, offsets)
        if key_index is not None:
            if not _is_dev(key_index):
                idx = np.asarray(key_index)
                if idx.ndim != 1 or idx.dtype.kind not in "iu" or (idx.size and (idx.min() < 0 or idx.max() >= 2 ** 32)):
                    raise ValueError("key_index must be a 1-D sequence of n indices in [0, 2^32)")
                key_index = _dev(idx.astype(np.uint32).view(np.int32), self.device)
            if key_index.dtype == torch.int64:
                key_index = key_index.to(torch.int32)  # an index of 2^31 or more is outside every set either way
            if not (key_index.dim() == 1 and key_index.numel() == n and key_index.is_contiguous() and
                    key_index.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("key_index must be a contiguous 1-D 32-bit device tensor of n entries")
        return ctx, messages, offsets, n, key_index

    def load_public_keys(self, public_keys) -> MLDSAKeySet:
        """A key set of the g public keys [g, pk bytes] (a device tensor, numpy array or list of bytes):
        ExpandA, tr and the NTT of t1 run once per key here and never again per signature."""
        return self._load_keys(public_keys, self.public_key_size, False)

    def verify_keyed(self, keyset, messages, signatures, key_index=None, offsets=None):
        """valid[i] = Verify(key key_index[i] of `keyset`, messages[i], signatures[i]): a numpy bool array [n],
        the same answers as :meth:`verify_batch` with that key in row i.  ``key_index``: a sequence, numpy
        array or device tensor of n indices; None (every row under key 0) only for a set of one key.  A row
        whose index is not below ``keyset.g`` is invalid.  The other arguments as in :meth:`verify_batch`."""
        return self.verify_keyed_status(keyset, messages, signatures, key_index, offsets).cpu().numpy() == 0

    def verify_keyed_status(self, keyset, messages, signatures, key_index=None, offsets=None):
        """As :meth:`verify_keyed`, returning the int32 [n] device tensor of the C ABI: 0 valid, -1 not."""
        ctx, messages, offsets, n, key_index = self._keyed_args(keyset, False, messages, offsets, key_index)
        if not _is_dev(signatures):
            signatures = _dev(_as_host(signatures, self.signature_size), self.device)
        _check_dev(signatures, self.signature_size, f"{self.FAMILY} signatures", n)
        status = torch.empty((n,), dtype=torch.int32, device=messages.device)
        rc = LIB.qrk_mldsa_verify_keyed_batch(ctx, keyset._handle, n, _ptr(key_index), _ptr(messages), _ptr(offsets),
                                              _ptr(signatures), None, 0, _ptr(status), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} keyed verify failed ({self.variant}): {last_error()}")
        return status

    @property
    def name(self) -> str:
        return f"ML-DSA (Level {self.security_level})"

    @property
    def display_name(self) -> str:
        return f"ML-DSA (Level {self.security_level})"

    @property
    def description(self) -> str:
        return ("ML-DSA is a lattice-based digital signature scheme. "
                "It is one of the NIST post-quantum cryptography standards.")


class MLDSASigner(MLDSASignature):
    """ML-DSA with key generation and signing on the GPU as well (``qrk_mldsa_keypair_batch`` /
    ``qrk_mldsa_sign_batch``, mldsa_sign.hip: FIPS 204 Algorithms 6 and 2 with the empty context string, what
    liboqs's ``OQS_SIG_sign`` produces).  ``generate_keypair`` and ``sign`` are the reference's calls
    (signatures.py:100-152); the ``*_batch`` methods work on device tensors.  Signing is hedged (32 fresh bytes of
    ``rnd`` per signature) unless ``deterministic=True`` (rnd = 32 zero bytes, which reproduces a signature bit
    for bit).  :class:`MLDSASignature` itself stays verification-only."""

    def __init__(self, security_level: int = 3, device: int = 0, deterministic: bool = False):
        super().__init__(security_level, device)
        self.deterministic = bool(deterministic)

    def generate_keypair(self) -> Tuple[bytes, bytes]:
        """(public key, secret key) from 32 fresh bytes of the OS CSPRNG."""
        pk, sk = self.generate_keypair_batch(1)
        return pk[0].cpu().numpy().tobytes(), sk[0].cpu().numpy().tobytes()

    def sign(self, private_key: bytes, message: bytes) -> bytes:
        """The signature of `message`.  Unlike ``verify`` this raises on any error, as the reference's does."""
        ctx = self._context()  # noqa: F841  (first: without a device this is the error to raise)
        if len(private_key) != self.secret_key_size:
            raise ValueError(f"{self.FAMILY} secret keys of {self.variant} have {self.secret_key_size} bytes, "
                             f"got {len(private_key)}")
        return self.sign_batch([bytes(private_key)], [bytes(message)])[0].cpu().numpy().tobytes()

    def generate_keypair_batch(self, n: int, seeds=None):
        """n key pairs: device tensors (pk [n, pk bytes], sk [n, sk bytes]).  ``seeds``: [n, 32] uint8, the xi of
        FIPS 204 Algorithm 6 per row (a device tensor, numpy array or list of bytes); None draws them from
        ``os.urandom``."""
        ctx = self._context()
        if seeds is None:
            seeds = np.frombuffer(os.urandom(n * 32), np.uint8).reshape(n, 32)
        if not _is_dev(seeds):
            seeds = _dev(_as_host(seeds, 32), self.device)
        _check_dev(seeds, 32, f"{self.FAMILY} key seeds", n)
        pk = torch.empty((n, self.public_key_size), dtype=torch.uint8, device=seeds.device)
        sk = torch.empty((n, self.secret_key_size), dtype=torch.uint8, device=seeds.device)
        rc = LIB.qrk_mldsa_keypair_batch(ctx, self.variant.encode(), n, _ptr(seeds), _ptr(pk), _ptr(sk), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} key generation failed ({self.variant}): {last_error()}")
        return pk, sk

    def sign_batch(self, private_keys, messages, offsets=None, rnd=None, return_status: bool = False):
        """sig[i] = Sign(private_keys[i], messages[i]): a uint8 device tensor [n, signature bytes].

        ``private_keys`` [n, sk bytes] and ``messages`` / ``offsets`` as in :meth:`verify_status`.  ``rnd``
        [n, 32]: the per-row randomiser; None draws it from ``os.urandom``, or uses 32 zero bytes (the
        deterministic variant of FIPS 204) if the object was made with ``deterministic=True``.  A row the
        library refuses (status -1: offsets that decrease, 2^31 bytes or more, a corrupt key, or a rejection
        loop that reached its cap of 814 iterations) has an all-zero signature; that raises ``RuntimeError``
        unless ``return_status=True``, which returns ``(signatures, status)`` with the int32 [n] device tensor
        instead."""
        ctx = self._context()
        messages, offsets, n = self._ragged(messages, offsets)
        if not _is_dev(private_keys):
            private_keys = _dev(_as_host(private_keys, self.secret_key_size), self.device)
        _check_dev(private_keys, self.secret_key_size, f"{self.FAMILY} secret keys", n)
        if rnd is None and not self.deterministic:
            rnd = np.frombuffer(os.urandom(n * 32), np.uint8).reshape(n, 32)
        if rnd is not None:
            if not _is_dev(rnd):
                rnd = _dev(_as_host(rnd, 32), self.device)
            _check_dev(rnd, 32, f"{self.FAMILY} rnd", n)
        sig = torch.empty((n, self.signature_size), dtype=torch.uint8, device=messages.device)
        status = torch.empty((n,), dtype=torch.int32, device=messages.device)
        rc = LIB.qrk_mldsa_sign_batch(ctx, self.variant.encode(), n, _ptr(private_keys), _ptr(messages), _ptr(offsets),
                                      _ptr(rnd), None, 0, _ptr(sig), _ptr(status), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} sign failed ({self.variant}): {last_error()}")
        if return_status:
            return sig, status
        bad = int((status != 0).sum())  # the one host wait of this path
        if bad:
            raise RuntimeError(f"qrkem {self.FAMILY} sign failed ({self.variant}): {bad} of {n} rows were refused "
                               "(corrupt secret key, malformed message offsets, or the iteration cap)")
        return sig

    def load_secret_keys(self, private_keys) -> MLDSAKeySet:
        """A key set of the g secret keys [g, sk bytes]: ExpandA, skDecode and the NTTs of s1, s2 and t0 run once
        per key.  The set keeps K and those NTTs in device memory until it is closed, which zeroes them."""
        return self._load_keys(private_keys, self.secret_key_size, True)

    def sign_keyed(self, keyset, messages, key_index=None, offsets=None, rnd=None, return_status: bool = False):
        """sig[i] = Sign(key key_index[i] of `keyset`, messages[i]): a uint8 device tensor [n, signature bytes],
        byte for byte what :meth:`sign_batch` gives with that key in row i.  ``key_index`` as in
        :meth:`verify_keyed`; ``rnd`` and ``return_status`` as in :meth:`sign_batch`.  A row is refused (status
        -1, an all-zero signature) for the reasons listed there, and when its index is not below ``keyset.g``."""
        ctx, messages, offsets, n, key_index = self._keyed_args(keyset, True, messages, offsets, key_index)
        if rnd is None and not self.deterministic:
            rnd = np.frombuffer(os.urandom(n * 32), np.uint8).reshape(n, 32)
        if rnd is not None:
            if not _is_dev(rnd):
                rnd = _dev(_as_host(rnd, 32), self.device)
            _check_dev(rnd, 32, f"{self.FAMILY} rnd", n)
        sig = torch.empty((n, self.signature_size), dtype=torch.uint8, device=messages.device)
        status = torch.empty((n,), dtype=torch.int32, device=messages.device)
        rc = LIB.qrk_mldsa_sign_keyed_batch(ctx, keyset._handle, n, _ptr(key_index), _ptr(messages), _ptr(offsets),
                                            _ptr(rnd), None, 0, _ptr(sig), _ptr(status), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} keyed sign failed ({self.variant}): {last_error()}")
        if return_status:
            return sig, status
        bad = int((status != 0).sum())  # the one host wait of this path
        if bad:
            raise RuntimeError(f"qrkem {self.FAMILY} sign failed ({self.variant}): {bad} of {n} rows were refused "
                               "(corrupt secret key, key index outside the set, malformed message offsets, or the "
                               "iteration cap)")
        return sig


class SPHINCSSignature(_BatchVerifier):
    """SPHINCS+ / SLH-DSA on one device, the SHA2 "f" parameter sets.  By default the variant is the round-3.1
    ``SPHINCS+-SHA2-*f-simple`` name the reference asks liboqs for (signatures.py:208-212); ``fips205=True``
    selects FIPS 205 pure SLH-DSA with the empty context string instead.  As for ML-DSA the context is created
    on first use.  Verification only by default; ``signing=True`` adds key generation and signing on the GPU
    (hedged; ``deterministic=True`` signs with opt_rand = PK.seed, which reproduces a signature bit for bit)."""

    VARIANTS = {1: "SPHINCS+-SHA2-128f-simple", 3: "SPHINCS+-SHA2-192f-simple", 5: "SPHINCS+-SHA2-256f-simple"}
    FIPS_VARIANTS = {1: "SLH-DSA-SHA2-128f", 3: "SLH-DSA-SHA2-192f", 5: "SLH-DSA-SHA2-256f"}
    FAMILY = "SPHINCS+"
    VERIFY_ONLY = SPHINCS_VERIFY_ONLY

    def __init__(self, security_level: int = 3, device: int = 0, fips205: bool = False, signing: bool = False,
                 deterministic: bool = False):
        if security_level not in self.VARIANTS:
            raise ValueError(f"Invalid security level: {security_level}. Must be 1, 3, or 5.")
        self.security_level = security_level
        self.fips205 = bool(fips205)
        self.signing = bool(signing)
        self.deterministic = bool(deterministic)
        self.variant = (self.FIPS_VARIANTS if self.fips205 else self.VARIANTS)[security_level]
        self._setup(device)
        self.n_bytes = self.public_key_size // 2

    # ------------------------------------------------------------------ key generation and signing (signing=True)
    def generate_keypair(self) -> Tuple[bytes, bytes]:
        """(public key, secret key) from 3 n fresh bytes of the OS CSPRNG (signatures.py:238-259)."""
        if not self.signing:
            return super().generate_keypair()
        pk, sk = self.generate_keypair_batch(1)
        return pk[0].cpu().numpy().tobytes(), sk[0].cpu().numpy().tobytes()

    def sign(self, private_key: bytes, message: bytes) -> bytes:
        """The signature of `message`.  Unlike ``verify`` this raises on any error, as the reference's does
        (signatures.py:290-292)."""
        if not self.signing:
            return super().sign(private_key, message)
        ctx = self._context()  # noqa: F841  (first: without a device this is the error to raise)
        if len(private_key) != self.secret_key_size:
            raise ValueError(f"{self.FAMILY} secret keys of {self.variant} have {self.secret_key_size} bytes, "
                             f"got {len(private_key)}")
        return self.sign_batch([bytes(private_key)], [bytes(message)])[0].cpu().numpy().tobytes()

    def generate_keypair_batch(self, n: int, seeds=None):
        """n key pairs: device tensors (pk [n, pk bytes], sk [n, sk bytes]).  ``seeds``: [n, 3 n_bytes] uint8 =
        SK.seed || SK.prf || PK.seed per row (a device tensor, numpy array or list of bytes); None draws them
        from ``os.urandom``."""
        if not self.signing:
            return super().generate_keypair()
        ctx = self._context()
        width = 3 * self.n_bytes
        if seeds is None:
            seeds = np.frombuffer(os.urandom(n * width), np.uint8).reshape(n, width)
        if not _is_dev(seeds):
            seeds = _dev(_as_host(seeds, width), self.device)
        _check_dev(seeds, width, f"{self.FAMILY} key seeds", n)
        pk = torch.empty((n, self.public_key_size), dtype=torch.uint8, device=seeds.device)
        sk = torch.empty((n, self.secret_key_size), dtype=torch.uint8, device=seeds.device)
        rc = LIB.qrk_sig_keypair_batch(ctx, self.variant.encode(), n, _ptr(seeds), _ptr(pk), _ptr(sk), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} key generation failed ({self.variant}): {last_error()}")
        return pk, sk

    def sign_batch(self, private_keys, messages, offsets=None, opt_rand=None, return_status: bool = False):
        """sig[i] = Sign(private_keys[i], messages[i]): a uint8 device tensor [n, signature bytes].

        ``private_keys`` [n, sk bytes] and ``messages`` / ``offsets`` as in :meth:`verify_status`.  ``opt_rand``
        [n, n_bytes]: the per-row randomiser; None draws it from ``os.urandom``, or uses PK.seed (the
        deterministic variant of FIPS 205) if the object was made with ``deterministic=True``.  A row the
        library refuses (status -1: offsets that decrease, 2^31 bytes or more, a corrupt key) has an all-zero
        signature; that raises ``RuntimeError`` unless ``return_status=True``, which returns
        ``(signatures, status)`` with the int32 [n] device tensor instead."""
        if not self.signing:
            return super().sign(b"", b"")
        ctx = self._context()
        messages, offsets, n = self._ragged(messages, offsets)
        if not _is_dev(private_keys):
            private_keys = _dev(_as_host(private_keys, self.secret_key_size), self.device)
        _check_dev(private_keys, self.secret_key_size, f"{self.FAMILY} secret keys", n)
        if opt_rand is None and not self.deterministic:
            opt_rand = np.frombuffer(os.urandom(n * self.n_bytes), np.uint8).reshape(n, self.n_bytes)
        if opt_rand is not None:
            if not _is_dev(opt_rand):
                opt_rand = _dev(_as_host(opt_rand, self.n_bytes), self.device)
            _check_dev(opt_rand, self.n_bytes, f"{self.FAMILY} opt_rand", n)
        sig = torch.empty((n, self.signature_size), dtype=torch.uint8, device=messages.device)
        status = torch.empty((n,), dtype=torch.int32, device=messages.device)
        rc = LIB.qrk_sig_sign_batch(ctx, self.variant.encode(), n, _ptr(private_keys), _ptr(messages), _ptr(offsets),
                                    _ptr(opt_rand), None, 0, _ptr(sig), _ptr(status), self._stream())
        if rc != 0:
            raise RuntimeError(f"qrkem {self.FAMILY} sign failed ({self.variant}): {last_error()}")
        if return_status:
            return sig, status
        bad = int((status != 0).sum())  # the one host wait of this path
        if bad:
            raise RuntimeError(f"qrkem {self.FAMILY} sign failed ({self.variant}): {bad} of {n} rows were refused "
                               "(corrupt secret key or malformed message offsets)")
        return sig

    @property
    def name(self) -> str:
        return f"SPHINCS+ (Level {self.security_level})"

    @property
    def display_name(self) -> str:
        return f"SPHINCS+ (Level {self.security_level})"

    @property
    def description(self) -> str:
        return ("SPHINCS+ is a stateless hash-based digital signature scheme. "
                "Its security relies only on the security of the underlying hash functions.")
