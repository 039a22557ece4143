"""Symmetric authenticated encryption on the GPU -- the reference's ``crypto/symmetric.py`` surface.

``SymmetricAlgorithm``, ``AES256GCM`` and ``ChaCha20Poly1305`` keep the contract of
``quantum_resistant_p2p/crypto/symmetric.py:19-260``: ``name``, ``key_size == 32``, ``generate_key()``,
``encrypt(key, plaintext, associated_data=None)`` returning nonce (12) || ciphertext || tag (16) and
``decrypt(key, ciphertext, associated_data=None)``, with the same ``ValueError``s.  The single calls are
n = 1 batches of ``qrk_aead_seal_batch`` / ``qrk_aead_open_batch`` (aead.hip); like ``_native.py`` there
is no CPU fallback.  Each class adds ``encrypt_batch`` / ``decrypt_batch`` over n keys at once.  Where the
host knows the longest row and it reaches ``long_min_bytes``, the same calls go through
``qrk_aead_seal_long_batch`` / ``qrk_aead_open_long_batch`` (aead_long.hip: one row across many workgroups)
and return the same bytes.

Ragged batches travel as :class:`PackedRows` (concatenated bytes plus n + 1 offsets on the device), the
packing :func:`qrkem.handshake.pack_infos` / :class:`qrkem.handshake.PackedInfos` use for HKDF infos.
"""
from __future__ import annotations

import abc
import ctypes as ct
import os
import threading
from typing import Optional, Sequence, Union

import numpy as np

from ._native import LIB, last_error
from .algorithm_base import CryptoAlgorithm
from .batch import _as_host, _check_dev, _is_dev
from .handshake import PackedInfos, _dev, _ptr, pack_infos

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

NONCE_LEN, TAG_LEN = 12, 16
OVERHEAD = NONCE_LEN + TAG_LEN
AUTH_ERROR = "Authentication failed or decryption error"  # symmetric.py:161, 259


class PackedRows:
    """n byte strings on the device: ``data`` (uint8, 1-D, the rows back to back), ``off`` (int64
    [n + 1], row i = data[off[i]:off[i + 1]]) and ``total`` = off[n], known to the host."""

    def __init__(self, data, off, n: int, total: int):
        if not (_is_dev(data) and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()):
            raise ValueError("rows: data must be a contiguous 1-D uint8 device tensor")
        if not (_is_dev(off) and off.dtype == torch.int64 and tuple(off.shape) == (n + 1,) and off.is_contiguous()):
            raise ValueError(f"rows: off must be a contiguous int64 device tensor of {n + 1} offsets")
        if data.numel() < max(total, 1):
            raise ValueError(f"rows: data holds {data.numel()} bytes, the offsets need {total}")
        self.data, self.off, self.n, self.total = data, off, n, total

    @classmethod
    def from_list(cls, rows: Sequence[bytes], device: int) -> "PackedRows":
        data, off = pack_infos([bytes(x) for x in rows])
        return cls(_dev(data, device), _dev(off.view(np.int64), device), len(rows), int(off[-1]))

    @classmethod
    def from_matrix(cls, t) -> "PackedRows":
        """Equal-length rows: a contiguous [n, L] uint8 device tensor (no copy for L > 0)."""
        _check_dev(t, t.shape[1] if t.dim() == 2 else -1, "rows")
        n, width = t.shape
        off = torch.arange(n + 1, dtype=torch.int64, device=t.device) * width
        data = t.reshape(-1) if n * width else torch.zeros(1, dtype=torch.uint8, device=t.device)
        return cls(data, off, n, n * width)

    def shifted(self, per_row: int, data) -> "PackedRows":
        """The layout of the C ABI's outputs: row i moved by per_row * i bytes (+28 sealed, -28 opened)."""
        step = torch.arange(self.n + 1, dtype=torch.int64, device=self.off.device) * per_row
        return PackedRows(data, self.off + step, self.n, self.total + per_row * self.n)

    def to_list(self) -> list:
        data, off = self.data.cpu().numpy(), self.off.cpu().numpy()
        return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(self.n)]


def _keys_dev(keys, n: Optional[int], device: int):
    if not _is_dev(keys):
        keys = _dev(_as_host(keys, 32), device)
    return _check_dev(keys, 32, "AEAD keys", n)


def _aad(associated_data, n: int, device: int) -> Optional[PackedInfos]:
    if associated_data is None or isinstance(associated_data, PackedInfos):
        inf = associated_data
    else:
        inf = PackedInfos(associated_data, n, device)
    if inf is not None and inf.off is not None and inf.n != n:
        raise ValueError(f"{inf.n} associated-data strings for {n} rows")
    return inf


def _stream(device: int) -> ct.c_void_p:
    return ct.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def seal_rows(ctx, alg: str, device: int, keys, rows: PackedRows, aad: Optional[PackedInfos], nonces) -> PackedRows:
    """qrk_aead_seal_batch over device buffers: row i of the result = nonce || ct || tag."""
    n = rows.n
    _check_dev(keys, 32, "AEAD keys", n)
    if nonces is not None:
        _check_dev(nonces, NONCE_LEN, "AEAD nonces", n)
    out = torch.empty((max(rows.total + OVERHEAD * n, 1),), dtype=torch.uint8, device=rows.data.device)
    rc = LIB.qrk_aead_seal_batch(ctx, alg.encode(), n, _ptr(keys), _ptr(nonces), _ptr(rows.data), _ptr(rows.off),
                                 _ptr(aad.data) if aad else None, _ptr(aad.off) if aad else None,
                                 aad.length if aad else 0, _ptr(out), _stream(device))
    if rc != 0:
        raise RuntimeError(f"qrkem AEAD seal failed ({alg}): {last_error()}")
    return rows.shifted(OVERHEAD, out)


def open_rows(ctx, alg: str, device: int, keys, sealed: PackedRows, aad: Optional[PackedInfos]):
    """qrk_aead_open_batch over device buffers: (plaintext rows, int32 status [n]: 0 or -1).  Every row
    of `sealed` must have its 28 bytes of overhead (qrkem.h: the offsets of the rows after a shorter one
    would overlap); :meth:`_GpuAEAD.decrypt_batch` pads such rows before it packs them."""
    n = sealed.n
    _check_dev(keys, 32, "AEAD keys", n)
    if sealed.total < OVERHEAD * n:
        raise ValueError(f"{n} sealed rows need at least {OVERHEAD * n} bytes, got {sealed.total}")
    # plaintext i ends at off[i + 1] - 28 (i + 1) <= total - 28, whatever the row lengths
    out = torch.empty((max(sealed.total - OVERHEAD, 1),), dtype=torch.uint8, device=sealed.data.device)
    status = torch.empty((n,), dtype=torch.int32, device=sealed.data.device)
    rc = LIB.qrk_aead_open_batch(ctx, alg.encode(), n, _ptr(keys), _ptr(sealed.data), _ptr(sealed.off),
                                 _ptr(aad.data) if aad else None, _ptr(aad.off) if aad else None,
                                 aad.length if aad else 0, _ptr(out), _ptr(status), _stream(device))
    if rc != 0:
        raise RuntimeError(f"qrkem AEAD open failed ({alg}): {last_error()}")
    return sealed.shifted(-OVERHEAD, out), status


def seal_rows_long(ctx, alg: str, device: int, keys, rows: PackedRows, aad: Optional[PackedInfos], nonces,
                   max_len: int) -> PackedRows:
    """:func:`seal_rows` through qrk_aead_seal_long_batch.  ``max_len`` (1 .. 2^31 - 1): the caller's bound on
    any row's plaintext length; a longer row is left unwritten."""
    n = rows.n
    _check_dev(keys, 32, "AEAD keys", n)
    if nonces is not None:
        _check_dev(nonces, NONCE_LEN, "AEAD nonces", n)
    out = torch.empty((max(rows.total + OVERHEAD * n, 1),), dtype=torch.uint8, device=rows.data.device)
    rc = LIB.qrk_aead_seal_long_batch(ctx, alg.encode(), n, _ptr(keys), _ptr(nonces), _ptr(rows.data),
                                      _ptr(rows.off), _ptr(aad.data) if aad else None,
                                      _ptr(aad.off) if aad else None, aad.length if aad else 0, max_len,
                                      _ptr(out), _stream(device))
    if rc != 0:
        raise RuntimeError(f"qrkem AEAD seal failed ({alg}): {last_error()}")
    return rows.shifted(OVERHEAD, out)


def open_rows_long(ctx, alg: str, device: int, keys, sealed: PackedRows, aad: Optional[PackedInfos], max_len: int):
    """:func:`open_rows` through qrk_aead_open_long_batch.  ``max_len``: the bound on any row's plaintext
    length (its sealed length less 28); a longer row gets status -1 and nothing is written for it."""
    n = sealed.n
    _check_dev(keys, 32, "AEAD keys", n)
    if sealed.total < OVERHEAD * n:
        raise ValueError(f"{n} sealed rows need at least {OVERHEAD * n} bytes, got {sealed.total}")
    out = torch.empty((max(sealed.total - OVERHEAD, 1),), dtype=torch.uint8, device=sealed.data.device)
    status = torch.empty((n,), dtype=torch.int32, device=sealed.data.device)
    rc = LIB.qrk_aead_open_long_batch(ctx, alg.encode(), n, _ptr(keys), _ptr(sealed.data), _ptr(sealed.off),
                                      _ptr(aad.data) if aad else None, _ptr(aad.off) if aad else None,
                                      aad.length if aad else 0, max_len, _ptr(out), _ptr(status), _stream(device))
    if rc != 0:
        raise RuntimeError(f"qrkem AEAD open failed ({alg}): {last_error()}")
    return sealed.shifted(-OVERHEAD, out), status


# The longest row from which the long calls are faster than the one-lane calls for Seal and for Open, both
# AEADs, at every larger measured size, rounded up to a power of two (tools/aead_long_bench.py on one MI355X,
# profiles/aead_long/bench.jsonl; DESIGN.md section 4 has the table).
LONG_MIN_BYTES = 1 << 12
# ... in batches of at most this many rows, the largest batch measured (the long calls won there too).  Above it
# every row keeps its own lane: nothing was measured there.
LONG_MAX_ROWS = 64


def _longest(rows, overhead: int = 0) -> Optional[int]:
    """The longest row's payload length where the host knows it without a device read: a list of byte
    strings or an [n, L] tensor; None for PackedRows (its caller passes ``max_len=``)."""
    if isinstance(rows, PackedRows):
        return None
    if _is_dev(rows):
        return max(int(rows.shape[1]) - overhead, 0) if rows.dim() == 2 else None
    return max((len(x) - overhead for x in rows), default=0)


def _rows_in(rows, device: int):
    """(PackedRows, kind) of a list of byte strings, an [n, L] device tensor or PackedRows."""
    if isinstance(rows, PackedRows):
        return rows, "packed"
    if _is_dev(rows):
        return PackedRows.from_matrix(rows), "matrix"
    return PackedRows.from_list(rows, device), "list"


def _rows_out(rows: PackedRows, kind: str):
    if kind == "packed":
        return rows
    if kind == "matrix":
        return rows.data[:rows.total].reshape(rows.n, rows.total // rows.n if rows.n else 0)
    return rows.to_list()


class SymmetricAlgorithm(CryptoAlgorithm):
    """Same abstract surface as crypto/symmetric.py:19-63."""

    @property
    @abc.abstractmethod
    def key_size(self) -> int:
        ...

    @abc.abstractmethod
    def generate_key(self) -> bytes:
        ...

    @abc.abstractmethod
    def encrypt(self, key: bytes, plaintext: bytes, associated_data: Optional[bytes] = None) -> bytes:
        ...

    @abc.abstractmethod
    def decrypt(self, key: bytes, ciphertext: bytes, associated_data: Optional[bytes] = None) -> bytes:
        ...


class _GpuAEAD(SymmetricAlgorithm):
    """One AEAD of libqrkem on one device.  The context is created on first use, so constructing the
    object (as the reference does at start-up, messaging.py:127) needs no GPU; using it does."""

    _ALG = ""
    #: rows at least this long (known to the host: a list, an [n, L] tensor, or ``max_len=`` beside
    #: PackedRows) go through the long calls; None: never, 0: always.  Same bytes either way.
    long_min_bytes: Optional[int] = LONG_MIN_BYTES
    #: ... when the batch has at most this many rows
    long_max_rows: int = LONG_MAX_ROWS

    def __init__(self, device: int = 0):
        self.device = device
        self._ctx = None
        self._ctx_lock = threading.Lock()

    def _long(self, longest: Optional[int], n: int) -> Optional[int]:
        """The ``max_len`` to call the long pair with, or None for the one-lane pair."""
        if self.long_min_bytes is None or longest is None or longest < self.long_min_bytes or n > self.long_max_rows:
            return None
        if longest >> 31:
            raise ValueError("AEAD rows are at most 2^31 - 1 bytes")
        return max(int(longest), 1)

    @property
    def name(self) -> str:
        return self._ALG

    @property
    def key_size(self) -> int:
        return 32

    def generate_key(self) -> bytes:
        return os.urandom(self.key_size)

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

    def _check_key(self, key: bytes) -> None:
        if len(key) != self.key_size:
            raise ValueError(f"Key must be {self.key_size} bytes, got {len(key)}")

    # ------------------------------------------------------------------ the reference's single calls
    def encrypt(self, key: bytes, plaintext: bytes, associated_data: Optional[bytes] = None) -> bytes:
        """nonce || ciphertext || tag under a fresh random 96-bit nonce (an n = 1 batch)."""
        self._check_key(key)
        return self.encrypt_batch([bytes(key)], [bytes(plaintext)], associated_data)[0]

    def decrypt(self, key: bytes, ciphertext: bytes, associated_data: Optional[bytes] = None) -> bytes:
        self._check_key(key)
        if len(ciphertext) < NONCE_LEN:
            raise ValueError(f"Ciphertext too short: {len(ciphertext)} bytes, need at least 12 bytes for nonce")
        plain, status = self.decrypt_batch([bytes(key)], [bytes(ciphertext)], associated_data)
        if int(status[0]) != 0:
            raise ValueError(AUTH_ERROR)
        return plain[0]

    # ------------------------------------------------------------------ batches
    def encrypt_batch(self, keys, plaintexts, associated_data=None, nonces=None, max_len: Optional[int] = None):
        """Seal plaintexts[i] under keys[i]: row i = nonce || ciphertext || tag.

        ``keys``: [n, 32] uint8 (device tensor, numpy array or list of bytes).  ``plaintexts``: a list
        of byte strings (-> list of bytes), an [n, L] device tensor (-> [n, L + 28] device tensor) or
        :class:`PackedRows` (-> PackedRows).  ``associated_data``: None, one byte string for all rows,
        one per row, or a :class:`PackedInfos`.  ``nonces``: [n, 12] or None (OS CSPRNG); a caller
        that supplies them must never reuse one under the same key.  ``max_len``: with PackedRows, the
        caller's bound on any row's length, which lets the call take the long path (a row above it is
        then left unwritten); for the other forms the host knows the longest row itself."""
        ctx = self._context()  # first: without a device this is the error to raise
        longest = _longest(plaintexts)
        rows, kind = _rows_in(plaintexts, self.device)
        keys = _keys_dev(keys, rows.n, self.device)
        if nonces is not None and not _is_dev(nonces):
            nonces = _dev(_as_host(nonces, NONCE_LEN), self.device)
        aad = _aad(associated_data, rows.n, self.device)
        bound = self._long(max_len if kind == "packed" else longest, rows.n)
        if bound is None:
            out = seal_rows(ctx, self._ALG, self.device, keys, rows, aad, nonces)
        else:
            out = seal_rows_long(ctx, self._ALG, self.device, keys, rows, aad, nonces, bound)
        return _rows_out(out, kind)

    def decrypt_batch(self, keys, sealed, associated_data=None, max_len: Optional[int] = None):
        """Open sealed[i] under keys[i]: (plaintexts, status), status int32 [n] = 0, or -1 where the row
        is shorter than 28 bytes or does not verify.  Failed rows come back as zeros (a list row
        shorter than 28 bytes as b""): no unauthenticated plaintext is returned.  Input and output
        forms as :meth:`encrypt_batch`; status is a numpy array for list input, else a device tensor.
        ``max_len``: with PackedRows, the bound on any row's plaintext length (as :meth:`encrypt_batch`;
        a row above it gets status -1)."""
        ctx = self._context()
        short = None
        if not isinstance(sealed, PackedRows) and not _is_dev(sealed):
            # a row without its 28 bytes of overhead is refused here and sent as 28 zero bytes, so that
            # the C ABI's offset rule (plaintext i at sealed_off[i] - 28 i) holds for the rows after it
            sealed = [bytes(x) for x in sealed]
            short = np.array([len(x) < OVERHEAD for x in sealed], dtype=bool)
            sealed = [bytes(OVERHEAD) if s else x for x, s in zip(sealed, short)]
        longest = _longest(sealed, OVERHEAD)
        rows, kind = _rows_in(sealed, self.device)
        if kind == "matrix" and rows.n and rows.total // rows.n < OVERHEAD:
            raise ValueError(f"sealed rows must have at least {OVERHEAD} bytes")
        keys = _keys_dev(keys, rows.n, self.device)
        aad = _aad(associated_data, rows.n, self.device)
        bound = self._long(max_len if kind == "packed" else longest, rows.n)
        if bound is None:
            out, status = open_rows(ctx, self._ALG, self.device, keys, rows, aad)
        else:
            out, status = open_rows_long(ctx, self._ALG, self.device, keys, rows, aad, bound)
        if kind != "list":
            return _rows_out(out, kind), status
        status = status.cpu().numpy()
        status[short] = -1
        return out.to_list(), status


class AES256GCM(_GpuAEAD):
    """AES-256-GCM (NIST SP 800-38D), 96-bit nonce, 128-bit tag."""

    _ALG = "AES-256-GCM"

    @property
    def description(self) -> str:
        return ("AES with a 256-bit key in Galois/Counter Mode: counter-mode encryption with a GHASH "
                "authentication tag (NIST SP 800-38D), run in batches on the GPU.")


class ChaCha20Poly1305(_GpuAEAD):
    """ChaCha20-Poly1305 (RFC 8439)."""

    _ALG = "ChaCha20-Poly1305"

    @property
    def description(self) -> str:
        return ("The ChaCha20 stream cipher authenticated with a Poly1305 one-time key per message "
                "(RFC 8439), run in batches on the GPU.")


BY_NAME = {"AES-256-GCM": AES256GCM, "ChaCha20-Poly1305": ChaCha20Poly1305}
