"""Batched KEM engine: N independent handshakes per call on one MI355X.

The reference performs one ``OQS_KEM_*`` call per handshake on the asyncio
thread (``quantum_resistant_p2p/crypto/key_exchange.py:133,155-156,178-179``).
:class:`BatchKEM` runs N of them per call through ``qrk_kem_*_batch`` in
libqrkem.so.  Device tensors (``torch.uint8`` on ``cuda``) are passed by pointer
and processed on the caller's current stream (zero copy); host arrays go through
the synchronous ``*_batch_host`` entry points.

Tensors are contiguous ``[n, len]`` uint8 -- the AoS layout the C ABI documents.
"""
from __future__ import annotations

import ctypes as ct
from typing import Optional

import numpy as np

from ._native import LIB, last_error
from .oqs import MechanismNotEnabledError, MechanismNotSupportedError, get_enabled_kem_mechanisms, \
    get_supported_kem_mechanisms, kem_sizes

try:  # torch is plumbing for device memory/streams, not a compute path
    import torch
except ImportError:  # pragma: no cover
    torch = None


def _is_dev(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _dptr(t) -> ct.c_void_p:
    assert t.dtype == torch.uint8 or t.dtype == torch.int32, t.dtype
    assert t.is_contiguous()
    return ct.c_void_p(t.data_ptr())


def _kptr(t) -> Optional[ct.c_void_p]:
    """A key_index device tensor (any 32-bit dtype), or None."""
    return None if t is None else ct.c_void_p(t.data_ptr())


def _check_dev(t, width: int, what: str, n: Optional[int] = None):
    """Device [n, width] uint8 contiguous, like _as_host's check for host arrays: the kernels
    index rows at the fixed stride `width`, so a wrong shape must fail here, not read past
    the tensor (the reference raises ValueError on a wrong-length input, oqs.py:341-347)."""
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{what}: expected a [n, {width}] uint8 tensor, got {tuple(t.shape)} {t.dtype}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{what}: batch size {t.shape[0]} != {n}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: tensor must be contiguous")
    return t


def _hptr(a: np.ndarray) -> ct.c_void_p:
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ct.c_void_p)


def _as_host(x, width: int) -> np.ndarray:
    if isinstance(x, (bytes, bytearray)):
        x = np.frombuffer(bytes(x), np.uint8).reshape(1, -1)
    elif isinstance(x, (list, tuple)):
        x = np.stack([np.frombuffer(bytes(b), np.uint8) for b in x]) if x else np.zeros((0, width), np.uint8)
    a = np.ascontiguousarray(np.asarray(x, dtype=np.uint8))
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"expected a [n, {width}] uint8 array, got shape {a.shape}")
    return a


class _KeySet:
    """What the key-set classes share: the handle of a set loaded on the device, its description, and its release."""
    _INFO = _FREE = ""  # the library's info / free call of the family

    def __init__(self, handle, alg: str, g: int, secret: bool, device: int = 0):
        self._handle = handle
        self.alg = alg
        self.g = int(g)
        self.secret = bool(secret)
        self.device = device

    @property
    def closed(self) -> bool:
        return not self._handle

    @property
    def device_bytes(self) -> int:
        """Bytes of device memory the set holds (the library's ``*_keyset_info``); 0 once closed."""
        if self.closed:
            return 0
        out = (ct.c_size_t * 4)()
        if getattr(LIB, self._INFO)(self._handle, out) != 0:
            raise RuntimeError(last_error())
        return int(out[3])

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            getattr(LIB, self._FREE)(h)

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
        return f"<{type(self).__name__} {self.alg} {kind} g={self.g}{' closed' if self.closed else ''}>"


class MLKEMKeySet(_KeySet):
    """g ML-KEM keys expanded once on the device (``qrk_mlkem_pubkeys_load`` / ``qrk_mlkem_seckeys_load``,
    mlkem_keyed.hip): what :meth:`BatchKEM.encaps_keyed` and :meth:`BatchKEM.decaps_keyed` index into.  Made by
    :meth:`BatchKEM.load_public_keys` / :meth:`BatchKEM.load_secret_keys`; owns the handle and is a context
    manager.  A secret set holds the dk bytes in device memory until :meth:`close`, which zeroes them (the
    library synchronises the device first)."""
    _INFO, _FREE = "qrk_mlkem_keyset_info", "qrk_mlkem_keyset_free"


class FrodoKeySet(_KeySet):
    """g FrodoKEM keys expanded once on the device (``qrk_frodo_pubkeys_load`` / ``qrk_frodo_seckeys_load``,
    frodo_keyed.hip): A as int8 limb planes, B unpacked and pkh per key, and S^T and s in a secret set.  Made by
    :meth:`FrodoBatchKEM.load_public_keys` / :meth:`FrodoBatchKEM.load_secret_keys`; owns the handle and is a
    context manager.  A secret set holds S^T and s in device memory until :meth:`close`, which zeroes them."""
    _INFO, _FREE = "qrk_frodo_keyset_info", "qrk_frodo_keyset_free"


class BatchKEM:
    """Batched KeyGen / Encaps / Decaps for one algorithm on one device."""

    def __init__(self, alg: str, device: int = 0, chunk: Optional[int] = None):
        if alg not in get_enabled_kem_mechanisms():
            if alg in get_supported_kem_mechanisms():
                raise MechanismNotEnabledError(alg)
            raise MechanismNotSupportedError(alg)
        self.alg = alg
        self._name = alg.encode()
        self.device = device
        s = kem_sizes(alg)
        self.pk_len = s["length_public_key"]
        self.sk_len = s["length_secret_key"]
        self.ct_len = s["length_ciphertext"]
        self.ss_len = s["length_shared_secret"]
        self.kp_coins = s["length_keypair_coins"]
        self.enc_coins = s["length_encaps_coins"]
        h = ct.c_void_p()
        if LIB.qrk_ctx_create(ct.byref(h), device) != 0:
            raise RuntimeError(f"qrkem: cannot create a context on device {device}: {last_error()}")
        self._ctx = h
        if chunk:
            LIB.qrk_ctx_set_chunk(self._ctx, chunk)

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

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise RuntimeError(f"qrkem {what} failed ({self.alg}): {last_error()}")

    def _empty(self, n: int, width: int):
        return torch.empty((n, width), dtype=torch.uint8, device=f"cuda:{self.device}")

    # ------------------------------------------------------------------ KeyGen
    def keypair(self, n: Optional[int] = None, coins=None):
        """Returns (pk [n, pk_len], sk [n, sk_len]).  ``coins`` [n, kp_coins] or None (OS CSPRNG).

        Device coins (or ``n`` without coins) -> device outputs; host coins -> numpy outputs."""
        if coins is None and n is None:
            raise ValueError("give n or coins")
        if coins is not None and not _is_dev(coins):
            c = _as_host(coins, self.kp_coins)
            n = c.shape[0]
            pk = np.zeros((n, self.pk_len), np.uint8)
            sk = np.zeros((n, self.sk_len), np.uint8)
            self._check(LIB.qrk_kem_keypair_batch_host(self._ctx, self._name, n, _hptr(pk), _hptr(sk), _hptr(c)),
                        "keypair")
            return pk, sk
        if coins is not None:
            n = _check_dev(coins, self.kp_coins, "keypair coins").shape[0]
        pk, sk = self._empty(n, self.pk_len), self._empty(n, self.sk_len)
        cp = _dptr(coins) if coins is not None else None
        self._check(LIB.qrk_kem_keypair_batch(self._ctx, self._name, n, _dptr(pk), _dptr(sk), cp, self._stream()),
                    "keypair")
        return pk, sk

    # ------------------------------------------------------------------ Encaps
    def encaps(self, pk, coins=None, return_status: bool = False):
        """Returns (ct, ss) (+ status int32[n]: -1 where pk fails the FIPS 203 7.2 check)."""
        if _is_dev(pk):
            n = _check_dev(pk, self.pk_len, "encaps pk").shape[0]
            c, ss = self._empty(n, self.ct_len), self._empty(n, self.ss_len)
            st = torch.empty((n,), dtype=torch.int32, device=pk.device) if return_status else None
            if coins is not None and not _is_dev(coins):
                coins = torch.from_numpy(_as_host(coins, self.enc_coins)).to(pk.device)
            if coins is not None:
                _check_dev(coins, self.enc_coins, "encaps coins", n)
            self._check(LIB.qrk_kem_encaps_batch(self._ctx, self._name, n, _dptr(c), _dptr(ss), _dptr(pk),
                                                 _dptr(coins) if coins is not None else None,
                                                 _dptr(st) if st is not None else None, self._stream()), "encaps")
            return (c, ss, st) if return_status else (c, ss)
        p = _as_host(pk, self.pk_len)
        n = p.shape[0]
        c = np.zeros((n, self.ct_len), np.uint8)
        ss = np.zeros((n, self.ss_len), np.uint8)
        st = np.zeros((n,), np.int32)
        cc = _as_host(coins, self.enc_coins) if coins is not None else None
        self._check(LIB.qrk_kem_encaps_batch_host(self._ctx, self._name, n, _hptr(c), _hptr(ss), _hptr(p),
                                                  _hptr(cc) if cc is not None else None, _hptr(st)), "encaps")
        return (c, ss, st) if return_status else (c, ss)

    # ------------------------------------------------------------------ Decaps
    def decaps(self, sk, ct_, return_status: bool = False):
        """Returns ss [n, ss_len] (+ status int32[n] with return_status).  ML-KEM / FrodoKEM:
        implicit rejection, status 0.  HQC: status -1 where the re-encryption check fails (the
        OQS_ERROR liboqs returns there); ss = K(sigma || ct) is written either way."""
        if _is_dev(sk) and _is_dev(ct_):
            n = _check_dev(sk, self.sk_len, "decaps sk").shape[0]
            _check_dev(ct_, self.ct_len, "decaps ct", n)
            ss = self._empty(n, self.ss_len)
            if return_status:
                st = torch.empty((n,), dtype=torch.int32, device=sk.device)
                self._check(LIB.qrk_kem_decaps_batch_status(self._ctx, self._name, n, _dptr(ss), _dptr(ct_),
                                                            _dptr(sk), _dptr(st), self._stream()), "decaps")
                return ss, st
            self._check(LIB.qrk_kem_decaps_batch(self._ctx, self._name, n, _dptr(ss), _dptr(ct_), _dptr(sk),
                                                 self._stream()), "decaps")
            return ss
        s = _as_host(sk, self.sk_len)
        c = _as_host(ct_, self.ct_len)
        if s.shape[0] != c.shape[0]:
            raise ValueError("sk and ct batch sizes differ")
        ss = np.zeros((s.shape[0], self.ss_len), np.uint8)
        st = np.zeros((s.shape[0],), np.int32)
        self._check(LIB.qrk_kem_decaps_batch_status_host(self._ctx, self._name, s.shape[0], _hptr(ss), _hptr(c),
                                                         _hptr(s), _hptr(st)), "decaps")
        return (ss, st) if return_status else ss

    # ------------------------------------------------------------------ key sets (ML-KEM)
    _KEYSET = MLKEMKeySet    # what the keyed methods take and the loaders make ...
    _KEYED_PREFIX = "qrk_mlkem_"  # ... and the family of library calls behind them

    def _keyed_call(self, name: str):
        """The library's `name` call of this class's key sets: pubkeys_load, seckeys_load, encaps_keyed_batch,
        decaps_keyed_batch."""
        return getattr(LIB, self._KEYED_PREFIX + name)

    def _keyed_only(self) -> None:
        if not self.alg.startswith("ML-KEM-"):
            raise ValueError(f"key sets are ML-KEM only: {self.alg} has none (use encaps / decaps)")

    def _load_keys(self, keys, width: int, secret: bool):
        self._keyed_only()
        what = "secret" if secret else "public"
        if not _is_dev(keys):
            keys = torch.from_numpy(_as_host(keys, width)).to(f"cuda:{self.device}")
        _check_dev(keys, width, f"{what} keys")
        g = keys.shape[0]
        if g == 0:
            raise ValueError(f"a key set holds at least one {what} key")
        h = ct.c_void_p()
        load = self._keyed_call("seckeys_load" if secret else "pubkeys_load")
        self._check(load(self._ctx, self._name, g, _dptr(keys), ct.byref(h), self._stream()), "key set load")
        torch.cuda.current_stream(self.device).synchronize()  # the set is ready on every stream; `keys` may go
        return self._KEYSET(h, self.alg, g, secret, self.device)

    def load_public_keys(self, pk) -> MLKEMKeySet:
        """A key set of the g encapsulation keys pk [g, pk_len] (a device tensor, numpy array or list of bytes):
        SampleNTT for A_hat, H(ek) and the FIPS 203 modulus check run once per key here and never again per row."""
        return self._load_keys(pk, self.pk_len, False)

    def load_secret_keys(self, sk) -> MLKEMKeySet:
        """A key set of the g decapsulation keys sk [g, sk_len]: SampleNTT for A_hat runs once per key here."""
        return self._load_keys(sk, self.sk_len, True)

    def _keyed_args(self, keyset, secret: bool, key_index, n: int):
        if not isinstance(keyset, self._KEYSET):
            article = "an" if self._KEYSET is MLKEMKeySet else "a"
            raise ValueError(f"keyset must be {article} {self._KEYSET.__name__}")
        if keyset.alg != self.alg:
            raise ValueError(f"the key set holds {keyset.alg} keys, this object is {self.alg}")
        if keyset.secret and not secret:
            raise ValueError("a secret key set cannot encapsulate: load the public keys with load_public_keys")
        if secret and not keyset.secret:
            raise ValueError("a public key set cannot decapsulate: load the secret keys with load_secret_keys")
        if keyset.device != self.device:
            raise ValueError(f"the key set is on device {keyset.device}, this object on device {self.device}")
        if key_index is None and keyset.g != 1:
            raise ValueError(f"key_index may be None only for a key set of one key, this one has {keyset.g}")
        if keyset.closed:
            raise ValueError("the key set is closed")
        if key_index is None:
            return None
        if not _is_dev(key_index):
            idx = np.asarray(key_index)
            if idx.ndim != 1 or idx.dtype.kind not in "iu" or (idx.size and (idx.min() < 0 or idx.max() >= 2 ** 32)):
                raise ValueError("key_index must be a 1-D sequence of n indices in [0, 2^32)")
            key_index = torch.from_numpy(idx.astype(np.uint32).view(np.int32)).to(f"cuda:{self.device}")
        if key_index.dtype == torch.int64:
            key_index = key_index.to(torch.int32)  # an index of 2^31 or more is outside every set either way
        if not (key_index.dim() == 1 and key_index.numel() == n and key_index.is_contiguous() and
                key_index.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
            raise ValueError("key_index must be a contiguous 1-D 32-bit device tensor of n entries")
        return key_index

    def encaps_keyed(self, keyset, key_index=None, n: Optional[int] = None, coins=None, return_status: bool = False):
        """Encaps of n rows under a public key set: row i uses key ``key_index[i]`` (None: key 0 of a set of one).
        n comes from key_index, coins or ``n``.  Returns device (ct, ss) (+ status int32[n]: -1 where the key
        fails the FIPS 203 7.2 check or the index is outside the set -- that row's ct and ss are zero): byte for
        byte what :meth:`encaps` returns for the same keys and coins."""
        self._keyed_only()
        if key_index is not None:
            n = len(key_index) if not _is_dev(key_index) else key_index.numel()
        elif coins is not None:
            n = len(coins) if not _is_dev(coins) else coins.shape[0]
        if n is None:
            raise ValueError("give key_index, coins or n")
        key_index = self._keyed_args(keyset, False, key_index, n)
        dev = f"cuda:{self.device}"
        if coins is not None and not _is_dev(coins):
            coins = torch.from_numpy(_as_host(coins, self.enc_coins)).to(dev)
        if coins is not None:
            _check_dev(coins, self.enc_coins, "encaps coins", n)
        c, ss = self._empty(n, self.ct_len), self._empty(n, self.ss_len)
        st = torch.empty((n,), dtype=torch.int32, device=dev) if return_status else None
        encaps = self._keyed_call("encaps_keyed_batch")
        self._check(encaps(self._ctx, keyset._handle, n, _kptr(key_index), _dptr(c), _dptr(ss),
                           _dptr(coins) if coins is not None else None, _dptr(st) if st is not None else None,
                           self._stream()), "encaps_keyed")
        return (c, ss, st) if return_status else (c, ss)

    def decaps_keyed(self, keyset, ct_, key_index=None, return_status: bool = False):
        """Decaps of the rows ct [n, ct_len] under a secret key set: row i uses key ``key_index[i]``.  Returns
        device ss [n, ss_len] (+ status int32[n]: 0, or -1 with a zero ss row where the index is outside the set;
        an invalid ciphertext is rejected implicitly, status 0): byte for byte what :meth:`decaps` returns."""
        self._keyed_only()
        if not _is_dev(ct_):
            ct_ = torch.from_numpy(_as_host(ct_, self.ct_len)).to(f"cuda:{self.device}")
        n = _check_dev(ct_, self.ct_len, "decaps ct").shape[0]
        key_index = self._keyed_args(keyset, True, key_index, n)
        ss = self._empty(n, self.ss_len)
        st = torch.empty((n,), dtype=torch.int32, device=ct_.device) if return_status else None
        decaps = self._keyed_call("decaps_keyed_batch")
        self._check(decaps(self._ctx, keyset._handle, n, _kptr(key_index), _dptr(ss), _dptr(ct_),
                           _dptr(st) if st is not None else None, self._stream()), "decaps_keyed")
        return (ss, st) if return_status else ss

    @property
    def effective_chunk(self) -> int:
        """Handshakes per internal chunk for this algorithm (FrodoKEM caps it by scratch size)."""
        return int(LIB.qrk_ctx_effective_chunk(self._ctx, self.alg.encode()))

    @property
    def scratch_bytes(self) -> int:
        """Device scratch the context holds (grown on demand, never shrunk)."""
        return int(LIB.qrk_ctx_scratch_bytes(self._ctx))

    def set_streams(self, streams: int) -> None:
        """0 (default): independent kernels of one operation share multi-role launches; 1: serial,
        one kernel per launch (per-kernel timings in isolation).  Every kernel runs on the caller's
        stream in both schedules."""
        self._check(LIB.qrk_ctx_set_streams(self._ctx, streams), "set_streams")

    # ------------------------------------------------------------------ kernel timing
    def profile(self, enable: bool = True) -> None:
        """Reset and enable/disable per-kernel HIP-event timing on the launch stream."""
        self._check(LIB.qrk_ctx_profile(self._ctx, int(enable)), "profile")

    def profile_read(self) -> dict:
        """{kernel name: (total ms, launches)} accumulated since profile(True)."""
        n = LIB.qrk_ctx_profile_collect(self._ctx)
        if n < 0:
            raise RuntimeError(f"qrkem profile collect failed: {last_error()}")
        out = {}
        for i in range(n):
            name, ms, cnt = ct.c_char_p(), ct.c_double(), ct.c_uint64()
            self._check(LIB.qrk_ctx_profile_get(self._ctx, i, ct.byref(name), ct.byref(ms), ct.byref(cnt)),
                        "profile_get")
            out[name.value.decode()] = (ms.value, cnt.value)
        return out

    # ------------------------------------------------------------------ bench helpers
    def bench_coins(self, n: int, length: int, seed: int, first: int = 0):
        out = self._empty(n, length)
        self._check(LIB.qrk_bench_coins(self._ctx, n, length, seed, first, _dptr(out), self._stream()),
                    "bench_coins")
        return out

    def digest_rows(self, a, b=None):
        """Per-record SHA3-256(a_i || b_i) of device tensors [n, la] / [n, lb] -> [n, 32] uint8
        (qrk_digest_rows): the records the sharded bench combines into shard digests."""
        n = a.shape[0]
        _check_dev(a, a.shape[1], "digest a")
        if b is not None:
            _check_dev(b, b.shape[1], "digest b", n)
        out = self._empty(n, 32)
        self._check(LIB.qrk_digest_rows(self._ctx, n, _dptr(a), a.shape[1], _dptr(b) if b is not None else None,
                                        b.shape[1] if b is not None else 0, _dptr(out), self._stream()),
                    "digest_rows")
        return out

    def cleanse(self) -> None:
        """Zero every context buffer that can hold keys or secret intermediates (qrk_ctx_cleanse)."""
        self._check(LIB.qrk_ctx_cleanse(self._ctx), "cleanse")

    def tamper(self, ct_, seed: int, mode: int) -> None:
        """In-place: mode 0 none, 1 every ciphertext, 2 Bernoulli(1/2) per index."""
        _check_dev(ct_, self.ct_len, "tamper ct")
        self._check(LIB.qrk_tamper(self._ctx, ct_.shape[0], self.ct_len, seed, mode, _dptr(ct_), self._stream()),
                    "tamper")

    def hqc_supports(self, r, kind: int):
        """HQC fixed-weight supports from device uint32 random words r [n][weight] (kind 0: w,
        1: w_r = w_e), duplicates removed as the spec does (test hook, qrk_hqc_supports)."""
        out = torch.empty_like(r)
        self._check(LIB.qrk_hqc_supports(self._ctx, self.alg.encode(), kind, r.shape[0], _dptr(r), _dptr(out),
                                          self._stream()), "hqc_supports")
        return out

    def hqc_code_decode(self, sk, ct_):
        """HQC decoder stages of Decaps alone on device sk [n, sk_len] / ct [n, ct_len]: returns
        (syms [n, n1], the Reed-Muller symbols decoded from v - u y; mprime [n, k], the message the
        Reed-Solomon decoder returns for them) (test hook, qrk_hqc_code_decode)."""
        if not self.alg.startswith("HQC-"):
            raise ValueError(f"not an HQC parameter set: {self.alg}")
        n = _check_dev(sk, self.sk_len, "code_decode sk").shape[0]
        _check_dev(ct_, self.ct_len, "code_decode ct", n)
        k = self.enc_coins - 16
        n1 = {16: 46, 24: 56, 32: 90}[k]
        syms, mp = self._empty(n, n1), self._empty(n, k)
        self._check(LIB.qrk_hqc_code_decode(self._ctx, self._name, n, _dptr(sk), _dptr(ct_), _dptr(syms), _dptr(mp),
                                            self._stream()), "hqc_code_decode")
        return syms, mp

    def hqc_decaps_trace(self, sk, ct_):
        """hqc_code_decode plus the word the decoder is given: returns (t [n, n1 n2 / 8], the bits of
        v - u y as k_hqc_decode hands them to the Reed-Muller stage; syms; mprime) (test hook,
        qrk_dbg_hqc_decaps_trace).  Outputs are pre-filled with 0xA5 so a missing store shows."""
        if not self.alg.startswith("HQC-"):
            raise ValueError(f"not an HQC parameter set: {self.alg}")
        n = _check_dev(sk, self.sk_len, "decaps_trace sk").shape[0]
        _check_dev(ct_, self.ct_len, "decaps_trace ct", n)
        k = self.enc_coins - 16
        n1 = {16: 46, 24: 56, 32: 90}[k]
        vb = self.ct_len - 16 - (self.pk_len - 40)
        t, syms, mp = (self._empty(n, w).fill_(0xA5) for w in (vb, n1, k))
        from ._debug import bind  # hooks are bound there, on first use: the product path never needs them
        self._check(bind().qrk_dbg_hqc_decaps_trace(self._ctx, self._name, n, _dptr(sk), _dptr(ct_), _dptr(t),
                                                    _dptr(syms), _dptr(mp), self._stream()), "hqc_decaps_trace")
        return t, syms, mp


class FrodoBatchKEM(BatchKEM):
    """:class:`BatchKEM` for a FrodoKEM name, with key sets: the four keyed methods of :class:`BatchKEM` (same
    parameter lists, same wrapper checks, same host and device inputs) over ``qrk_frodo_*`` and
    :class:`FrodoKeySet`.  Gen(A), the unpacking of B and H(pk) run once per key at load; a keyed call computes S'A
    of all rows that share a key as one integer matrix product against the stored A.  Results are byte for byte
    those of :meth:`encaps` / :meth:`decaps` for the same keys and mu.  :class:`BatchKEM` itself has key sets for
    ML-KEM only."""
    _KEYSET = FrodoKeySet
    _KEYED_PREFIX = "qrk_frodo_"

    def __init__(self, alg: str, device: int = 0, chunk: Optional[int] = None):
        if not str(alg).startswith("FrodoKEM-"):
            raise ValueError(f"FrodoBatchKEM is for FrodoKEM names: {alg} is none (use BatchKEM)")
        super().__init__(alg, device, chunk)

    def _keyed_only(self) -> None:
        if not self.alg.startswith("FrodoKEM-"):
            raise ValueError(f"FrodoBatchKEM is for FrodoKEM names: {self.alg} is none (use BatchKEM)")

    def load_public_keys(self, pk) -> FrodoKeySet:
        """A key set of the g public keys pk [g, pk_len] (a device tensor, numpy array or list of bytes): Gen(A),
        the unpacking of B and pkh = H(pk) run once per key here and never again per row."""
        return self._load_keys(pk, self.pk_len, False)

    def load_secret_keys(self, sk) -> FrodoKeySet:
        """A key set of the g secret keys sk [g, sk_len]: Gen(A) runs once per key here; S^T, s and pkh are copied."""
        return self._load_keys(sk, self.sk_len, True)

    def encaps_keyed(self, keyset, key_index=None, n: Optional[int] = None, coins=None, return_status: bool = False):
        """Encaps of n rows under a public key set: row i uses key ``key_index[i]`` (None: key 0 of a set of one);
        ``coins`` is mu [n, enc_coins] or None (OS CSPRNG).  Returns device (ct, ss) (+ status int32[n]: -1 and a
        zero ct / ss row where the index is outside the set): byte for byte what :meth:`encaps` returns."""
        return super().encaps_keyed(keyset, key_index, n, coins, return_status)

    def decaps_keyed(self, keyset, ct_, key_index=None, return_status: bool = False):
        """Decaps of the rows ct [n, ct_len] under a secret key set.  Returns device ss [n, ss_len] (+ status
        int32[n]: 0, or -1 with a zero ss row where the index is outside the set; an invalid ciphertext is rejected
        implicitly with the key's s, status 0): byte for byte what :meth:`decaps` returns."""
        return super().decaps_keyed(keyset, ct_, key_index, return_status)
