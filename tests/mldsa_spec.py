"""Executable restatement of FIPS 204 (August 2024), "pure" ML-DSA, in plain Python (hashlib + numpy).

Written from the standard's algorithms, by number: KeyGen_internal (6), Sign_internal (7),
Verify_internal (8), the external Sign / Verify (2, 3) with M' = 0x00 || len(ctx) || ctx || M, and the
encodings, samplers and NTTs they use (16-42).  The twiddle table is derived from zeta = 1753 and
8-bit reversal, not stored.  The `_internal` functions keep the ACVP interface (xi; sk, M', rnd;
pk, M', sigma); the parameter set is taken from the key length, or named with `ps=`.

No other ML-DSA implementation was at hand when this was written, so what the tests pin is that
this file and the HIP kernels (csrc/mldsa.hip), written independently from the same standard, agree
byte for byte on mu, w1 and c~'; parity with an outside implementation is unpinned.

`verify_trace` returns what the library's test hook qrk_dbg_mldsa_verify_trace writes: mu, the
recomputed c~', the w1Encode bytes and a flag word (FLAG_HINT: hint encoding malformed, FLAG_NORM:
||z||_inf >= gamma1 - beta, FLAG_HASH: c~ != c~').  A malformed hint leaves w1 undefined, so the
other outputs are zero then; the other two bits are computed independently of each other.
"""
from __future__ import annotations

import hashlib
from typing import NamedTuple, Optional

import numpy as np

Q = 8380417
D = 13
N = 256
ZETA = 1753
FLAG_HINT, FLAG_NORM, FLAG_HASH = 1, 2, 4


class Params(NamedTuple):
    name: str
    k: int
    l: int
    eta: int
    tau: int
    lam: int
    gamma1: int
    gamma2: int
    omega: int

    @property
    def beta(self) -> int:
        return self.tau * self.eta

    @property
    def ctilde(self) -> int:
        return self.lam // 4

    @property
    def zbits(self) -> int:
        return 1 + (self.gamma1 - 1).bit_length()

    @property
    def w1bits(self) -> int:
        return ((Q - 1) // (2 * self.gamma2) - 1).bit_length()

    @property
    def pk(self) -> int:
        return 32 + 320 * self.k

    @property
    def sk(self) -> int:
        ebits = (2 * self.eta).bit_length()
        return 128 + 32 * ((self.k + self.l) * ebits + self.k * D)

    @property
    def sig(self) -> int:
        return self.ctilde + self.l * 32 * self.zbits + self.omega + self.k

    @property
    def w1(self) -> int:
        return self.k * 32 * self.w1bits


PARAMS = {
    "ML-DSA-44": Params("ML-DSA-44", 4, 4, 2, 39, 128, 1 << 17, (Q - 1) // 88, 80),
    "ML-DSA-65": Params("ML-DSA-65", 6, 5, 4, 49, 192, 1 << 19, (Q - 1) // 32, 55),
    "ML-DSA-87": Params("ML-DSA-87", 8, 7, 2, 60, 256, 1 << 19, (Q - 1) // 32, 75),
}


def params(ps=None, pk: Optional[bytes] = None, sk: Optional[bytes] = None) -> Params:
    if isinstance(ps, Params):
        return ps
    if ps is not None:
        return PARAMS[ps]
    for p in PARAMS.values():
        if (pk is not None and len(pk) == p.pk) or (sk is not None and len(sk) == p.sk):
            return p
    raise ValueError("no ML-DSA parameter set has a key of this length")


# ------------------------------------------------------------------ hashing
def H(data: bytes, n: int) -> bytes:
    return hashlib.shake_256(data).digest(n)


class Xof:
    """A SHAKE squeezed a byte range at a time (hashlib recomputes from the start: fine at this size)."""

    def __init__(self, kind: int, seed: bytes):
        self._mk = (hashlib.shake_128 if kind == 128 else hashlib.shake_256)
        self._seed, self._buf, self.pos = seed, b"", 0

    def read(self, n: int) -> bytes:
        if self.pos + n > len(self._buf):
            self._buf = self._mk(self._seed).digest(max(2 * len(self._buf), self.pos + n, 1024))
        out = self._buf[self.pos:self.pos + n]
        self.pos += n
        return out


# ------------------------------------------------------------------ NTT (Algorithms 41-43)
def brv8(i: int) -> int:
    return int(f"{i:08b}"[::-1], 2)


def zetas() -> np.ndarray:
    return np.array([pow(ZETA, brv8(i), Q) for i in range(N)], dtype=np.int64)


ZETAS = zetas()
INV256 = pow(256, -1, Q)  # 8347681


def ntt(w) -> np.ndarray:
    w = np.asarray(w, dtype=np.int64) % Q
    m, ln = 0, 128
    while ln >= 1:
        w = w.reshape(-1, 2, ln)
        nb = w.shape[0]
        z = ZETAS[m + 1:m + 1 + nb].reshape(-1, 1)
        t = z * w[:, 1, :] % Q
        w = np.stack([(w[:, 0, :] + t) % Q, (w[:, 0, :] - t) % Q], axis=1)
        m += nb
        ln //= 2
    return w.reshape(N)


def ntt_inv(w) -> np.ndarray:
    w = np.asarray(w, dtype=np.int64) % Q
    m, ln = 256, 1
    while ln < 256:
        w = w.reshape(-1, 2, ln)
        nb = w.shape[0]
        z = (-ZETAS[m - nb:m][::-1]).reshape(-1, 1)
        a, b = w[:, 0, :], w[:, 1, :]
        w = np.stack([(a + b) % Q, z * (a - b) % Q], axis=1)
        m -= nb
        ln *= 2
    return w.reshape(N) * INV256 % Q


def ntt_slow(w) -> list:
    """Algorithm 41 as written, loop for loop (the check of the vectorised form above)."""
    w = [int(x) % Q for x in w]
    m, ln = 0, 128
    while ln >= 1:
        start = 0
        while start < N:
            m += 1
            z = int(ZETAS[m])
            for j in range(start, start + ln):
                t = z * w[j + ln] % Q
                w[j + ln] = (w[j] - t) % Q
                w[j] = (w[j] + t) % Q
            start += 2 * ln
        ln //= 2
    return w


# ------------------------------------------------------------------ bit packing (Algorithms 16-21)
def _pack(vals, bits: int) -> bytes:
    acc = 0
    for i, v in enumerate(vals):
        acc |= int(v) << (bits * i)
    return acc.to_bytes((bits * len(vals) + 7) // 8, "little")


def _unpack(data: bytes, bits: int, count: int = N) -> np.ndarray:
    acc = int.from_bytes(data, "little")
    mask = (1 << bits) - 1
    return np.array([(acc >> (bits * i)) & mask for i in range(count)], dtype=np.int64)


def simple_bit_pack(w, b: int) -> bytes:
    return _pack(w, b.bit_length())


def simple_bit_unpack(v: bytes, b: int) -> np.ndarray:
    return _unpack(v, b.bit_length())


def bit_pack(w, a: int, b: int) -> bytes:
    return _pack([b - int(x) for x in w], (a + b).bit_length())


def bit_unpack(v: bytes, a: int, b: int) -> np.ndarray:
    return b - _unpack(v, (a + b).bit_length())


def hint_bit_pack(p: Params, h) -> bytes:
    y = bytearray(p.omega + p.k)
    index = 0
    for i in range(p.k):
        for j in range(N):
            if h[i][j]:
                y[index] = j
                index += 1
        y[p.omega + i] = index
    return bytes(y)


def hint_bit_unpack(p: Params, y: bytes):
    """Algorithm 21: the k hint polynomials, or None (the standard's "bottom") for a malformed input."""
    h = np.zeros((p.k, N), dtype=np.int64)
    index = 0
    for i in range(p.k):
        if y[p.omega + i] < index or y[p.omega + i] > p.omega:
            return None
        first = index
        while index < y[p.omega + i]:
            if index > first and y[index - 1] >= y[index]:
                return None
            h[i][y[index]] = 1
            index += 1
    for i in range(index, p.omega):
        if y[i] != 0:
            return None
    return h


# ------------------------------------------------------------------ encodings (Algorithms 22-28)
def pk_encode(p: Params, rho: bytes, t1) -> bytes:
    return rho + b"".join(simple_bit_pack(t1[i], 1023) for i in range(p.k))


def pk_decode(p: Params, pk: bytes):
    return pk[:32], [simple_bit_unpack(pk[32 + 320 * i:32 + 320 * (i + 1)], 1023) for i in range(p.k)]


def sk_encode(p: Params, rho, K, tr, s1, s2, t0) -> bytes:
    out = rho + K + tr
    out += b"".join(bit_pack(s, p.eta, p.eta) for s in s1)
    out += b"".join(bit_pack(s, p.eta, p.eta) for s in s2)
    out += b"".join(bit_pack(t, (1 << (D - 1)) - 1, 1 << (D - 1)) for t in t0)
    return out


def sk_decode(p: Params, sk: bytes):
    rho, K, tr = sk[:32], sk[32:64], sk[64:128]
    eb = 32 * (2 * p.eta).bit_length()
    pos = 128
    s1 = [bit_unpack(sk[pos + eb * i:pos + eb * (i + 1)], p.eta, p.eta) for i in range(p.l)]
    pos += eb * p.l
    s2 = [bit_unpack(sk[pos + eb * i:pos + eb * (i + 1)], p.eta, p.eta) for i in range(p.k)]
    pos += eb * p.k
    t0 = [bit_unpack(sk[pos + 416 * i:pos + 416 * (i + 1)], (1 << (D - 1)) - 1, 1 << (D - 1)) for i in range(p.k)]
    return rho, K, tr, s1, s2, t0


def sig_encode(p: Params, ctilde: bytes, z, h) -> bytes:
    return ctilde + b"".join(bit_pack(zi, p.gamma1 - 1, p.gamma1) for zi in z) + hint_bit_pack(p, h)


def sig_decode(p: Params, sig: bytes):
    zb = 32 * p.zbits
    ctilde = sig[:p.ctilde]
    z = [bit_unpack(sig[p.ctilde + zb * i:p.ctilde + zb * (i + 1)], p.gamma1 - 1, p.gamma1) for i in range(p.l)]
    return ctilde, z, hint_bit_unpack(p, sig[p.ctilde + zb * p.l:])


def w1_encode(p: Params, w1) -> bytes:
    return b"".join(simple_bit_pack(w, (Q - 1) // (2 * p.gamma2) - 1) for w in w1)


# ------------------------------------------------------------------ samplers (Algorithms 29-34)
def sample_in_ball(p: Params, rho: bytes, stream=None) -> np.ndarray:
    """Algorithm 29; `stream` (anything with .read(n)) replaces SHAKE256(rho) in tests of the sampler."""
    c = np.zeros(N, dtype=np.int64)
    x = stream if stream is not None else Xof(256, rho)
    signs = int.from_bytes(x.read(8), "little")
    for i in range(N - p.tau, N):
        j = x.read(1)[0]
        while j > i:
            j = x.read(1)[0]
        c[i] = c[j]
        c[j] = 1 - 2 * ((signs >> (i + p.tau - N)) & 1)
    return c


def coeff_from_three_bytes(b0: int, b1: int, b2: int):
    z = ((b2 & 0x7F) << 16) | (b1 << 8) | b0
    return z if z < Q else None


def rej_ntt_poly_stream(stream) -> np.ndarray:
    """Algorithm 30 on any byte source with .read(n)."""
    a = []
    while len(a) < N:
        v = coeff_from_three_bytes(*stream.read(3))
        if v is not None:
            a.append(v)
    return np.array(a, dtype=np.int64)


def rej_ntt_poly(seed34: bytes) -> np.ndarray:
    return rej_ntt_poly_stream(Xof(128, seed34))


def rej_bounded_poly(p: Params, seed66: bytes) -> np.ndarray:
    x = Xof(256, seed66)
    a = []
    while len(a) < N:
        z = x.read(1)[0]
        for b in (z & 15, z >> 4):
            if p.eta == 2 and b < 15 and len(a) < N:
                a.append(2 - b % 5)
            elif p.eta == 4 and b < 9 and len(a) < N:
                a.append(4 - b)
    return np.array(a, dtype=np.int64)


def expand_a(p: Params, rho: bytes):
    return [[rej_ntt_poly(rho + bytes([s, r])) for s in range(p.l)] for r in range(p.k)]


def expand_s(p: Params, rho66: bytes):
    s1 = [rej_bounded_poly(p, rho66 + r.to_bytes(2, "little")) for r in range(p.l)]
    s2 = [rej_bounded_poly(p, rho66 + (r + p.l).to_bytes(2, "little")) for r in range(p.k)]
    return s1, s2


def expand_mask(p: Params, rho: bytes, mu: int):
    c = p.zbits
    return [bit_unpack(H(rho + (mu + r).to_bytes(2, "little"), 32 * c), p.gamma1 - 1, p.gamma1) for r in range(p.l)]


# ------------------------------------------------------------------ rounding (Algorithms 35-40)
def mod_pm(r, a: int):
    """r mod+- a: the representative in (-a/2, a/2]."""
    r = np.asarray(r, dtype=np.int64) % a
    return np.where(r > a // 2, r - a, r)


def power2round(r):
    rp = np.asarray(r, dtype=np.int64) % Q
    r0 = mod_pm(rp, 1 << D)
    return (rp - r0) >> D, r0


def decompose(p: Params, r):
    rp = np.asarray(r, dtype=np.int64) % Q
    r0 = mod_pm(rp, 2 * p.gamma2)
    wrap = (rp - r0) == Q - 1
    r1 = np.where(wrap, 0, (rp - r0) // (2 * p.gamma2))
    return r1, np.where(wrap, r0 - 1, r0)


def high_bits(p: Params, r):
    return decompose(p, r)[0]


def low_bits(p: Params, r):
    return decompose(p, r)[1]


def make_hint(p: Params, z, r):
    return (high_bits(p, r) != high_bits(p, np.asarray(r) + np.asarray(z))).astype(np.int64)


def use_hint(p: Params, h, r):
    m = (Q - 1) // (2 * p.gamma2)
    r1, r0 = decompose(p, r)
    h = np.asarray(h, dtype=np.int64)
    return np.where(h == 1, np.where(r0 > 0, (r1 + 1) % m, (r1 - 1) % m), r1)


def inf_norm(polys) -> int:
    return max(int(np.max(np.abs(mod_pm(w, Q)))) for w in polys)


# ------------------------------------------------------------------ the scheme (Algorithms 6-8, 1-3)
def keygen_internal(xi: bytes, ps="ML-DSA-65"):
    p = params(ps)
    assert len(xi) == 32
    seed = H(xi + bytes([p.k, p.l]), 128)
    rho, rho66, K = seed[:32], seed[32:96], seed[96:]
    A = expand_a(p, rho)
    s1, s2 = expand_s(p, rho66)
    s1h = [ntt(s) for s in s1]
    t = [(ntt_inv(sum(A[i][j] * s1h[j] for j in range(p.l)) % Q) + s2[i]) % Q for i in range(p.k)]
    t1, t0 = zip(*(power2round(ti) for ti in t))
    pk = pk_encode(p, rho, t1)
    return pk, sk_encode(p, rho, K, H(pk, 64), s1, s2, t0)


def sign_internal(sk: bytes, Mprime: bytes, rnd: bytes, ps=None) -> bytes:
    p = params(ps, sk=sk)
    rho, K, tr, s1, s2, t0 = sk_decode(p, sk)
    s1h, s2h, t0h = ([ntt(s) for s in v] for v in (s1, s2, t0))
    A = expand_a(p, rho)
    mu = H(tr + Mprime, 64)
    rho2 = H(K + rnd + mu, 64)
    kappa = 0
    while True:
        y = expand_mask(p, rho2, kappa)
        kappa += p.l
        yh = [ntt(v) for v in y]
        w = [ntt_inv(sum(A[i][j] * yh[j] for j in range(p.l)) % Q) for i in range(p.k)]
        ctilde = H(mu + w1_encode(p, [high_bits(p, wi) for wi in w]), p.ctilde)
        ch = ntt(sample_in_ball(p, ctilde))
        cs1 = [ntt_inv(ch * s % Q) for s in s1h]
        cs2 = [ntt_inv(ch * s % Q) for s in s2h]
        z = [(y[j] + cs1[j]) % Q for j in range(p.l)]
        r = [(w[i] - cs2[i]) % Q for i in range(p.k)]
        if inf_norm(z) >= p.gamma1 - p.beta or max(int(np.max(np.abs(low_bits(p, ri)))) for ri in r) >= p.gamma2 - p.beta:
            continue
        ct0 = [ntt_inv(ch * t % Q) for t in t0h]
        h = [make_hint(p, -ct0[i], r[i] + ct0[i]) for i in range(p.k)]
        if inf_norm(ct0) >= p.gamma2 or sum(int(hi.sum()) for hi in h) > p.omega:
            continue
        return sig_encode(p, ctilde, [mod_pm(zi, Q) for zi in z], h)


def verify_trace_internal(pk: bytes, Mprime: bytes, sig: bytes, ps=None) -> dict:
    p = params(ps, pk=pk)
    assert len(pk) == p.pk and len(sig) == p.sig
    rho, t1 = pk_decode(p, pk)
    ctilde, z, h = sig_decode(p, sig)
    if h is None:
        return {"mu": bytes(64), "ctilde": bytes(p.ctilde), "w1": bytes(p.w1), "flags": FLAG_HINT}
    A = expand_a(p, rho)
    mu = H(H(pk, 64) + Mprime, 64)
    ch = ntt(sample_in_ball(p, ctilde))
    zh = [ntt(v) for v in z]
    w = [ntt_inv((sum(A[i][j] * zh[j] for j in range(p.l)) - ch * ntt(t1[i] << D)) % Q) for i in range(p.k)]
    w1 = w1_encode(p, [use_hint(p, h[i], w[i]) for i in range(p.k)])
    ctilde2 = H(mu + w1, p.ctilde)
    flags = (FLAG_NORM if inf_norm(z) >= p.gamma1 - p.beta else 0) | (FLAG_HASH if ctilde != ctilde2 else 0)
    return {"mu": mu, "ctilde": ctilde2, "w1": w1, "flags": flags}


def verify_internal(pk: bytes, Mprime: bytes, sig: bytes, ps=None) -> bool:
    p = params(ps, pk=pk)
    if len(pk) != p.pk or len(sig) != p.sig:
        return False
    return verify_trace_internal(pk, Mprime, sig, p)["flags"] == 0


def format_message(M: bytes, ctx: bytes = b"") -> bytes:
    if len(ctx) > 255:
        raise ValueError("ctx is longer than 255 bytes")
    return bytes([0, len(ctx)]) + ctx + M


def sign(sk: bytes, M: bytes, ctx: bytes = b"", rnd: bytes = bytes(32), ps=None) -> bytes:
    """Algorithm 2; rnd = 32 zero bytes is the standard's deterministic variant."""
    return sign_internal(sk, format_message(M, ctx), rnd, ps)


def verify(pk: bytes, M: bytes, sig: bytes, ctx: bytes = b"", ps=None) -> bool:
    if len(ctx) > 255:
        return False
    return verify_internal(pk, format_message(M, ctx), sig, ps)


def verify_trace(pk: bytes, M: bytes, sig: bytes, ctx: bytes = b"", ps=None) -> dict:
    return verify_trace_internal(pk, format_message(M, ctx), sig, ps)
