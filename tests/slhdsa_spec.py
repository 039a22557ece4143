"""SLH-DSA-SHA2 / SPHINCS+-SHA2-simple "f" parameter sets in plain Python (hashlib only): the reference the
GPU verifier (csrc/slhdsa.hip) is tested against.

Written from FIPS 205 (algorithm numbers in the comments).  The ``SLH-DSA-SHA2-*f`` names are pure SLH-DSA
(Algorithm 24 over Algorithm 20); the ``SPHINCS+-SHA2-*f-simple`` names are the round-3.1 submission as
liboqs ships it.  For SHA2 "simple" the two flavours differ in exactly two places, both in this file:

  * ``_frame``         message framing: FIPS 205 Algorithm 24 line 4 hashes M' = 0 || len(ctx) || ctx || M;
                       the submission's ``crypto_sign_verify`` (sign.c) hashes M itself and has no context.
  * ``_fors_indices``  FIPS 205 Algorithm 17 line 1, base_2b(md, a, k) (Algorithm 4: big-endian);
                       the submission's ``message_to_indices`` (fors.c) reads the k a bits least significant
                       bit first within each byte.

Neither liboqs, the submission package nor an OpenSSL with SLH-DSA was at hand when this was written, so
parity with an outside implementation (KAT files) is unpinned; those two functions are the lines to check.

``sign`` is the deterministic variant (opt_rand = PK.seed).  ``Hasher`` keeps one pre-seeded hash object per
key, so one F is one ``copy()`` + ``update()``, and counts SHA-2 compressions (``c256`` / ``c512``, the
PK.seed blocks counted once) for tools/slhdsa_verify_bench.py.
"""
from __future__ import annotations

import hashlib
import hmac
from typing import NamedTuple

FLAG_ROOT = 1  # the reconstructed top root differs from PK.root
FLAG_LONG = 2  # internal: a message of 2^31 bytes or more (never produced here)

WOTS_HASH, WOTS_PK, TREE, FORS_TREE, FORS_ROOTS, WOTS_PRF, FORS_PRF = range(7)


class Params(NamedTuple):
    name: str
    n: int
    h: int
    d: int
    hp: int
    a: int
    k: int
    m: int
    fips: bool

    @property
    def len1(self) -> int:
        return 2 * self.n

    @property
    def len(self) -> int:
        return 2 * self.n + 3

    @property
    def pk(self) -> int:
        return 2 * self.n

    @property
    def sk(self) -> int:
        return 4 * self.n

    @property
    def sig(self) -> int:
        return self.n * (1 + self.k * (self.a + 1) + self.h + self.d * self.len)

    @property
    def md(self) -> int:
        return (self.k * self.a + 7) // 8


_SETS = {"128f": (16, 66, 22, 3, 6, 33, 34), "192f": (24, 66, 22, 3, 8, 33, 42), "256f": (32, 68, 17, 4, 9, 35, 49)}
PARAMS = {}
for _s, _v in _SETS.items():
    PARAMS[f"SPHINCS+-SHA2-{_s}-simple"] = Params(f"SPHINCS+-SHA2-{_s}-simple", *_v, False)
    PARAMS[f"SLH-DSA-SHA2-{_s}"] = Params(f"SLH-DSA-SHA2-{_s}", *_v, True)


def blocks(length: int, big: bool) -> int:
    """Compressions SHA-256 (SHA-512 if big) spends on `length` more bytes, padding included."""
    return (length + 17 + 127) // 128 if big else (length + 9 + 63) // 64


class Hasher:
    """F, H, T_l, PRF, PRF_msg and H_msg of FIPS 205 section 11.2 for one PK.seed."""

    def __init__(self, p: Params, pk_seed: bytes):
        self.p, self.n, self.pk_seed = p, p.n, pk_seed
        self.big = p.n > 16
        self.s256 = hashlib.sha256(pk_seed + bytes(64 - p.n))
        self.s512 = hashlib.sha512(pk_seed + bytes(128 - p.n)) if self.big else None
        self.c256, self.c512 = 1, 1 if self.big else 0

    def F(self, adrs: bytes, m1: bytes) -> bytes:
        h = self.s256.copy()
        h.update(adrs + m1)
        self.c256 += 1
        return h.digest()[:self.n]

    PRF = F  # PRF(PK.seed, SK.seed, ADRS) has F's shape

    def T(self, adrs: bytes, m: bytes) -> bytes:
        """H and T_l: SHA-256 for n = 16, SHA-512 otherwise."""
        if self.big:
            h = self.s512.copy()
            self.c512 += blocks(22 + len(m), True)
        else:
            h = self.s256.copy()
            self.c256 += blocks(22 + len(m), False)
        h.update(adrs + m)
        return h.digest()[:self.n]

    def _hash(self, data: bytes) -> bytes:
        if self.big:
            self.c512 += blocks(len(data), True)
            return hashlib.sha512(data).digest()
        self.c256 += blocks(len(data), False)
        return hashlib.sha256(data).digest()

    def H_msg(self, r: bytes, pk_root: bytes, m: bytes) -> bytes:
        seed = r + self.pk_seed + self._hash(r + self.pk_seed + pk_root + m)
        out, c = b"", 0
        while len(out) < self.p.m:  # MGF1
            out += self._hash(seed + c.to_bytes(4, "big"))
            c += 1
        return out[:self.p.m]

    def PRF_msg(self, sk_prf: bytes, opt_rand: bytes, m: bytes) -> bytes:
        return hmac.new(sk_prf, opt_rand + m, hashlib.sha512 if self.big else hashlib.sha256).digest()[:self.n]


def adrs(layer: int, tree: int, typ: int, w1: int = 0, w2: int = 0, w3: int = 0) -> bytes:
    """The 22-byte compressed address: layer (1) || tree (8) || type (1) || three words."""
    return (bytes([layer]) + tree.to_bytes(8, "big") + bytes([typ]) + w1.to_bytes(4, "big") + w2.to_bytes(4, "big") +
            w3.to_bytes(4, "big"))


# ------------------------------------------------------------------ the two flavour switches
def _frame(p: Params, msg: bytes, ctx: bytes) -> bytes:
    if p.fips:  # FIPS 205 Algorithm 22 / 24: M' = toByte(0, 1) || toByte(|ctx|, 1) || ctx || M
        if len(ctx) > 255:
            raise ValueError("context strings are at most 255 bytes")
        return bytes([0, len(ctx)]) + ctx + msg
    if ctx:  # round 3.1 (sign.c crypto_sign_verify): no context string exists
        raise ValueError("SPHINCS+ round 3.1 has no context string")
    return msg


def _fors_indices(p: Params, md: bytes) -> list:
    if p.fips:  # FIPS 205 Algorithm 17 line 1: base_2b(md, a, k), most significant bit first
        total = int.from_bytes(md, "big") >> (8 * len(md) - p.k * p.a)
        return [(total >> (p.a * (p.k - 1 - i))) & ((1 << p.a) - 1) for i in range(p.k)]
    # round 3.1 fors.c message_to_indices: bit j of index i is bit (i a + j) & 7 of byte (i a + j) >> 3
    total = int.from_bytes(md, "little")
    return [(total >> (p.a * i)) & ((1 << p.a) - 1) for i in range(p.k)]


# ------------------------------------------------------------------ shared by both flavours
def split_digest(p: Params, digest: bytes):
    """md, idx_tree, idx_leaf (FIPS 205 Algorithm 19 / 20 lines 7-12)."""
    md = digest[:p.md]
    idx_tree = int.from_bytes(digest[p.md:p.md + 8], "big") % (1 << (p.h - p.hp))
    idx_leaf = digest[p.md + 8] % (1 << p.hp)
    return md, idx_tree, idx_leaf


def wots_digits(p: Params, m: bytes) -> list:
    """base_w of the message and of the checksum, both big-endian (Algorithm 7 / 8 lines 1-7)."""
    d = []
    for b in m:
        d += [b >> 4, b & 15]
    csum = sum(15 - x for x in d) << 4  # len2 lg_w = 12 bits, left-aligned in two bytes
    return d + [(csum >> 12) & 15, (csum >> 8) & 15, (csum >> 4) & 15]


def _chain(hs: Hasher, x: bytes, start: int, steps: int, prefix: bytes) -> bytes:
    """Algorithm 5; prefix = the compressed address up to and including the chain word."""
    for j in range(start, start + steps):
        x = hs.F(prefix + j.to_bytes(4, "big"), x)
    return x


def wots_pk_from_sig(p, hs, sig: bytes, m: bytes, layer: int, tree: int, leaf: int) -> bytes:
    """Algorithm 8."""
    n = p.n
    out = []
    for i, dg in enumerate(wots_digits(p, m)):
        out.append(_chain(hs, sig[i * n:(i + 1) * n], dg, 15 - dg, adrs(layer, tree, WOTS_HASH, leaf, i)[:18]))
    return hs.T(adrs(layer, tree, WOTS_PK, leaf), b"".join(out))


def _climb(p, hs, node: bytes, auth: bytes, idx: int, height: int, mk) -> bytes:
    """The auth-path loops of Algorithms 11 and 17; mk(height, index) gives the address."""
    n = p.n
    for j in range(height):
        a = auth[j * n:(j + 1) * n]
        pair = node + a if ((idx >> j) & 1) == 0 else a + node
        node = hs.T(mk(j + 1, idx >> (j + 1)), pair)
    return node


def xmss_pk_from_sig(p, hs, leaf: int, sig: bytes, m: bytes, layer: int, tree: int) -> bytes:
    """Algorithm 11."""
    node = wots_pk_from_sig(p, hs, sig[:p.len * p.n], m, layer, tree, leaf)
    return _climb(p, hs, node, sig[p.len * p.n:], leaf, p.hp, lambda z, i: adrs(layer, tree, TREE, 0, z, i))


def fors_pk_from_sig(p, hs, sig: bytes, md: bytes, tree: int, leaf: int) -> bytes:
    """Algorithm 17."""
    n, a = p.n, p.a
    roots = []
    for i, idx in enumerate(_fors_indices(p, md)):
        part = sig[i * (a + 1) * n:(i + 1) * (a + 1) * n]
        node = hs.F(adrs(0, tree, FORS_TREE, leaf, 0, (i << a) + idx), part[:n])
        roots.append(_climb(p, hs, node, part[n:], idx, a,
                            lambda z, j, i=i: adrs(0, tree, FORS_TREE, leaf, z, (i << (a - z)) + j)))
    return hs.T(adrs(0, tree, FORS_ROOTS, leaf), b"".join(roots))


def verify_trace(name: str, pk: bytes, msg: bytes, sig: bytes, ctx: bytes = b"", hasher=None) -> dict:
    """Algorithm 20 (slh_verify_internal) over the framed message: digest (m bytes), fors_pk (n),
    roots (d n bytes: the root every hypertree layer reconstructed, Algorithm 13) and the flag word."""
    p = PARAMS[name]
    n = p.n
    if len(pk) != p.pk or len(sig) != p.sig:
        raise ValueError("wrong public key or signature length")
    pk_seed, pk_root = pk[:n], pk[n:]
    hs = hasher or Hasher(p, pk_seed)
    digest = hs.H_msg(sig[:n], pk_root, _frame(p, msg, ctx))
    md, tree, leaf = split_digest(p, digest)
    fors_len = p.k * (p.a + 1) * n
    node = fors_pk = fors_pk_from_sig(p, hs, sig[n:n + fors_len], md, tree, leaf)
    roots = []
    xl = (p.hp + p.len) * n
    for j in range(p.d):
        node = xmss_pk_from_sig(p, hs, leaf, sig[n + fors_len + j * xl:n + fors_len + (j + 1) * xl], node, j, tree)
        roots.append(node)
        leaf, tree = tree % (1 << p.hp), tree >> p.hp
    return {"digest": digest, "fors_pk": fors_pk, "roots": b"".join(roots), "flags": 0 if node == pk_root else FLAG_ROOT}


def verify(name: str, pk: bytes, msg: bytes, sig: bytes, ctx: bytes = b"") -> bool:
    p = PARAMS[name]
    if len(pk) != p.pk or len(sig) != p.sig or len(ctx) > 255 or (ctx and not p.fips):
        return False
    return verify_trace(name, pk, msg, sig, ctx)["flags"] == 0


# ------------------------------------------------------------------ key generation and signing (tests only)
def _tree(hs, leaves: list, mk) -> list:
    """All levels of a Merkle tree over `leaves`: levels[z][i]; mk(height, index) gives the address."""
    levels = [leaves]
    z = 0
    while len(levels[-1]) > 1:
        z += 1
        cur = levels[-1]
        levels.append([hs.T(mk(z, i), cur[2 * i] + cur[2 * i + 1]) for i in range(len(cur) // 2)])
    return levels


def _auth(levels: list, idx: int) -> bytes:
    return b"".join(levels[j][(idx >> j) ^ 1] for j in range(len(levels) - 1))


def _wots_sk(p, hs, sk_seed: bytes, layer: int, tree: int, leaf: int, i: int) -> bytes:
    return hs.PRF(adrs(layer, tree, WOTS_PRF, leaf, i), sk_seed)


def _xmss_levels(p, hs, sk_seed: bytes, layer: int, tree: int) -> list:
    """Algorithm 9 for every node of one XMSS tree (leaves: Algorithm 6)."""
    leaves = []
    for leaf in range(1 << p.hp):
        ends = [_chain(hs, _wots_sk(p, hs, sk_seed, layer, tree, leaf, i), 0, 15,
                       adrs(layer, tree, WOTS_HASH, leaf, i)[:18]) for i in range(p.len)]
        leaves.append(hs.T(adrs(layer, tree, WOTS_PK, leaf), b"".join(ends)))
    return _tree(hs, leaves, lambda z, i: adrs(layer, tree, TREE, 0, z, i))


def keygen(name: str, sk_seed: bytes, sk_prf: bytes, pk_seed: bytes):
    """Algorithm 18 (slh_keygen_internal): (pk, sk)."""
    p = PARAMS[name]
    assert len(sk_seed) == len(sk_prf) == len(pk_seed) == p.n
    hs = Hasher(p, pk_seed)
    root = _xmss_levels(p, hs, sk_seed, p.d - 1, 0)[-1][0]
    return pk_seed + root, sk_seed + sk_prf + pk_seed + root


def sign(name: str, sk: bytes, msg: bytes, ctx: bytes = b"") -> bytes:
    """Algorithm 19 (slh_sign_internal) with opt_rand = PK.seed, over the framed message."""
    p = PARAMS[name]
    n, a = p.n, p.a
    sk_seed, sk_prf, pk_seed, pk_root = (sk[i * n:(i + 1) * n] for i in range(4))
    hs = Hasher(p, pk_seed)
    m = _frame(p, msg, ctx)
    r = hs.PRF_msg(sk_prf, pk_seed, m)
    md, tree, leaf = split_digest(p, hs.H_msg(r, pk_root, m))
    out = [r]
    roots = []
    for i, idx in enumerate(_fors_indices(p, md)):  # Algorithm 16
        sks = [hs.PRF(adrs(0, tree, FORS_PRF, leaf, 0, (i << a) + j), sk_seed) for j in range(1 << a)]
        leaves = [hs.F(adrs(0, tree, FORS_TREE, leaf, 0, (i << a) + j), s) for j, s in enumerate(sks)]
        levels = _tree(hs, leaves, lambda z, j, i=i: adrs(0, tree, FORS_TREE, leaf, z, (i << (a - z)) + j))
        out += [sks[idx], _auth(levels, idx)]
        roots.append(levels[-1][0])
    node = hs.T(adrs(0, tree, FORS_ROOTS, leaf), b"".join(roots))
    for layer in range(p.d):  # Algorithm 12 over Algorithm 10
        levels = _xmss_levels(p, hs, sk_seed, layer, tree)
        for i, dg in enumerate(wots_digits(p, node)):
            out.append(_chain(hs, _wots_sk(p, hs, sk_seed, layer, tree, leaf, i), 0, dg,
                              adrs(layer, tree, WOTS_HASH, leaf, i)[:18]))
        out.append(_auth(levels, leaf))
        node = levels[-1][0]
        leaf, tree = tree % (1 << p.hp), tree >> p.hp
    sig = b"".join(out)
    assert len(sig) == p.sig and node == pk_root
    return sig
