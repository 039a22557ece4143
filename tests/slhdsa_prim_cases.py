"""Constructed inputs for the SLH-DSA device primitives (csrc/slhdsa_common.cuh, csrc/sha2.cuh) -- TEST
INFRASTRUCTURE.

Shared by tests/test_slhdsa_prim_cases.py (CPU: the inputs are what they claim to be, from the spec alone) and
tests/test_gpu_slhdsa_prims.py (the probe tests/slhdsa_probe.hip).  Everything is built deterministically from
labels; nothing is stored.  Expected values come from tests/slhdsa_spec.py, hashlib or plain Python integers;
the one piece of arithmetic kept here is a plain-Python SHA-2 compression function for tails that start from
an arbitrary state, which hashlib cannot express (the CPU test checks it against hashlib first).
"""
from __future__ import annotations

import hashlib
import math
from typing import NamedTuple

import slhdsa_spec as spec

NAMES = sorted(spec.PARAMS)
SIZES = (16, 24, 32)
SET_OF = {16: "128f", 24: "192f", 32: "256f"}


def ps_of(name: str) -> int:
    """The probe's parameter-set number: 2 set + flavour (csrc/slhdsa_common.cuh make())."""
    p = spec.PARAMS[name]
    return 2 * SIZES.index(p.n) + (1 if p.fips else 0)


def params_of(n: int) -> spec.Params:
    return spec.PARAMS[f"SLH-DSA-SHA2-{SET_OF[n]}"]


def rand(label: str, size: int) -> bytes:
    return hashlib.shake_256(b"slhdsa-prim-cases/" + label.encode()).digest(size)


# ------------------------------------------------------------------ WOTS+ nodes
def _node(digits) -> bytes:
    assert len(digits) % 2 == 0 and all(0 <= d < 16 for d in digits)
    return bytes((digits[2 * i] << 4) | digits[2 * i + 1] for i in range(len(digits) // 2))


def _with_csum(n: int, target: int) -> bytes:
    """A node whose checksum sum(15 - digit) is exactly `target`, spent from the first digit on."""
    assert 0 <= target <= 30 * n
    digits = []
    for _ in range(2 * n):
        v = min(15, target)
        digits.append(15 - v)
        target -= v
    return _node(digits)


CSUM_TARGETS = (15, 16, 255, 256, 511, 512)


def wots_nodes(n: int) -> list:
    """(label, node) pairs.  Beyond the listed groups: sixteen rotations, so that every digit value stands at
    every position by construction, and a ladder of checksums 17 j, so that the two low checksum digits take
    every value by construction."""
    out = [("all-zero digits", bytes(n)), ("all-0xF digits", b"\xff" * n)]
    for pos in range(2 * n):
        out.append((f"digit 0 at {pos} among 0xF", _node([0 if i == pos else 15 for i in range(2 * n)])))
        out.append((f"digit 0xF at {pos} among 0", _node([15 if i == pos else 0 for i in range(2 * n)])))
    for t in CSUM_TARGETS + (30 * n - 1,):
        if t <= 30 * n:
            out.append((f"checksum {t}", _with_csum(n, t)))
    for r in range(16):
        out.append((f"rotation {r}", _node([(i + r) & 15 for i in range(2 * n)])))
    for j in range(30 * n // 17 + 1):
        out.append((f"checksum ladder {17 * j}", _with_csum(n, 17 * j)))
    for i in range(64):
        out.append((f"random {i}", rand(f"wots/{n}/{i}", n)))
    return out


# ------------------------------------------------------------------ bit patterns
def walk(nbytes: int, ones: bool = False) -> list:
    """A single 1 (or a single 0 among ones) at every bit of nbytes bytes; bit b is bit 7 - b % 8 of byte b // 8."""
    out = []
    for b in range(8 * nbytes):
        v = 1 << (8 * nbytes - 1 - b)
        if ones:
            v ^= (1 << (8 * nbytes)) - 1
        out.append(v.to_bytes(nbytes, "big"))
    return out


def md_patterns(name: str) -> list:
    """(label, md) pairs over the p.md bytes of md, the unused bits of the last byte included."""
    p = spec.PARAMS[name]
    out = [("zeros", bytes(p.md)), ("ones", b"\xff" * p.md)]
    out += [(f"one at bit {b}", v) for b, v in enumerate(walk(p.md))]
    out += [(f"zero at bit {b}", v) for b, v in enumerate(walk(p.md, ones=True))]
    out += [(f"random {i}", rand(f"md/{name}/{i}", p.md)) for i in range(64)]
    return out


def index_digests(name: str) -> list:
    """(label, digest) pairs: m bytes whose md part is random and whose nine index bytes hold the pattern."""
    p = spec.PARAMS[name]
    assert p.m == p.md + 9
    head = rand(f"digest-md/{name}", p.md)
    pats = [("zeros", bytes(9)), ("ones", b"\xff" * 9)]
    pats += [(f"one at bit {b}", v) for b, v in enumerate(walk(9))]
    pats += [(f"zero at bit {b}", v) for b, v in enumerate(walk(9, ones=True))]
    pats += [(f"random {i}", rand(f"digest/{name}/{i}", 9)) for i in range(64)]
    return [(label, head + v) for label, v in pats]


def layer_indices(p: spec.Params, digest: bytes) -> list:
    """The d (tree, leaf) pairs in plain integers: split_digest, then h' bits at a time."""
    _, tree, leaf = spec.split_digest(p, digest)
    out = []
    for _ in range(p.d):
        out.append((tree, leaf))
        leaf = tree & ((1 << p.hp) - 1)
        tree >>= p.hp
    return out


# ------------------------------------------------------------------ addresses
class Address(NamedTuple):
    layer: int
    tree: int
    type: int
    w1: int
    w2: int
    w3: int


WIDTHS = (8, 64, 8, 32, 32, 32)
ONES = tuple((1 << w) - 1 for w in WIDTHS)


def addresses(n: int) -> list:
    """(label, Address) pairs for parameter set n."""
    p = params_of(n)
    top_tree = (1 << (p.h - p.hp)) - 1
    leaf, chain, fors = (1 << p.hp) - 1, p.len - 1, (p.k << p.a) - 1
    out = [(f"type {t}", Address(3, 0x0123456789ABCDEF & top_tree, t, 5, 6, 7)) for t in range(7)]
    out.append(("layer d - 1", Address(p.d - 1, 0, spec.TREE, 0, p.hp, 0)))
    out.append(("largest tree", Address(0, top_tree, spec.FORS_TREE, leaf, 0, 1)))
    if n == 32:
        out.append(("tree 2^64 - 1", Address(0, (1 << 64) - 1, spec.WOTS_HASH, 1, 2, 3)))
    out.append(("largest words", Address(p.d - 1, top_tree, spec.FORS_TREE, leaf, chain, fors)))
    out.append(("largest chain", Address(p.d - 1, top_tree, spec.WOTS_HASH, leaf, chain, 14)))
    for f, name in enumerate(Address._fields):
        out.append((f"only {name} all-ones", Address(*[ONES[i] if i == f else 0 for i in range(6)])))
        out.append((f"only {name} zero", Address(*[0 if i == f else ONES[i] for i in range(6)])))
    return out


def adrs_bytes(a: Address) -> bytes:
    return spec.adrs(*a)


class HashCase(NamedTuple):
    label: str
    seed: bytes
    adrs: Address
    nodes: bytes  # one node for F, left || right for H, l nodes for T_l


def hash_cases(n: int, nodes: int, tag: str) -> list:
    return [HashCase(label, rand(f"{tag}/{n}/seed/{label}", n), a, rand(f"{tag}/{n}/nodes/{label}", nodes * n))
            for label, a in addresses(n)]


# ------------------------------------------------------------------ H_msg
H_MSG_LENGTHS = range(301)


def h_msg_contexts(name: str) -> tuple:
    return (b"", b"\x5a", rand(f"ctx/{name}", 255)) if spec.PARAMS[name].fips else (b"",)


def h_msg_cases(name: str, ctx: bytes) -> list:
    """(R, PK.seed || PK.root, message) for every message length 0..300."""
    p = spec.PARAMS[name]
    return [(rand(f"hmsg/{name}/{len(ctx)}/r/{k}", p.n), rand(f"hmsg/{name}/{len(ctx)}/pk/{k}", 2 * p.n),
             rand(f"hmsg/{name}/{len(ctx)}/m/{k}", k)) for k in H_MSG_LENGTHS]


def h_msg_expected(name: str, ctx: bytes, r: bytes, pkr: bytes, msg: bytes) -> bytes:
    p = spec.PARAMS[name]
    return spec.Hasher(p, pkr[:p.n]).H_msg(r, pkr[p.n:], spec._frame(p, msg, ctx))


# ------------------------------------------------------------------ SHA-2 in plain Python
def _primes(count: int) -> list:
    out, c = [], 2
    while len(out) < count:
        if all(c % q for q in out):
            out.append(c)
        c += 1
    return out


def _icbrt(v: int) -> int:
    x = 1 << ((v.bit_length() + 2) // 3)
    while True:
        y = (2 * x + v // (x * x)) // 3
        if y >= x:
            return x
        x = y


class Sha2(NamedTuple):
    """FIPS 180-4 SHA-256 (bits = 32) or SHA-512 (bits = 64); the constants are the fractional parts of the
    square and cube roots of the first primes, computed here."""
    bits: int
    rounds: int
    rot: tuple  # S0, S1 (three rotations each), s0, s1 (two rotations and a shift each)

    @property
    def mask(self) -> int:
        return (1 << self.bits) - 1

    @property
    def block(self) -> int:
        return 2 * self.bits

    def iv(self) -> list:
        return [math.isqrt(q << (2 * self.bits)) & self.mask for q in _primes(8)]

    def k(self) -> list:
        return [_icbrt(q << (3 * self.bits)) & self.mask for q in _primes(self.rounds)]

    def _r(self, x: int, s: int) -> int:
        return ((x >> s) | (x << (self.bits - s))) & self.mask

    def compress(self, state: list, block: bytes) -> list:
        assert len(block) == self.block
        wb = self.bits // 8
        w = [int.from_bytes(block[wb * t:wb * (t + 1)], "big") for t in range(16)]
        S0, S1, s0, s1 = self.rot
        for t in range(16, self.rounds):
            x, y = w[t - 15], w[t - 2]
            a = self._r(x, s0[0]) ^ self._r(x, s0[1]) ^ (x >> s0[2])
            b = self._r(y, s1[0]) ^ self._r(y, s1[1]) ^ (y >> s1[2])
            w.append((w[t - 16] + a + w[t - 7] + b) & self.mask)
        k = _K[self.bits]
        a, b, c, d, e, f, g, h = state
        for t in range(self.rounds):
            t1 = (h + (self._r(e, S1[0]) ^ self._r(e, S1[1]) ^ self._r(e, S1[2])) + ((e & f) ^ (~e & self.mask & g)) +
                  k[t] + w[t]) & self.mask
            t2 = ((self._r(a, S0[0]) ^ self._r(a, S0[1]) ^ self._r(a, S0[2])) + ((a & b) ^ (a & c) ^ (b & c))) & self.mask
            a, b, c, d, e, f, g, h = (t1 + t2) & self.mask, a, b, c, (d + t1) & self.mask, e, f, g
        return [(s + v) & self.mask for s, v in zip(state, (a, b, c, d, e, f, g, h))]

    def padded(self, prefix: int, data: bytes) -> bytes:
        """data || 0x80 || zeros || the bit length of prefix + len(data) bytes, to a whole number of blocks."""
        lenb = self.bits // 4
        pad = (-(len(data) + 1 + lenb)) % self.block
        return data + b"\x80" + bytes(pad) + (8 * (prefix + len(data))).to_bytes(lenb, "big")

    def tail(self, state: list, prefix: int, data: bytes, over: dict | None = None) -> list:
        """The state after the padded end of a stream whose first `prefix` bytes are in `state`; over: word
        index -> value replacing that word of the first tail block."""
        buf = bytearray(self.padded(prefix, data))
        wb = self.bits // 8
        for t, v in (over or {}).items():
            buf[wb * t:wb * (t + 1)] = v.to_bytes(wb, "big")
        for b in range(0, len(buf), self.block):
            state = self.compress(state, bytes(buf[b:b + self.block]))
        return state

    def digest(self, data: bytes) -> bytes:
        return b"".join(v.to_bytes(self.bits // 8, "big") for v in self.tail(self.iv(), 0, data))


SHA256 = Sha2(32, 64, ((2, 13, 22), (6, 11, 25), (7, 18, 3), (17, 19, 10)))
SHA512 = Sha2(64, 80, ((28, 34, 39), (14, 18, 41), (1, 8, 7), (19, 61, 6)))
_K = {32: SHA256.k(), 64: SHA512.k()}


class TailCase(NamedTuple):
    label: str
    state: list
    prefix: int
    data: bytes
    over: dict  # word index -> value, words of tail block 0 held in registers


def tail_cases(big: bool) -> list:
    """Group 1: every length 0..200 from the initial state (hashlib is the reference).  Group 2: a random
    state with prefixes up to 2^31, so that the upper word of the bit length is set.  Group 3: words of block 0
    replaced from registers, as h_msg does for the inner digest."""
    h = SHA512 if big else SHA256
    tag = "512" if big else "256"
    wb = h.bits // 8
    out = [TailCase(f"initial state, {k} bytes", h.iv(), 0, rand(f"tail{tag}/a/{k}", k), {}) for k in range(201)]
    lens = (0, 1, 55, 56, 63, 64, 119) + ((111, 112, 127, 128) if big else ())
    for prefix in (h.block, 2**29 - h.block, 2**29, 2**31):
        for k in lens:
            st = [int.from_bytes(rand(f"tail{tag}/s/{prefix}/{k}/{j}", wb), "big") for j in range(8)]
            out.append(TailCase(f"random state, prefix {prefix}, {k} bytes", st, prefix,
                                rand(f"tail{tag}/b/{prefix}/{k}", k), {}))
    # (length, replaced words): the words after R || PK.seed as h_msg replaces them, in a tail of two blocks
    # and of one (there clear of the length words 14 and 15)
    first = 4 if big else 8
    for k, words in ((h.block + 36, range(first, first + 8)), (20, range(first, 14)), (h.block, range(16))):
        over = {t: int.from_bytes(rand(f"tail{tag}/o/{k}/{t}", wb), "big") for t in words}
        st = [int.from_bytes(rand(f"tail{tag}/os/{k}/{j}", wb), "big") for j in range(8)]
        out.append(TailCase(f"words {words[0]}..{words[-1]} replaced, {k} bytes", st, h.block,
                            rand(f"tail{tag}/ob/{k}", k), over))
    assert all(c.prefix % h.block == 0 and c.prefix + len(c.data) < 2**32 for c in out)
    return out


# ------------------------------------------------------------------ row_span
class SpanCase(NamedTuple):
    label: str
    o0: int
    o1: int
    accepted: bool


ROW_SPANS = (
    SpanCase("empty row", 0, 0, True),
    SpanCase("largest accepted span", 0, 2**31 - 1, True),
    SpanCase("smallest refused span", 0, 2**31, False),
    SpanCase("largest accepted span, offset", 7, 7 + 2**31 - 1, True),
    SpanCase("smallest refused span, offset", 7, 7 + 2**31, False),
    SpanCase("decreasing offsets", 5, 4, False),
    SpanCase("large start, small row", 2**40, 2**40 + 7, True),
    SpanCase("start near the top of the range", 2**63, 2**63 + 1, True),
    SpanCase("wrap", 2**64 - 1, 0, False),
    SpanCase("whole-range span", 0, 2**64 - 1, False),
)
