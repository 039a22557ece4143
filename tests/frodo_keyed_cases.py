"""Models and chosen inputs for the FrodoKEM key sets -- TEST INFRASTRUCTURE.

Shared by tests/test_gpu_frodo_keyed.py (the HIP kernels) and tests/test_frodo_keyed_cases.py (the models themselves,
on the CPU).  Three things the kernels of csrc/frodo_keyed.hip do that no per-row kernel does:

1. group the rows of a chunk by key (k_frk_group): group_model is the same stable counting sort in numpy -- a
   permutation of the rows with an index inside the set, a tile table of at most TILE same-key rows per tile, tiles
   ending at key borders;
2. store A as two int8 limb planes (A = 256 hi + lo): limb_split;
3. multiply S' of all rows of a tile with the stored A (k_frk_sa): expected_ct computes the ciphertext with plain
   u16 matrix arithmetic (frodo_spec.pack / unpack / encode for the bytes), from A as a matrix -- no limbs, no tiles.

TILE, KFRAG, KSTAGE, CFRAG, CBLOCK are the kernel's shapes (FRK_TH, the 64-row MFMA step, FRK_KC, the 16-column
fragment, FRK_CB): the borders the chosen matrices put their entries on.
"""
import hashlib

import numpy as np

import frodo_spec as F

NBAR = F.NBAR
TILE, KFRAG, KSTAGE, CFRAG, CBLOCK = 16, 64, 128, 16, 128
SHAKE = ["FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE"]
ALGS = SHAKE + [a.replace("SHAKE", "AES") for a in SHAKE]
SMAX = {640: 12, 976: 10, 1344: 6}
EDGE_VALUES = [0x0000, 0x007F, 0x0080, 0x00FF, 0x7F80, 0x7FFF, 0x8000, 0xFF80, 0xFFFF]
ROW_COUNTS = [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1]
SET_SIZES = [1, 2, 17]
REFUSED = 0xFFFFFFFF  # an index outside every set


def pitch(n: int) -> int:
    return (n + 127) // 128 * 128


def set_bytes(n: int, secret: bool, g: int) -> int:
    """Device bytes of a set of g keys, the formula include/qrkem.h documents: per key 2 n^2 (limb planes) + 16 n (B)
    + 32 (pkh), a secret key 16 n (S^T) + 32 (s) more; every part 256-aligned, the planes with 256 bytes of slack."""
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    total = al(2 * n * n * g + 256) + al(16 * n * g) + al(32 * g)
    return total + (al(16 * n * g) + al(32 * g) if secret else 0)


def edge_values(n: int) -> list:
    """The limb-edge entries; FrodoKEM-640's A is 15-bit, so its list is the values of that range."""
    return [v for v in EDGE_VALUES if n != 640 or v < 0x8000]


# ---------------------------------------------------------------- 1. grouping
def group_model(key_index, g: int, tile: int = TILE):
    """(perm, tiles, refused): perm = the rows with key_index < g, sorted by key, stable; tiles = [(key, first slot
    of perm, rows)] in key order, at most `tile` rows each; refused = the other rows.  key_index None: all key 0."""
    k = np.asarray(key_index, dtype=np.int64)
    ok = k < g
    rows = np.flatnonzero(ok)
    perm = rows[np.argsort(k[rows], kind="stable")]
    tiles, slot = [], 0
    for key, cnt in zip(*np.unique(k[rows], return_counts=True)):
        for t0 in range(0, int(cnt), tile):
            tiles.append((int(key), slot + t0, min(tile, int(cnt) - t0)))
        slot += int(cnt)
    return perm, tiles, np.flatnonzero(~ok)


def index_patterns(g: int, n: int, seed: int = 0):
    """name -> key_index (uint32 [n]) for a set of g keys: the patterns every parity case runs."""
    rng = np.random.default_rng(0xF20D0 + 131 * g + n + seed)
    i = np.arange(n, dtype=np.int64)
    out = {"zeros": np.zeros(n, np.int64), "last": np.full(n, g - 1, np.int64), "mod": i % g,
           "reversed": (n - 1 - i) % g, "random": rng.integers(0, g, n)}
    lone = np.full(n, g - 1, np.int64)  # one key with exactly one row among many of another
    lone[n // 2] = 0
    out["lone"] = lone
    return {k: v.astype(np.uint32) for k, v in out.items()}


# ---------------------------------------------------------------- 2. limbs
def limb_split(A):
    """(lo, hi) int8 with A == 256 hi + lo mod 2^16: lo = the low byte, hi = the high byte of A + 128, as int8."""
    a = np.asarray(A).astype(np.int64) & 0xFFFF
    lo = (a & 0xFF).astype(np.uint8).view(np.int8)
    hi = (((a + 128) >> 8) & 0xFF).astype(np.uint8).view(np.int8)
    return lo, hi


# ---------------------------------------------------------------- 3. chosen matrices and samples
def derive(alg: str, what: str, outlen: int) -> np.ndarray:
    return np.frombuffer(hashlib.shake_256(b"qrk-frodo-keyed" + alg.encode() + what.encode()).digest(outlen), np.uint8)


def border_rows(n: int) -> list:
    """First and last row of A, of every 64-row MFMA step and of every 128-row staging step of S'."""
    s = {0, n - 1}
    for b in range(0, n, KFRAG):
        s |= {b, min(n, b + KFRAG) - 1}
    return sorted(s)


def border_cols(n: int) -> list:
    """First and last column of A, of every 16-column fragment and (among them) of every 128-column workgroup."""
    s = {0, n - 1}
    for b in range(0, n, CFRAG):
        s |= {b, b + CFRAG - 1}
    return sorted(s)


def chosen_matrices(alg: str):
    """[(label, A u16 [n][n])]: every limb-edge value as a constant matrix; one-hot at the four corners of A and on
    both sides of the first 64-row step, 128-row staging step, 16-column fragment and 128-column workgroup border;
    and two matrices that are zero except on the border rows x border columns of every tile of the kernel, where each
    entry is a limb-edge value picked by position (so an entry read from a neighbouring position shows).  The last
    two carry all borders at once: less sharp than one one-hot matrix per border (a matrix is a key of 2 n^2 bytes),
    which is why the values differ by position and come in two shifts.  The 144-byte pitch of the staged S' rows is
    exercised through the S' patterns (every staged byte nonzero), not by a matrix."""
    n = F.params(alg)["n"]
    vals = edge_values(n)
    out = [(f"constant {v:#06x}", np.full((n, n), v, np.uint16)) for v in vals]
    corners = ((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1))
    inner = ((KFRAG - 1, CFRAG - 1), (KFRAG, CFRAG), (KSTAGE - 1, CBLOCK - 1), (KSTAGE, CBLOCK))
    for r, c in corners + inner:
        A = np.zeros((n, n), np.uint16)
        A[r, c] = vals[-1]
        out.append((f"one-hot [{r}][{c}]", A))
    R, C = np.array(border_rows(n)), np.array(border_cols(n))
    for shift in (0, 4):
        A = np.zeros((n, n), np.uint16)
        pick = (np.arange(len(R))[:, None] * len(C) + np.arange(len(C))[None, :] + shift) % (len(vals) - 1) + 1  # not 0
        A[np.ix_(R, C)] = np.array(vals, np.uint16)[pick]
        out.append((f"tile borders, values shifted by {shift}", A))
    return out


def sample_patterns(alg: str):
    """[(label, S' int8 [8][n])]: all +max, all -max, alternating signs, one-hot at column 0 and at column n - 1."""
    n = F.params(alg)["n"]
    m = SMAX[n]
    alt = np.where((np.add.outer(np.arange(NBAR), np.arange(n)) & 1) == 0, m, -m).astype(np.int8)
    first, last = np.zeros((NBAR, n), np.int8), np.zeros((NBAR, n), np.int8)
    first[:, 0] = [m, -m] * 4
    last[:, n - 1] = [-m, m] * 4
    return [("all +max", np.full((NBAR, n), m, np.int8)), ("all -max", np.full((NBAR, n), -m, np.int8)),
            ("alternating", alt), ("one-hot column 0", first), (f"one-hot column {n - 1}", last)]


def edge_rows(alg: str):
    """The rows of the limb / layout test: every chosen matrix is a key, every (key, S' pattern) pair a row, ordered
    so that neighbouring rows name different keys.  Returns dict(matrices [g][n][n], labels, key_index, s8, e16,
    epp16, mu, pk [g][pk])."""
    p = F.params(alg)
    n, m = p["n"], SMAX[p["n"]]
    mats, pats = chosen_matrices(alg), sample_patterns(alg)
    g = len(mats)
    pairs = [(k, s) for s in range(len(pats)) for k in range(g)]  # key fastest: the keys interleave
    rows = len(pairs)
    rng = np.random.default_rng(0xED6E + n)
    s8 = np.zeros((rows, NBAR, pitch(n)), np.int8)
    for i, (_, s) in enumerate(pairs):
        s8[i, :, :n] = pats[s][1]
    return {"matrices": np.stack([A for _, A in mats]), "key_index": np.array([k for k, _ in pairs], np.uint32),
            "labels": [f"A {mats[k][0]}, S' {pats[s][0]}" for k, s in pairs], "s8": s8,
            "e16": rng.integers(-m, m + 1, (rows, NBAR * n)).astype(np.int16),
            "epp16": rng.integers(-m, m + 1, (rows, 64)).astype(np.int16),
            "mu": derive(alg, "mu", rows * p["len_mu"]).reshape(rows, p["len_mu"]).copy(),
            "pk": derive(alg, "pk", g * p["pk"]).reshape(g, p["pk"]).copy()}


def expected_ct(alg: str, A, pk: bytes, s8, e16, epp16, mu: bytes) -> bytes:
    """ct of one row: Pack(S'A + E') || Pack(S'B + E'' + Encode(mu)) mod q, plain matrix arithmetic mod 2^16.  The
    products go through float64, which is exact here (|sum| <= n 65535 12 < 2^53)."""
    p = F.params(alg)
    n, logq = p["n"], p["logq"]
    q = (1 << logq) - 1
    Sp = np.asarray(s8)[:, :n].astype(np.float64)
    SA = (Sp @ np.asarray(A).astype(np.float64)).astype(np.int64)
    Bp = (SA + np.asarray(e16).reshape(NBAR, n).astype(np.int64)) & q
    Bpk = F.unpack(bytes(pk[16:]), n * NBAR, logq).reshape(n, NBAR)
    V = (Sp @ Bpk.astype(np.float64)).astype(np.int64) + np.asarray(epp16).reshape(NBAR, NBAR).astype(np.int64)
    Cm = (V + F.encode(p, bytes(mu)).astype(np.int64)) & q
    return F.pack(Bp, logq) + F.pack(Cm, logq)
