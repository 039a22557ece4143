"""Chosen inputs for FrodoKEM Decaps' decryption M = C - B'S and mu' = Decode(M) -- TEST INFRASTRUCTURE.

Shared by tests/test_gpu_frodo_decrypt.py (the HIP kernels) and tests/test_frodo_edge_oracle.py (the C
oracle against oracle/py/frodo_spec.py on the same S^T cases).  Everything is numpy int64 arithmetic
mod q on values chosen here; keys and ciphertexts are assembled in the usual byte layout with the
packers of tests/golden/make_golden_frodo_edge.py.
"""
import numpy as np

import frodo_spec as F
import make_golden_frodo_edge as E

NBAR = F.NBAR


def honest_key(alg: str) -> tuple[bytes, bytes]:
    """One honest key pair of the C oracle, from fixed coins."""
    import oracle as orc
    return orc.keypair(alg, bytes(range(F.params(alg)["keypair_coins"])))


def assemble_ct(p: dict, Bp: np.ndarray, C: np.ndarray) -> np.ndarray:
    """ct rows = Pack(B') || Pack(C) from B' [rows, 8, n] (None: zero) and C [rows, 8, 8] (mod q)."""
    rows = C.shape[0]
    c1 = np.zeros((rows, p["logq"] * p["n"]), np.uint8) if Bp is None else E.pack_rows(Bp.reshape(rows, -1), p["logq"])
    return np.concatenate([c1, E.pack_rows(C.reshape(rows, -1), p["logq"])], axis=1)


def with_st(p: dict, sk: bytes, St: np.ndarray) -> np.ndarray:
    """sk rows: the honest sk with its S^T replaced by St [rows, 8, n] (16-bit two's complement)."""
    rows = St.shape[0]
    out = np.tile(np.frombuffer(sk, np.uint8), (rows, 1))
    off = p["sec"] + p["pk"]
    out[:, off:off + 2 * NBAR * p["n"]] = (St.reshape(rows, -1) & 0xFFFF).astype("<u2").view(np.uint8)
    return out


def decode_rows(p: dict, M: np.ndarray) -> np.ndarray:
    """frodo_spec.decode of every M [rows, 8, 8] -> uint8 [rows, 32] (len_mu bytes, then zeros)."""
    out = np.zeros((M.shape[0], 32), np.uint8)
    for r in range(M.shape[0]):
        out[r, :p["len_mu"]] = np.frombuffer(F.decode(p, M[r]), np.uint8)
    return out


# ---------------------------------------------------------------- Decode over the whole residue ring
def ring_rows(p: dict) -> np.ndarray:
    """C [q/64, 8, 8]: every residue 0..q-1 exactly once.  Residue v sits in row r = v mod R (R = q/64)
    at position (v div R + r) mod 64, so a row walks the ring in steps of R (every symbol 64 / 2^B times)
    and consecutive residues land in consecutive rows at different positions."""
    q = 1 << p["logq"]
    R = q // 64
    v = np.arange(q, dtype=np.int64)
    r = v % R
    C = np.full((R, 64), -1, np.int64)
    C[r, (v // R + r) % 64] = v
    assert np.array_equal(np.sort(C.ravel()), v)
    return C.reshape(R, NBAR, NBAR)


def threshold_rows(p: dict) -> np.ndarray:
    """C [4 2^B, 8, 8]: row r, position pos holds T_m + d with T_m = (2m + 1) 2^(logq-B-1) the upper
    threshold of symbol m = (pos + r) mod 2^B and d = (-2, -1, 0, +1)[r div 2^B]: every position meets
    every threshold from both sides, neighbouring positions different symbols."""
    nsym, q = 1 << p["B"], 1 << p["logq"]
    r = np.arange(4 * nsym, dtype=np.int64)[:, None]
    pos = np.arange(64, dtype=np.int64)[None, :]
    m = (pos + r) % nsym
    d = np.array([-2, -1, 0, 1], np.int64)[r // nsym]
    C = ((2 * m + 1) * E.th(p) + d) % q
    return C.reshape(-1, NBAR, NBAR)


# ---------------------------------------------------------------- the product at its extremes
def onehot_positions(n: int) -> list[tuple[int, int]]:
    return [(k, j) for k in (0, 7) for j in (0, 1, 7, 8, n // 4 - 1, n // 4, n // 2, 3 * n // 4 - 1, n - 1)]


def product_cases(alg: str, per_case: int = 2, seed: int = 2024):
    """(names, St [rows, 8, n], B' [rows, 8, n], C [rows, 8, 8], M [rows, 8, 8]) with S^T entries as
    signed 16-bit values, M = C - B' S mod q in int64.  S^T: every entry 0x8000, every entry 0x7FFF,
    +-12 alternating, uniform int16 -- each against B' all q-1 and B' uniform -- then one entry +1 or -1
    at each onehot_positions (k, j) against the ramp B'[i][j] = (i n + j) mod q.  C is uniform."""
    p = F.params(alg)
    n, q = p["n"], 1 << p["logq"]
    rng = np.random.default_rng(seed + n)
    kk, jj = np.meshgrid(np.arange(NBAR), np.arange(n), indexing="ij")
    names, St, Bp = [], [], []
    dense = {
        "0x8000": lambda: np.full((NBAR, n), -0x8000, np.int64),
        "0x7FFF": lambda: np.full((NBAR, n), 0x7FFF, np.int64),
        "+-12": lambda: np.where((kk + jj) % 2 == 0, 12, -12).astype(np.int64),
        "int16": lambda: rng.integers(-0x8000, 0x8000, (NBAR, n), dtype=np.int64),
    }
    for sname, mk in dense.items():
        for bname in ("q-1", "uniform"):
            for _ in range(per_case):
                names.append(f"S^T {sname}, B' {bname}")
                St.append(mk())
                Bp.append(np.full((NBAR, n), q - 1, np.int64) if bname == "q-1" else rng.integers(0, q, (NBAR, n)))
    ramp = (np.arange(NBAR * n, dtype=np.int64) % q).reshape(NBAR, n)
    for k, j in onehot_positions(n):
        for s in (1, -1):
            one = np.zeros((NBAR, n), np.int64)
            one[k, j] = s
            names.append(f"S^T[{k}][{j}] = {s:+d}, B' ramp")
            St.append(one)
            Bp.append(ramp)
    St, Bp = np.stack(St), np.stack(Bp)
    C = rng.integers(0, q, (len(names), NBAR, NBAR), dtype=np.int64)
    M = (C - Bp @ St.transpose(0, 2, 1)) % q
    return names, St, Bp, C, M


# ---------------------------------------------------------------- Encaps on public keys at the edges of B
def edge_pks(alg: str) -> np.ndarray:
    """pk rows [3, pk]: an honest seedA with B all q-1, B all zero, B rows alternating 0 and q-1."""
    p = F.params(alg)
    n, q = p["n"], 1 << p["logq"]
    seed_a = np.frombuffer(honest_key(alg)[0][:16], np.uint8)
    B = np.zeros((3, n, NBAR), np.int64)
    B[0] = q - 1
    B[2, 1::2] = q - 1
    return np.concatenate([np.tile(seed_a, (3, 1)), E.pack_rows(B.reshape(3, -1), p["logq"])], axis=1)
