"""Chosen inputs for the FrodoKEM forward path (KeyGen, Encaps, Decaps' re-encryption) -- TEST INFRASTRUCTURE.

Shared by tests/test_gpu_frodo_forward.py (the HIP kernels, through the hooks qrk_dbg_frodo_sample and
qrk_dbg_frodo_from_samples and through the public calls), tests/test_frodo_forward_cases.py (the reference itself,
on the CPU) and tests/golden/make_golden_frodo_forward.py (SHA-256 of the expected outputs, because the pure-Python
AES Gen(A) of FrodoKEM-976 / -1344 takes seconds).  Every input is built by rule from SHAKE256(TAG || alg || what),
as in tests/golden/make_golden_frodo_edge.py; every expected byte comes from oracle/py/frodo_spec.py (gen_a, sample,
pack, unpack, encode, _mm through keygen_from_samples / encrypt_from_samples) or, for the public calls, from the C
oracle, which tests/test_frodo_forward_cases.py holds to frodo_spec on these very rows.  The only facts about the
sampler used here are the specification's CDF tables (frodo_spec) and the maxima they imply.

1. The sampler alone: every 16-bit word, and the words at every table boundary placed at the ends of every region.
2. Products and packing from crafted sample matrices: CASES below.
3. Crafted public keys (every byte string of the right length is one) and secret keys with S^T at the int16 ends.
"""
import contextlib
import functools
import hashlib

import numpy as np

import frodo_spec as F
import make_golden_frodo_edge as E

NBAR = F.NBAR
ALGS = ["FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE",
        "FrodoKEM-640-AES", "FrodoKEM-976-AES", "FrodoKEM-1344-AES"]
TAG = b"qrk-frodo-forward"


def derive(alg: str, what: bytes, outlen: int) -> bytes:
    return hashlib.shake_256(TAG + alg.encode() + what).digest(outlen)


def seed_a(alg: str) -> bytes:
    """The one seedA of a name: every crafted key and every from-samples case uses it, so A is generated once."""
    return derive(alg, b"seedA", 16)


def smax(p: dict) -> int:
    """The largest |sample|: the number of CDF entries below the last (32767, which no 15-bit value exceeds)."""
    m = len(p["cdf"]) - 1
    assert p["cdf"][-1] == 32767 and m == {640: 12, 976: 10, 1344: 6}[p["n"]]
    return m


def pitch(n: int) -> int:
    """Row pitch of S' / S^T in the hooks' layout: n rounded up to 128, the pad columns zero."""
    return (n + 127) // 128 * 128


_A = {}
_REAL_GEN_A = F.gen_a


@contextlib.contextmanager
def memo_gen_a():
    """frodo_spec.gen_a computed once per (set, seedA) while the block runs: the AES matrices are 51,200 / 119,072 /
    225,792 pure-Python blocks."""
    def gen_a(p, s):
        key = (p["n"], p["prg"], bytes(s))
        if key not in _A:
            _A[key] = _REAL_GEN_A(p, s)
        return _A[key]
    prev, F.gen_a = F.gen_a, gen_a
    try:
        yield
    finally:
        F.gen_a = prev


# ---------------------------------------------------------------- 1. the sampler alone
def words_per_row(p: dict, kg: bool) -> int:
    return 2 * p["n"] * NBAR if kg else (2 * p["n"] + NBAR) * NBAR


def regions(p: dict, kg: bool) -> list[tuple[str, int]]:
    """(name, index in the row's word stream) of the first and last entry of every output region."""
    n8 = NBAR * p["n"]
    if kg:
        return [("S^T[0][0]", 0), (f"S^T[7][{p['n'] - 1}]", n8 - 1), ("E[0][0]", n8), (f"E[{p['n'] - 1}][7]", 2 * n8 - 1)]
    return [("S'[0][0]", 0), (f"S'[7][{p['n'] - 1}]", n8 - 1), ("E'[0][0]", n8), (f"E'[7][{p['n'] - 1}]", 2 * n8 - 1),
            ("E''[0]", 2 * n8), ("E''[63]", 2 * n8 + 63)]


def sampler_expected(p: dict, kg: bool, words: np.ndarray):
    """frodo_spec.sample of words uint16 [rows, words_per_row] in the hook's output layout:
    (s8 int8 [rows, 8, pitch] with zero pad columns, e16 int16 [rows, 8 n], epp16 int16 [rows, 64] or None)."""
    n, rows = p["n"], words.shape[0]
    assert words.shape[1] == words_per_row(p, kg)
    v = E.signed(F.sample(p, words))
    assert np.abs(v).max() <= smax(p)
    s8 = np.zeros((rows, NBAR, pitch(n)), np.int8)
    s8[:, :, :n] = v[:, :NBAR * n].reshape(rows, NBAR, n)
    e16 = v[:, NBAR * n:2 * NBAR * n].astype(np.int16)
    return s8, e16, (None if kg else v[:, 2 * NBAR * n:].astype(np.int16))


def every_word_rows(p: dict, kg: bool, shuffled: bool) -> np.ndarray:
    """All 65,536 words, ascending or in a fixed shuffle, over as many rows as it takes (7 / 5 / 4); the last row
    is filled by going round again."""
    seq = np.arange(1 << 16, dtype=np.int64)
    if shuffled:
        seq = np.random.default_rng(0x5AFF1E + p["n"] + int(kg)).permutation(seq)
    nv = words_per_row(p, kg)
    rows = -(-len(seq) // nv)
    assert rows == {640: 7, 976: 5, 1344: 4}[p["n"]]
    return np.resize(seq, rows * nv).reshape(rows, nv).astype(np.uint16)


def boundary_table(p: dict) -> list[tuple[int, int, str]]:
    """(word, sample, label).  prnd = word >> 1 and the sample counts the entries T[i] < prnd, negated when bit 0 is
    set: 2 T[j] and 2 T[j] + 1 give +-j (prnd = T[j] does not pass entry j), 2 T[j] + 2 and 2 T[j] + 3 give +-(j + 1)."""
    out = []
    for j, t in enumerate(p["cdf"][:-1]):
        for d, v in ((0, j), (1, -j), (2, j + 1), (3, -(j + 1))):
            out.append((2 * t + d, v, f"T[{j}] = {t}, word 2T+{d} = {2 * t + d}"))
    m = smax(p)
    return out + [(0, 0, "word 0"), (1, 0, "word 1 (minus zero)"), (0xFFFE, m, "word 0xFFFE"), (0xFFFF, -m, "word 0xFFFF")]


def boundary_streams(p: dict, kg: bool):
    """One stream per (boundary word, region end): the word there, zero (which samples to 0) everywhere else.
    (words uint16 [M, words_per_row], [(label, region, index, sample)] per stream)."""
    meta = [(label, rname, idx, v, w) for w, v, label in boundary_table(p) for rname, idx in regions(p, kg)]
    words = np.zeros((len(meta), words_per_row(p, kg)), np.uint16)
    for i, (_, _, idx, _, w) in enumerate(meta):
        words[i, idx] = w
    return words, [m[:4] for m in meta]


# ---------------------------------------------------------------- 2. crafted sample matrices
MATRIX_KINDS = ("+max", "-max", "zero", "altrow", "altcol", "honest")  # and "onehot", below
E_KINDS = ("+max", "-max", "zero")
MU_KINDS = ("00", "FF")


def onehot_positions(n: int) -> list[tuple[int, int]]:
    """(k, j): rows 0 and 7 of S' / S^T; columns at the borders of the 64-row wave tiles (63 | 64, 127 | 128), of the
    last whole tile, of the partial tile of 976 = 15 64 + 16 (n - 17 | n - 16) and at both ends."""
    return [(k, j) for k in (0, 7) for j in (0, 63, 64, 127, 128, n - 65, n - 64, n - 17, n - 16, n - 1)]


def case_list(n: int) -> list[tuple]:
    """The chosen list, the same for both modes and every name: (matrix kind, E kind, mu kind).

    * every dense matrix kind (all +max, all -max, zero, sign alternating by row, by column, an honest pseudo-random
      one) with every E kind (E' / E'' / E all +max, all -max, zero): 18 cases, mu alternating all-zero / all-0xFF.
      The order puts +max / +max beside +max / -max and -max / +max beside -max / -max: neighbours in the batch sit
      at opposite extremes;
    * one-hot +-max at each of the 20 onehot_positions, the sign alternating along j and opposite in rows 0 and 7,
      the E kind and mu cycling, so one-hot meets every E kind and both mu: 20 cases;
    * the control: honest matrix, honest E, pseudo-random mu.
    KeyGen takes no mu; its cases differ in S^T and E alone."""
    cases = [(m, e, MU_KINDS[(i + j) % 2]) for i, m in enumerate(MATRIX_KINDS) for j, e in enumerate(E_KINDS)]
    for idx, (k, j) in enumerate(onehot_positions(n)):
        sign = 1 if (idx + (k == 7)) % 2 == 0 else -1
        cases.append((("onehot", k, j, sign), E_KINDS[idx % 3], MU_KINDS[(idx // 3) % 2]))
    return cases + [("honest", "honest", "rand")]


def case_name(c: tuple) -> str:
    m = c[0] if isinstance(c[0], str) else f"onehot[{c[0][1]}][{c[0][2]}]{'+' if c[0][3] > 0 else '-'}max"
    return f"S {m} | E {c[1]} | mu {c[2]}"


def _honest(alg: str, what: bytes, count: int) -> np.ndarray:
    p = F.params(alg)
    return E.signed(F.sample(p, np.frombuffer(derive(alg, what, 2 * count), "<u2")))


def matrix(alg: str, kind, rows: int, cols: int, what: bytes) -> np.ndarray:
    """A [rows][cols] sample matrix (int64, signed) of the given kind."""
    m = smax(F.params(alg))
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    if kind == "zero":
        return np.zeros((rows, cols), np.int64)
    if kind in ("+max", "-max"):
        return np.full((rows, cols), m if kind == "+max" else -m, np.int64)
    if kind == "altrow":
        return np.where(r % 2 == 0, m, -m).astype(np.int64)
    if kind == "altcol":
        return np.where(c % 2 == 0, m, -m).astype(np.int64)
    if kind == "honest":
        return _honest(alg, b"honest" + what, rows * cols).reshape(rows, cols)
    _, k, j, sign = kind
    out = np.zeros((rows, cols), np.int64)
    out[k, j] = sign * m
    return out


@functools.lru_cache(maxsize=None)
def from_samples_inputs(alg: str, kg: bool) -> dict:
    """Inputs of every case of case_list, stacked in the hooks' layout: s8 int8 [cases, 8, pitch], e16 int16
    [cases, 8 n] (Encaps E' [8][n]; KeyGen E [n][8]), and for Encaps epp16 int16 [cases, 64], pk (the name's seedA,
    B pseudo-random) and mu; for KeyGen seedA rows."""
    p = F.params(alg)
    n, cases = p["n"], case_list(p["n"])
    s8 = np.zeros((len(cases), NBAR, pitch(n)), np.int8)
    e16 = np.zeros((len(cases), NBAR * n), np.int16)
    epp16 = np.zeros((len(cases), 64), np.int16)
    mu = np.zeros((len(cases), p["len_mu"]), np.uint8)
    for i, (mk, ek, muk) in enumerate(cases):
        s8[i, :, :n] = matrix(alg, mk, NBAR, n, b"S")
        e16[i] = (matrix(alg, ek, n, NBAR, b"E") if kg else matrix(alg, ek, NBAR, n, b"E'")).ravel()
        epp16[i] = matrix(alg, ek, NBAR, NBAR, b"E''").ravel()
        mu[i] = {"00": 0, "FF": 0xFF}.get(muk, 0) if muk != "rand" else np.frombuffer(derive(alg, b"mu", p["len_mu"]), np.uint8)
    out = {"names": [case_name(c) for c in cases], "s8": s8, "e16": e16}
    if kg:
        out["seedA"] = np.tile(np.frombuffer(seed_a(alg), np.uint8), (len(cases), 1))
    else:
        B = np.frombuffer(derive(alg, b"B", 2 * n * NBAR), "<u2").astype(np.int64) & ((1 << p["logq"]) - 1)
        pk = seed_a(alg) + E.pack_rows(B.reshape(1, -1), p["logq"]).tobytes()
        out.update(epp16=epp16, mu=mu, pk=np.tile(np.frombuffer(pk, np.uint8), (len(cases), 1)))
    return out


@functools.lru_cache(maxsize=None)
def from_samples_expected(alg: str, kg: bool) -> np.ndarray:
    """Expected output rows of every case: Encaps ct = Pack(S'A + E') || Pack(S'B + E'' + Encode(mu)); KeyGen
    pk = seedA || Pack(A S + E).  frodo_spec alone."""
    p, inp = F.params(alg), from_samples_inputs(alg, kg)
    n, out = p["n"], []
    with memo_gen_a():
        for i in range(len(inp["names"])):
            S = inp["s8"][i, :, :n].astype(np.int64)
            if kg:
                out.append(F.keygen_from_samples(p, seed_a(alg), S, inp["e16"][i].astype(np.int64).reshape(n, NBAR)))
            else:
                Bp, C = F.encrypt_from_samples(p, inp["pk"][i].tobytes(), S,
                                               inp["e16"][i].astype(np.int64).reshape(NBAR, n),
                                               inp["epp16"][i].astype(np.int64).reshape(NBAR, NBAR), inp["mu"][i].tobytes())
                out.append(F.pack(Bp, p["logq"]) + F.pack(C, p["logq"]))
    return np.stack([np.frombuffer(x, np.uint8) for x in out])


def keygen_sk_part(alg: str) -> np.ndarray:
    """What k_fr_kg_pack writes into sk beside the pk copy: S^T as int16 little-endian, [cases, 16 n] bytes."""
    p, inp = F.params(alg), from_samples_inputs(alg, True)
    return np.ascontiguousarray(inp["s8"][:, :, :p["n"]].astype("<i2")).view(np.uint8).reshape(len(inp["names"]), -1)


def digests(rows: np.ndarray) -> list[str]:
    return [hashlib.sha256(r.tobytes()).hexdigest() for r in rows]


def tiled(count: int, total: int) -> np.ndarray:
    """Row indices of a batch of `total` rows over `count` cases: the cases in order, again and again."""
    return np.arange(total) % count


# ---------------------------------------------------------------- 3. crafted keys through the public calls
def crafted_b(alg: str) -> tuple[list[str], np.ndarray]:
    """(names, B [kinds, n, 8] mod q) of the attacker-chosen public keys."""
    p = F.params(alg)
    n, q = p["n"], 1 << p["logq"]
    r, c = np.meshgrid(np.arange(n), np.arange(NBAR), indexing="ij")
    kinds = {
        "all 0": np.zeros((n, NBAR), np.int64),
        "all q-1": np.full((n, NBAR), q - 1, np.int64),
        "all q/2": np.full((n, NBAR), q // 2, np.int64),
        "0 / q-1 by row": np.where(r % 2 == 0, 0, q - 1),
        "0 / q-1 by column": np.where(c % 2 == 0, 0, q - 1),
        "0x5555 / 0x2AAA": np.where((r + c) % 2 == 0, 0x5555, 0x2AAA) & (q - 1),
    }
    for i, j in ((0, 0), (n - 1, 7), (n // 4, 3)):
        one = np.zeros((n, NBAR), np.int64)
        one[i, j] = q - 1
        kinds[f"one-hot q-1 at ({i},{j})"] = one
    kinds["random"] = np.frombuffer(derive(alg, b"crafted B", 2 * n * NBAR), "<u2").astype(np.int64).reshape(n, NBAR) & (q - 1)
    return list(kinds), np.stack([np.asarray(v, np.int64) for v in kinds.values()])


@functools.lru_cache(maxsize=None)
def honest_keys(alg: str, count: int) -> tuple[np.ndarray, np.ndarray]:
    import oracle as orc
    p = F.params(alg)
    coins = np.frombuffer(derive(alg, b"honest keys", count * p["keypair_coins"]), np.uint8).reshape(count, -1)
    return orc.batch_keypair(alg, np.ascontiguousarray(coins))


@functools.lru_cache(maxsize=None)
def encaps_rows(alg: str) -> dict:
    """Crafted public keys with an honest key after each: names, pk rows, mu rows (inputs only)."""
    p = F.params(alg)
    names, B = crafted_b(alg)
    crafted = np.concatenate([np.tile(np.frombuffer(seed_a(alg), np.uint8), (len(names), 1)),
                              E.pack_rows(B.reshape(len(names), -1), p["logq"])], axis=1)
    hpk, _ = honest_keys(alg, len(names))
    pk = np.empty((2 * len(names), p["pk"]), np.uint8)
    pk[0::2], pk[1::2] = crafted, hpk
    mu = np.frombuffer(derive(alg, b"encaps mu", len(pk) * p["len_mu"]), np.uint8).reshape(len(pk), -1)
    return {"names": [x for nm in names for x in ("B " + nm, "honest key")], "pk": pk, "mu": np.ascontiguousarray(mu)}


ST_KINDS = {"honest": None, "0x7FFF": 0x7FFF, "0x8000": 0x8000, "0xFFFF": 0xFFFF}
CT_PARTS = ("honest", "zeros", "ones")


@functools.lru_cache(maxsize=None)
def decaps_rows(alg: str) -> dict:
    """sk = s || pk || S^T || H(pk) rows and ciphertexts (inputs only; the Encaps under each pk is the C oracle's).

    * row 0: an honest key pair and its honest ciphertext (accepted);
    * the honest Encaps under every crafted pk, with the honest key's S^T (no secret matches a crafted B);
    * S^T honest / every word 0x7FFF / 0x8000 / 0xFFFF, crossed with B' and C each honest, all-zero or all-ones
      (all nine pairs; the all-honest pair only under the three extreme S^T again), the pk cycling through the
      crafted keys and the honest one."""
    import oracle as orc
    p = F.params(alg)
    n, sec, c1 = p["n"], p["sec"], p["logq"] * p["n"]
    enc = encaps_rows(alg)
    hpk, hsk = honest_keys(alg, len(enc["pk"]) // 2)
    pks = [enc["pk"][i] for i in range(0, len(enc["pk"]), 2)] + [hpk[0]]
    pk_names = enc["names"][0::2] + ["honest key"]
    s, st_honest = hsk[0][:sec], hsk[0][sec + p["pk"]:sec + p["pk"] + 2 * NBAR * n]
    plan = [(len(pks) - 1, "honest", "honest", "honest")] + [(i, "honest", "honest", "honest") for i in range(len(pks) - 1)]
    i = 0
    for st in ST_KINDS:
        for b in CT_PARTS:
            for c in CT_PARTS:
                if (st, b, c) != ("honest", "honest", "honest"):
                    plan.append((i % len(pks), st, b, c))
                    i += 1
    pk = np.stack([pks[t[0]] for t in plan])
    mu = np.frombuffer(derive(alg, b"decaps mu", len(plan) * p["len_mu"]), np.uint8).reshape(len(plan), -1)
    ct, ss_enc = orc.batch_encaps(alg, np.ascontiguousarray(pk), np.ascontiguousarray(mu))
    ct, sk = ct.copy(), np.empty((len(plan), p["sk"]), np.uint8)
    for r, (ip, st, b, c) in enumerate(plan):
        stb = st_honest if ST_KINDS[st] is None else np.full(NBAR * n, ST_KINDS[st], "<u2").view(np.uint8)
        sk[r] = np.concatenate([s, pk[r], stb, np.frombuffer(E.shake(p, pk[r].tobytes(), sec), np.uint8)])
        for part, lo, hi in ((b, 0, c1), (c, c1, p["ct"])):
            if part != "honest":
                ct[r, lo:hi] = 0 if part == "zeros" else 0xFF
    names = [f"pk {pk_names[ip]} | S^T {st} | B' {b} | C {c}" for ip, st, b, c in plan]
    return {"names": names, "sk": sk, "ct": ct, "ss_enc": ss_enc, "plan": plan}
