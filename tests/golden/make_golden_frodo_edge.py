"""Golden FrodoKEM encapsulations whose acceptance is decided at a decoding threshold
(tests/golden/frodo_edge.json) -- TEST INFRASTRUCTURE.

An honest ciphertext decrypts to Encode(mu) plus noise of a few hundred, far inside a decoding cell of
half-width th = 2^(logq - B - 1) (4096 / 4096 / 2048), so Decaps never meets Decode near a threshold.
These keys put it there with noise known in closed form.  With one seedA per set, S^T is zero except
S^T[i0][j0] = delta and E = 0, so B = A S has column i0 = delta A[:, j0] and zeros elsewhere, pkh = H(pk)
and sk = s || pk || S^T || pkh as usual.  For an honest Encaps with coins mu under that pk, Decaps
computes M = C - B'S = Encode(mu) + E'' - E'S, and (E'S)[k][i] = delta E'[k][j0] for i = i0, else 0:

    M - Encode(mu)  =  E''[k][i0] - delta E'[k][j0]   at (k, i0),      E''[k][i]   elsewhere.

With delta = th / m a sample E'[k][j0] = -+m puts position (k, i0) at +-th + E''[k][i0]: the row decodes
to mu -- and is accepted, since the re-encryption of mu is the ciphertext -- exactly when every noise
value e has -th <= e <= th - 1.  E' and E'' are the sampler's output on SHAKE(0x96 || seedSE) with
(seedSE || k) = H(pkh || mu): one hash stream per candidate mu, and only column j0 of A per key.

Search (deterministic).  seedA = SHAKE256("qrk-frodo-edge" || alg || "seedA"), 16 bytes; key t of a set
has (i0, j0) = KEYS(n)[t] and s = SHAKE256("qrk-frodo-edge" || alg || "s" || t); candidate c of key t is
mu = SHAKE256("qrk-frodo-edge" || alg || "mu" || t || LE64(c)).  Per key, in candidate order: the first
row decided by each exact value th-1, th, -th, -th-1 alone (one position of column i0 holds it, every
other position is SAFE: at least th/8 away from both thresholds), the first NEAR rows with a position
within 2 of a threshold, and the first PLAIN accepting and PLAIN rejecting rows without one.  Rows are
stored in candidate order, so accepting and rejecting rows alternate as the sampler dealt them.

Stored: seedA; per key (i0, j0, delta) and per row mu, the accept bit, the closed-form noise of column
i0, SHA-256 of the C oracle's ct and of its Encaps ss.  Keys and ciphertexts are rebuilt at test time
(build_key); tests/test_frodo_edge_oracle.py holds the C oracle and oracle/py/frodo_spec.py to these rows.

    python tests/golden/make_golden_frodo_edge.py
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1] / "oracle" / "py"), str(HERE.parents[1] / "oracle")]

import frodo_spec as F  # noqa: E402
from kat_drbg import aes_encrypt_block  # noqa: E402

ALGS = ("FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE", "FrodoKEM-640-AES")
M_DIV = {640: 4, 976: 4, 1344: 2}  # delta = th / m: the sample E' = -+m reaches the threshold
NEAR, PLAIN = 32, 6                # rows per key beside the four decided by one exact value
MAX_CANDIDATES = 20000
MAX_ROWS = 256                     # per set
NBAR = F.NBAR
TAG = b"qrk-frodo-edge"


def th(p: dict) -> int:
    return 1 << (p["logq"] - p["B"] - 1)


def keys_of(n: int) -> list[tuple[int, int]]:
    return [(0, 0), (3, n // 4), (7, n - 1)]


def shake(p: dict, data: bytes, outlen: int) -> bytes:
    """The parameter set's hash: SHAKE128 for FrodoKEM-640, SHAKE256 for -976 / -1344."""
    return (hashlib.shake_128 if p["n"] == 640 else hashlib.shake_256)(data).digest(outlen)


def derive(alg: str, what: bytes, outlen: int) -> bytes:
    return hashlib.shake_256(TAG + alg.encode() + what).digest(outlen)


def pack_rows(vals: np.ndarray, d: int) -> np.ndarray:
    """frodo_spec.pack of every row of vals [rows, count] (count a multiple of 8) -> uint8 [rows, count d / 8]."""
    v = np.asarray(vals, dtype=np.int64) & ((1 << d) - 1)
    if d == 16:  # whole big-endian words
        return np.ascontiguousarray(v.astype(">u2")).view(np.uint8).reshape(v.shape[0], -1)
    bits = (v[:, :, None] >> np.arange(d - 1, -1, -1)) & 1
    return np.packbits(bits.astype(np.uint8).reshape(v.shape[0], -1), axis=1)


def unpack_rows(data: np.ndarray, d: int) -> np.ndarray:
    """frodo_spec.unpack of every row of data uint8 [rows, bytes] -> int64 [rows, bytes 8 / d]."""
    bits = np.unpackbits(np.ascontiguousarray(data), axis=1).reshape(data.shape[0], -1, d).astype(np.int64)
    return (bits << np.arange(d - 1, -1, -1)).sum(axis=2)


def a_column(p: dict, seed_a: bytes, j0: int) -> np.ndarray:
    """Column j0 of A = Gen(seedA): n SHAKE128 rows, or n AES-128 blocks."""
    n = p["n"]
    col = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if p["prg"] == "SHAKE":
            row = hashlib.shake_128(i.to_bytes(2, "little") + seed_a).digest(2 * n)
            col[i] = int.from_bytes(row[2 * j0:2 * j0 + 2], "little")
        else:
            j = j0 & ~7
            blk = aes_encrypt_block(seed_a, i.to_bytes(2, "little") + j.to_bytes(2, "little") + bytes(12))
            col[i] = int.from_bytes(blk[2 * (j0 - j):2 * (j0 - j) + 2], "little")
    return col


def assemble_key(alg: str, seed_a: bytes, s: bytes, Bm: np.ndarray, St: np.ndarray) -> tuple[bytes, bytes]:
    """(pk, sk) in the usual layout from B [n][8] (mod q) and S^T [8][n] (any 16-bit values)."""
    p = F.params(alg)
    pk = seed_a + pack_rows(np.asarray(Bm).reshape(1, -1), p["logq"]).tobytes()
    St16 = (np.asarray(St, dtype=np.int64) & 0xFFFF).astype("<u2")
    sk = s + pk + St16.tobytes() + shake(p, pk, p["sec"])
    assert len(pk) == p["pk"] and len(sk) == p["sk"]
    return pk, sk


def build_key(alg: str, seed_a: bytes, t: int, i0: int, j0: int, delta: int) -> tuple[bytes, bytes]:
    """Key t of a set: S^T[i0][j0] = delta, E = 0, B = A S."""
    p = F.params(alg)
    n = p["n"]
    St = np.zeros((NBAR, n), dtype=np.int64)
    St[i0, j0] = delta
    Bm = np.zeros((n, NBAR), dtype=np.int64)
    Bm[:, i0] = (delta * a_column(p, seed_a, j0)) & ((1 << p["logq"]) - 1)
    return assemble_key(alg, seed_a, derive(alg, b"s" + bytes([t]), p["sec"]), Bm, St)


def signed(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.int64)
    return np.where(x >= 0x8000, x - 0x10000, x)


def noise_of(alg: str, pkh: bytes, mu: bytes, i0: int, j0: int, delta: int) -> np.ndarray:
    """M - Encode(mu) of an honest Encaps with coins mu under a build_key key, in closed form: [8][8]."""
    p = F.params(alg)
    n = p["n"]
    seed_se = shake(p, pkh + mu, 2 * p["sec"])[:p["sec"]]
    r = np.frombuffer(shake(p, b"\x96" + seed_se, (2 * n + NBAR) * NBAR * 2), dtype="<u2")
    Ep_col = signed(F.sample(p, r[n * NBAR:2 * n * NBAR]).reshape(NBAR, n)[:, j0])
    e = signed(F.sample(p, r[2 * n * NBAR:])).reshape(NBAR, NBAR)
    e[:, i0] -= delta * Ep_col
    return e


def near_threshold(p: dict, e) -> np.ndarray:
    """Within 2 of a threshold: the thresholds lie between th-1 | th and between -th-1 | -th, so
    th-2 .. th+1 and -th-2 .. -th+1."""
    T, e = th(p), np.asarray(e)
    return np.minimum(np.abs(e - (T - 0.5)), np.abs(e + (T + 0.5))) < 2


def decided_by(p: dict, col) -> int | None:
    """The exact value th-1 / th / -th / -th-1 that alone decides a row with noise `col` in column i0
    (every other position SAFE: at least th/8 away from both thresholds), else None.  Positions outside
    column i0 hold E'' alone, |E''| <= 12, and are always SAFE."""
    T, col = th(p), np.asarray(col)
    near = near_threshold(p, col)
    safe = (col >= -T + T // 8) & (col <= T - 1 - T // 8)
    if near.sum() == 1 and safe.sum() == col.size - 1 and int(col[near][0]) in (T - 1, T, -T, -T - 1):
        return int(col[near][0])
    return None


def classify(p: dict, e: np.ndarray, i0: int):
    """(accept, near, decider) of a row's noise e [8][8]."""
    T = th(p)
    accept = bool(np.all((e >= -T) & (e <= T - 1)))
    assert np.abs(np.delete(e, i0, axis=1)).max() <= 12
    return accept, bool(near_threshold(p, e).any()), decided_by(p, e[:, i0])


def search_key(alg: str, t: int, pkh: bytes, i0: int, j0: int, delta: int) -> tuple[list[dict], int]:
    p = F.params(alg)
    T = th(p)
    want = {T - 1: None, T: None, -T: None, -T - 1: None}
    near_rows, acc_rows, rej_rows = [], [], []
    c = 0
    while (any(v is None for v in want.values()) or len(near_rows) < NEAR or len(acc_rows) < PLAIN
           or len(rej_rows) < PLAIN):
        assert c < MAX_CANDIDATES, f"{alg} key {t}: search did not finish"
        mu = derive(alg, b"mu" + bytes([t]) + c.to_bytes(8, "little"), p["len_mu"])
        e = noise_of(alg, pkh, mu, i0, j0, delta)
        accept, near, decider = classify(p, e, i0)
        row = {"c": c, "mu": mu.hex(), "accept": int(accept), "noise": [int(x) for x in e[:, i0]]}
        if decider is not None and want[decider] is None:
            want[decider] = row
        elif near and len(near_rows) < NEAR:
            near_rows.append(row)
        elif not near and accept and len(acc_rows) < PLAIN:
            acc_rows.append(row)
        elif not near and not accept and len(rej_rows) < PLAIN:
            rej_rows.append(row)
        c += 1
    rows = sorted(list(want.values()) + near_rows + acc_rows + rej_rows, key=lambda r: r["c"])
    return rows, c


def rows_of(alg: str, key: dict):
    """(mu [rows, len_mu] uint8, accept bool [rows], noise int64 [rows, 8]) of one key of the fixture."""
    mu = np.stack([np.frombuffer(bytes.fromhex(r["mu"]), np.uint8) for r in key["rows"]])
    return mu, np.array([r["accept"] for r in key["rows"]], bool), np.array([r["noise"] for r in key["rows"]], np.int64)


def check(alg: str, gold: dict) -> None:
    """The conditions the fixture must meet (not tunable), from the file alone."""
    p = F.params(alg)
    T = th(p)
    assert [(k["i0"], k["j0"]) for k in gold["keys"]] == keys_of(p["n"])
    rows = [(k, r) for k in gold["keys"] for r in k["rows"]]
    assert len(rows) <= MAX_ROWS
    assert sum(r["accept"] for _, r in rows) >= 16 and sum(1 - r["accept"] for _, r in rows) >= 16
    decided = {}
    for k, r in rows:
        assert k["delta"] * M_DIV[p["n"]] == T and len(r["noise"]) == NBAR
        e = np.array(r["noise"])
        # positions outside column i0 hold E'' alone, |E''| <= 12: the accept bit is column i0's
        assert r["accept"] == int(np.all((e >= -T) & (e <= T - 1)))
        v = decided_by(p, e)
        if v is not None:
            decided.setdefault(v, []).append(r["accept"])
    assert sorted(decided) == [-T - 1, -T, T - 1, T], sorted(decided)
    assert set(decided[T - 1]) == {1} and set(decided[-T]) == {1}
    assert set(decided[T]) == {0} and set(decided[-T - 1]) == {0}


def main():
    import oracle as orc
    out = {}
    for alg in ALGS:
        p = F.params(alg)
        seed_a = derive(alg, b"seedA", 16)
        delta = th(p) // M_DIV[p["n"]]
        keys, tried = [], []
        for t, (i0, j0) in enumerate(keys_of(p["n"])):
            pk, sk = build_key(alg, seed_a, t, i0, j0, delta)
            rows, c = search_key(alg, t, sk[-p["sec"]:], i0, j0, delta)
            mu = np.stack([np.frombuffer(bytes.fromhex(r["mu"]), np.uint8) for r in rows])
            n = len(rows)
            pks, sks = (np.tile(np.frombuffer(x, np.uint8), (n, 1)) for x in (pk, sk))
            ct, ss = orc.batch_encaps(alg, pks, mu)
            ss_d = orc.batch_decaps(alg, sks, ct)
            for i, r in enumerate(rows):
                del r["c"]
                assert bool(r["accept"]) == (ss_d[i].tobytes() == ss[i].tobytes()), (alg, t, i)
                r["ct"] = hashlib.sha256(ct[i].tobytes()).hexdigest()
                r["ss"] = hashlib.sha256(ss[i].tobytes()).hexdigest()
            keys.append({"i0": i0, "j0": j0, "delta": delta, "rows": rows})
            tried.append(c)
        out[alg] = {"seedA": seed_a.hex(), "candidates_tried": tried, "keys": keys}
        check(alg, out[alg])
        acc = sum(r["accept"] for k in keys for r in k["rows"])
        tot = sum(len(k["rows"]) for k in keys)
        print(f"{alg}: tried {tried}, {tot} rows, {acc} accept, {tot - acc} reject")
    # one row per line
    sets = []
    for alg, d in out.items():
        ks = []
        for k in d["keys"]:
            rows = ",\n".join("    " + json.dumps(r, separators=(",", ":")) for r in k["rows"])
            khead = json.dumps({a: v for a, v in k.items() if a != "rows"}, separators=(",", ":"))[1:-1]
            ks.append("  {" + khead + f',"rows":[\n{rows}\n  ]}}')
        head = json.dumps({k: v for k, v in d.items() if k != "keys"}, separators=(",", ":"))[1:-1]
        sets.append(f' {json.dumps(alg)}:{{{head},"keys":[\n' + ",\n".join(ks) + "\n ]}")
    text = "{\n" + ",\n".join(sets) + "\n}\n"
    assert json.loads(text) == out
    (HERE / "frodo_edge.json").write_text(text)


if __name__ == "__main__":
    main()
