"""The plans the threaded GPU tests run (tests/test_gpu_threads.py) and the checker that judges them.  No GPU, no
torch: inputs come from fixed seeds and the fixtures under tests/golden/, expected bytes from the C oracle, from
mldsa_spec / slhdsa_spec / aead.json / RFC 5869 and Python's base64 -- never from the library under test.

plan(kind) -> one list of Step per worker thread.  A Step names what one library call (or one short chain of them)
is given and what it must return; check(step, got) compares row by row and names thread, round, step and the first
row that differs.  overlaps(log) counts the pairs of calls from different threads that were inside the library at
the same time: without it a run that happened to be serial would pass and prove nothing.

kinds
  shared   eight threads for ONE context: ML-KEM KeyGen -> Encaps -> Decaps, 4 rounds, n from MLKEM_N
  mixed    eight threads, eight families, a context each, 3 rounds
  errors   thread 0: calls that fail cleanly; threads 1, 2: good steps of `shared`
  keyed    four threads over one ML-KEM and one ML-DSA key set
"""
import base64
import dataclasses
import functools
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT / "oracle", ROOT / "oracle" / "py", ROOT / "tests" / "golden", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import oracle as orc  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
T = 8
FILL, STATUS_FILL = 0xA5, 7
MLKEM = ("ML-KEM-512", "ML-KEM-768", "ML-KEM-1024")
# keygen_pipe (host) / keygen_multi (device) up to 16, its border, the one-launch kernels up to 1024, the batched
# schedule above
MLKEM_N = (1, 16, 17, 300, 1024, 1025, 1100, 64)
SHARED_ROUNDS, MIXED_ROUNDS = 4, 3
TAMPER_THREAD = 4  # a device-pointer thread of `shared`: qrk_tamper works on device buffers
MLDSA, SLHDSA = "ML-DSA-65", "SLH-DSA-SHA2-128f"
KEYED_G = 17


@dataclasses.dataclass
class Step:
    thread: int
    round: int
    index: int
    family: str   # the label a thread of `mixed` is told apart by
    alg: str
    op: str
    n: int
    inputs: dict  # name -> ndarray or list of bytes
    want: dict    # name -> ndarray ([n, w] uint8, [n] int32) or list of bytes / ints, one entry per row
    host: bool = False  # host pointers (the *_host entry points) instead of device tensors

    def where(self) -> str:
        return f"thread {self.thread} round {self.round} step {self.index} ({self.alg} {self.op} n={self.n})"


# ------------------------------------------------------------------ the checker
def rows_of(x) -> list:
    """One comparable value per row: bytes for a byte matrix, int for a status vector, the entries of a list."""
    if isinstance(x, np.ndarray):
        if x.ndim == 1 and x.dtype != np.uint8:
            return [int(v) for v in x]
        return [r.tobytes() for r in np.atleast_2d(x)]
    return [bytes(v) if isinstance(v, (bytes, bytearray, memoryview)) else int(v) for v in x]


def _show(v) -> str:
    return v[:8].hex() + ".." if isinstance(v, bytes) and len(v) > 8 else (v.hex() if isinstance(v, bytes) else str(v))


def check(step: Step, got: dict):
    """None, or what is wrong: thread, round and step, the output and the first row that differs."""
    for key, want in step.want.items():
        if key not in got:
            return f"{step.where()}: no output {key!r}"
        w, g = rows_of(want), rows_of(got[key])
        if len(w) != len(g):
            return f"{step.where()}: {key} has {len(g)} rows, expected {len(w)}"
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                note = ""
                if isinstance(a, bytes) and a and a == bytes([FILL]) * len(a):
                    note = " (left at its prefill)"
                elif a == STATUS_FILL and not isinstance(a, bytes):
                    note = " (left at its prefill)"
                elif a in w:
                    note = f" (it is the expected row {w.index(a)})"
                return f"{step.where()}: {key} row {i} differs{note}: got {_show(a)}, expected {_show(b)}"
    return None


def overlaps(log) -> int:
    """log: (thread, enter_ns, return_ns) per call, time.monotonic_ns().  The number of pairs of calls from
    different threads whose closed intervals [enter, return] intersect."""
    ev = sorted(log, key=lambda e: e[1])
    count = 0
    for i, (ta, _, ra) in enumerate(ev):
        for tb, eb, _ in ev[i + 1:]:
            if eb > ra:
                break
            count += ta != tb
    return count


def fingerprint(plan) -> str:
    """SHA-256 over every field of every step: two builds of a plan are equal when these are."""
    h = hashlib.sha256()

    def feed(x):
        if isinstance(x, dict):
            for k in sorted(x):
                h.update(k.encode() + b"=")
                feed(x[k])
        elif isinstance(x, np.ndarray):
            h.update(str((x.dtype, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (list, tuple)):
            h.update(b"[%d" % len(x))
            for v in x:
                feed(v)
        elif isinstance(x, (bytes, bytearray)):
            h.update(b"b%d:" % len(x) + bytes(x))
        else:
            h.update(repr(x).encode() + b";")

    for steps in plan:
        h.update(b"|thread")
        for s in steps:
            feed([s.thread, s.round, s.index, s.family, s.alg, s.op, s.n, s.host, s.inputs, s.want])
    return h.hexdigest()


# ------------------------------------------------------------------ KEM steps against the C oracle
def tamper(ct: np.ndarray, seed: int, mode: int = 2) -> np.ndarray:
    """qrk_tamper as include/qrkem.h defines it: h_i = SHAKE256("qrk-tamper" || LE64(seed) || LE64(i))[0..8), bit
    (h_i >> 1) mod 8 ctlen of row i flipped; mode 1 every row, mode 2 the rows with h_i odd."""
    out = ct.copy()
    n, L = out.shape
    for i in range(n):
        h = int.from_bytes(hashlib.shake_256(b"qrk-tamper" + seed.to_bytes(8, "little") + i.to_bytes(8, "little")).digest(8),
                           "little")
        if mode == 1 or (mode == 2 and h & 1):
            bit = (h >> 1) % (8 * L)
            out[i, bit // 8] ^= 1 << (bit % 8)
    return out


@functools.lru_cache(maxsize=None)
def kem_ref(alg: str, n: int, seed: int) -> dict:
    s = orc.sizes(alg)
    kp, en = s["keypair_coins"], s["encaps_coins"]
    coins = orc.bench_coins(n, kp + en, seed=seed)
    kc, ec = np.ascontiguousarray(coins[:, :kp]), np.ascontiguousarray(coins[:, kp:])
    pk, sk = orc.batch_keypair(alg, kc, 8)
    c, ss = orc.batch_encaps(alg, pk, ec, 8)
    ss2, st2 = orc.batch_decaps(alg, sk, c, 8, with_status=True)
    assert np.array_equal(ss2, ss) and not st2.any()
    return {"kc": kc, "ec": ec, "pk": pk, "sk": sk, "ct": c, "ss": ss}


def kem_round(t, r, first, family, alg, n, seed, host, tampered=False) -> list:
    """KeyGen -> Encaps -> Decaps of one round, every input from the oracle's chain, so a wrong output of one step
    does not hide in the next.  The Decaps uses this round's own secret key."""
    ref = kem_ref(alg, n, seed)
    zeros = np.zeros(n, np.int32)
    mk = lambda i, op, inputs, want: Step(t, r, first + i, family, alg, op, n, inputs, want, host)  # noqa: E731
    steps = [mk(0, "keypair", {"coins": ref["kc"]}, {"pk": ref["pk"], "sk": ref["sk"]}),
             mk(1, "encaps", {"pk": ref["pk"], "coins": ref["ec"]}, {"ct": ref["ct"], "ss": ref["ss"], "status": zeros}),
             mk(2, "decaps", {"sk": ref["sk"], "ct": ref["ct"]}, {"ss": ref["ss"], "status": zeros})]
    if tampered:
        bad = tamper(ref["ct"], seed, 2)
        flipped = np.any(bad != ref["ct"], axis=1)
        assert 0 < flipped.sum() < n
        ss_bad, st_bad = orc.batch_decaps(alg, ref["sk"], bad, 8, with_status=True)
        assert not np.any(np.all(ss_bad[flipped] == ref["ss"][flipped], axis=1))  # the rejection keys
        assert np.array_equal(ss_bad[~flipped], ref["ss"][~flipped])
        steps.append(mk(3, "decaps_tampered", {"sk": ref["sk"], "ct": ref["ct"], "seed": seed},
                        {"ct_tampered": bad, "ss": ss_bad, "status": st_bad}))
    return steps


def shared_alg(t: int) -> str:
    """All three parameter sets at the small n; ML-KEM-768 alone at the two largest."""
    return "ML-KEM-768" if MLKEM_N[t] > 1024 else MLKEM[t % 3]


def shared_thread(t: int, rounds: int = SHARED_ROUNDS) -> list:
    steps = []
    for r in range(rounds):
        steps += kem_round(t, r, len(steps), shared_alg(t), shared_alg(t), MLKEM_N[t], 0x7EAD0000 + 64 * t + r,
                           host=t % 2 == 1, tampered=t == TAMPER_THREAD)
    return steps


# ------------------------------------------------------------------ the other families, against what they are compared with today
@functools.lru_cache(maxsize=None)
def mldsa_sets():
    import make_golden_mldsa as gold
    import make_golden_mldsa_sign as sgold
    f, s = gold.load()[MLDSA], sgold.load()[MLDSA]
    rows = [(f["pk"], m, sg) for m, sg in zip(f["msgs"], f["sigs"])]
    rows += [gold.apply_tamper(e, f["pk"], f["msgs"], f["sigs"]) for e in f["tampers"]]
    status = [0] * len(f["msgs"]) + [-1] * len(f["tampers"])
    sign_rows = [r for r in s["rows"] if r["ctx_len"] == 0]
    return s, rows, status, sign_rows


def rotate(xs, r):
    r %= len(xs)
    return list(xs[r:]) + list(xs[:r])


def sha3_rows(rows) -> list:
    return [hashlib.sha3_256(bytes(x)).digest() for x in rows]


def mldsa_thread(t: int, rounds: int) -> list:
    s, vrows, vstatus, srows = mldsa_sets()
    steps = []
    for r in range(rounds):
        mk = lambda op, n, inputs, want: Step(t, r, len(steps), MLDSA, MLDSA, op, n, inputs, want)  # noqa: E731
        steps.append(mk("sig_keygen", 2, {"xi": [s["xi"]] * 2}, {"pk": [s["pk"]] * 2, "sk": [s["sk"]] * 2}))
        part = rotate(srows, r)
        steps.append(mk("sig_sign", len(part), {"sk": [x["sk"] for x in part], "msg": [x["msg"] for x in part]},
                        {"sig_sha3": [bytes.fromhex(x["sig_sha3"]) for x in part], "status": [0] * len(part)}))
        rows, status = rotate(vrows, 5 * r), rotate(vstatus, 5 * r)
        steps.append(mk("sig_verify", len(rows), {"pk": [x[0] for x in rows], "msg": [x[1] for x in rows],
                                                  "sig": [x[2] for x in rows]}, {"status": status}))
    return steps


@functools.lru_cache(maxsize=None)
def slhdsa_rows():
    import make_golden_slhdsa as gold
    import slhdsa_spec as spec
    from test_slhdsa_spec import tampers
    f = gold.load()[SLHDSA]
    sigs = gold.signatures(SLHDSA, f)  # the spec's signatures, checked against the stored SHA3-256
    rows = [(f["pk"], m, s) for m, s in zip(f["msgs"], sigs)]
    rows += [c[1:4] for c in tampers(spec.PARAMS[SLHDSA], f["pk"], f["msgs"][1], sigs[1])]
    return rows, [0] * len(sigs) + [-1] * (len(rows) - len(sigs))


def slhdsa_thread(t: int, rounds: int) -> list:
    rows, status = slhdsa_rows()
    out = []
    for r in range(rounds):
        rr, st = rotate(rows, 2 * r), rotate(status, 2 * r)
        out.append(Step(t, r, len(out), SLHDSA, SLHDSA, "sig_verify", len(rr),
                        {"pk": [x[0] for x in rr], "msg": [x[1] for x in rr], "sig": [x[2] for x in rr]}, {"status": st}))
    return out


def symmetric_thread(t: int, rounds: int) -> list:
    from test_handshake_oracle import RFC5869
    records = json.loads((GOLDEN / "aead.json").read_text())["records"]
    out = []
    for r in range(rounds):
        for alg in sorted(records):
            recs = rotate(records[alg], 7 * r)
            f = lambda k: [bytes.fromhex(x[k]) for x in recs]  # noqa: E731
            keys, nonces, pts, aads, sealed = f("key"), f("nonce"), f("pt"), f("aad"), f("sealed")
            mk = lambda op, inputs, want: Step(t, r, len(out), "AEAD+HKDF", alg, op, len(recs), inputs, want)  # noqa: E731
            out.append(mk("aead_seal", {"key": keys, "nonce": nonces, "pt": pts, "aad": aads}, {"sealed": sealed}))
            # every third row with its last tag bit flipped: refused, and its plaintext span zeroed
            bad = [s[:-1] + bytes([s[-1] ^ 1]) if i % 3 == 2 else s for i, s in enumerate(sealed)]
            out.append(mk("aead_open", {"key": keys, "sealed": bad, "aad": aads},
                          {"pt": [bytes(len(p)) if i % 3 == 2 else p for i, p in enumerate(pts)],
                           "status": [-1 if i % 3 == 2 else 0 for i in range(len(recs))]}))
        for ikm, salt, info, L, _prk, okm in RFC5869:
            out.append(Step(t, r, len(out), "AEAD+HKDF", "HKDF-SHA256", "hkdf", 1,
                            {"ikm": [ikm], "salt": salt, "info": info, "L": L}, {"okm": [bytes.fromhex(okm)]}))
    return out


def wire_thread(t: int, rounds: int) -> list:
    out = []
    for r in range(rounds):
        for n, L in ((65, 1184), (3, 1), (17, 800), (33, 1088)):  # L mod 3 = 2, 1, 2, 2; then 0:
            for length in (L, L + 1 if (L + 1) % 3 == 0 else L + 2):
                raw = orc.bench_coins(n, (length + 7) // 8 * 8, seed=0xB64 + 97 * r + length)[:, :length]
                raw = np.ascontiguousarray(raw)
                text = np.stack([np.frombuffer(base64.b64encode(x.tobytes()), np.uint8) for x in raw])
                out.append(Step(t, r, len(out), "base64", "base64", "b64_encode", n, {"raw": raw}, {"text": text}))
                out.append(Step(t, r, len(out), "base64", "base64", "b64_decode", n, {"text": text, "L": length},
                                {"raw": raw, "status": np.zeros(n, np.int32)}))
    return out


def mixed_plan(rounds: int = MIXED_ROUNDS) -> list:
    kems = [("ML-KEM-512", 300), ("ML-KEM-1024", 1100), ("HQC-128", 64), ("FrodoKEM-640-SHAKE", 8)]
    plan = []
    for t, (alg, n) in enumerate(kems):
        steps = []
        for r in range(rounds):
            steps += kem_round(t, r, len(steps), alg, alg, n, 0x3C1D0000 + 64 * t + r, host=False)
        plan.append(steps)
    plan += [mldsa_thread(4, rounds), slhdsa_thread(5, rounds), symmetric_thread(6, rounds), wire_thread(7, rounds)]
    return plan


# ------------------------------------------------------------------ clean failures (thread 0 of `errors`)
UNKNOWN_KEM, UNKNOWN_SIG = "ML-KEM-999", "ML-DSA-99"
ERR_KEM = "unsupported KEM: " + UNKNOWN_KEM
ERR_SIG = "unsupported signature algorithm: " + UNKNOWN_SIG


def error_thread(t: int, rounds: int) -> list:
    """Five kinds of clean failure in turn.  want["rc"] is the ABI call's return value; want["error"] the text
    qrk_last_error() must hold afterwards IN THIS THREAD: a call that returns -1 sets it, a call that reports through
    status (rc 0) or fails in the Python wrapper leaves the thread's previous text."""
    import mldsa_spec
    ref = kem_ref("ML-KEM-768", 2, 0xE44)
    pk = ref["pk"].copy()
    pk[1, 0], pk[1, 1] = 3329 & 0xFF, (pk[1, 1] & 0xF0) | (3329 >> 8)  # the first 12-bit field of row 1 is q
    s, _, _, srows = mldsa_sets()
    p = mldsa_spec.PARAMS[MLDSA]
    bad_sk = bytearray(s["sk"])
    ebits = (2 * p.eta).bit_length()
    bad_sk[128] = (bad_sk[128] & ~((1 << ebits) - 1)) | (2 * p.eta + 1)  # s1[0][0] = eta - (2 eta + 1) = -eta - 1
    assert int(mldsa_spec.sk_decode(p, bytes(bad_sk))[3][0][0]) == -p.eta - 1
    honest = next(x for x in srows if x["kind"] == "honest")
    key = bytes(range(32))
    out, last = [], ""
    for r in range(rounds):
        mk = lambda alg, op, n, inputs, want: Step(t, r, len(out), "errors", alg, op, n, inputs, want)  # noqa: E731
        last = ERR_KEM
        out.append(mk(UNKNOWN_KEM, "fail_unknown_kem", 1, {}, {"rc": [-1], "error": [last.encode()]}))
        out.append(mk("ML-KEM-768", "fail_wrong_width", 2, {"pk": ref["pk"][:, :-1]},
                      {"raised": [b"ValueError"], "error": [last.encode()]}))
        out.append(mk("ML-KEM-768", "encaps", 2, {"pk": pk, "coins": ref["ec"]},
                      {"rc": [0], "status": [0, -1], "ct0": [ref["ct"][0].tobytes()], "error": [last.encode()]}))
        last = ERR_SIG
        out.append(mk(UNKNOWN_SIG, "fail_unknown_sig", 1, {}, {"rc": [-1], "error": [last.encode()]}))
        out.append(mk("AES-256-GCM", "aead_open", 1, {"key": [key], "sealed": [bytes(27)], "aad": [b""]},
                      {"status": [-1], "error": [last.encode()]}))
        out.append(mk(MLDSA, "sig_sign", 2, {"sk": [bytes(bad_sk), honest["sk"]], "msg": [honest["msg"]] * 2},
                      {"sig_sha3": [hashlib.sha3_256(bytes(p.sig)).digest(), bytes.fromhex(honest["sig_sha3"])],
                       "status": [-1, 0], "error": [last.encode()]}))
    return out


ERROR_TEXTS = (ERR_KEM, ERR_SIG)


# ------------------------------------------------------------------ key sets
def keyed_patterns(g: int, n: int, t: int) -> np.ndarray:
    i = np.arange(n, dtype=np.uint32)
    return [i % g, (g - 1 - i % g).astype(np.uint32),
            np.random.default_rng(0xC0FFEE + n).integers(0, g, n, dtype=np.uint32),
            np.where(i % 2 == 0, 0, g - 1).astype(np.uint32)][t % 4]


@functools.lru_cache(maxsize=None)
def keyed_keys(alg: str = "ML-KEM-768"):
    import mlkem_keyed_cases as cases
    seeds = np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in cases.load_fixture()["seeds"][:KEYED_G]])
    return orc.batch_keypair(alg, seeds, 8)


def keyed_plan(rounds: int = 3, alg: str = "ML-KEM-768") -> list:
    """Per thread and round: keyed Encaps and Decaps (every odd row's ciphertext flipped) under 17 ML-KEM keys, and
    keyed deterministic signing of the mldsa_sign.json rows under the set of their distinct secret keys; each thread
    with its own row count and index pattern.  inputs["set"] holds the keys the set is loaded from."""
    pk, sk = keyed_keys(alg)
    _, _, _, srows = mldsa_sets()
    sks = sorted({x["sk"] for x in srows})
    plan = []
    for t in range(4):
        steps, n = [], (65, 33, 130, 17)[t]
        index = keyed_patterns(KEYED_G, n, t)
        for r in range(rounds):
            coins = orc.bench_coins(n, 32, seed=0x6E7ED + 16 * t + r)
            c, ss = orc.batch_encaps(alg, pk[index], coins, 8)
            bad = c.copy()
            bad[1::2, (7 * t + r) % c.shape[1]] ^= 0x20
            ss_bad = orc.batch_decaps(alg, sk[index], bad, 8)
            zeros = np.zeros(n, np.int32)
            mk = lambda a, op, m, inputs, want: Step(t, r, len(steps), "keyed", a, op, m, inputs, want)  # noqa: E731
            steps.append(mk(alg, "encaps_keyed", n, {"index": index, "coins": coins}, {"ct": c, "ss": ss, "status": zeros}))
            steps.append(mk(alg, "decaps_keyed", n, {"index": index, "ct": bad}, {"ss": ss_bad, "status": zeros}))
            part = rotate(srows, 3 * t + r)[:len(srows) - t]
            steps.append(mk(MLDSA, "sign_keyed", len(part),
                            {"index": [sks.index(x["sk"]) for x in part], "msg": [x["msg"] for x in part]},
                            {"sig_sha3": [bytes.fromhex(x["sig_sha3"]) for x in part], "status": [0] * len(part)}))
        plan.append(steps)
    return plan


def keyed_sets(alg: str = "ML-KEM-768") -> dict:
    pk, sk = keyed_keys(alg)
    _, _, _, srows = mldsa_sets()
    return {"mlkem_pk": pk, "mlkem_sk": sk, "mldsa_sk": sorted({x["sk"] for x in srows})}


# ------------------------------------------------------------------ plans
def plan(kind: str) -> list:
    if kind == "shared":
        return [shared_thread(t) for t in range(T)]
    if kind == "mixed":
        return mixed_plan()
    if kind == "errors":
        # B: the host-pointer steps of thread 3 of `shared` (n = 300); C: the device-pointer ones of thread 2 (n = 17)
        b, c = shared_thread(3, 3), shared_thread(2, 3)
        for i, steps in ((1, b), (2, c)):
            for s in steps:
                s.thread = i
        return [error_thread(0, 6), b, c]
    if kind == "keyed":
        return keyed_plan()
    raise ValueError(kind)
