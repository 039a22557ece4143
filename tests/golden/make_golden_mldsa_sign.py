"""Writes tests/golden/mldsa_sign.json from tests/mldsa_spec.py (deterministic; regenerates bit-identically):

    python tests/golden/make_golden_mldsa_sign.py

Signing cases for the GPU signer (csrc/mldsa_sign.hip): per parameter set one honest key (xi stored), the
deterministic variant (rnd = 32 zero bytes), and for every row the iterations Sign_internal's loop runs, why each
rejected iteration was rejected, and the SHA3-256 of the signature.  `trace` below is the spec's loop
(mldsa_spec.sign_internal; `step` and `hint_of` are its lines in its order) with that bookkeeping added;
`test_mldsa_sign_golden.py` checks it against spec.sign.  Reasons: "z" ||z|| >= gamma1 - beta, "r" ||LowBits(w - c s2)|| >= gamma2 - beta, "zr" both,
then "t" ||c t0|| >= gamma2, else "h" more than omega hints.

Rows per set:
  fixed     message lengths 0 and 1; 69, 70, 71 (the mu absorb 64 + 2 + |ctx| + |M| at 135, 136, 137 bytes, around
            the SHAKE256 rate); lengths 0 and 33 under a context string of 255 bytes
  searched  messages message(name, counter), counter = 0, 1, ... (length 32 + counter % 64): the first with one
            iteration, the first with at least ten, and the first whose reasons add "z", "r", "zr" and "h" to
            what the rows so far cover.  The search for "h" gives up after H_BUDGET spec iterations.
  crafted   keys that are not KeyGen outputs (marked; their signatures need not verify, byte parity is what they
            pin).  "t" (ML-DSA-44 only: tau 2^12 is below gamma2 for the other two, so the branch cannot be
            reached there): the honest key with t0 replaced so that coefficient 255 of c t0_0 in the first
            iteration of a row that passes z / r there is the sum of tau terms of 2^12 or 2^12 - 1 (-2^12 has no
            encoding), at least tau (2^12 - 1) = 159 705 >= gamma2 = 95 232.  "h", only where the search found no
            honest row: t0 = 2^12 and -(2^12 - 1) alternating, so that c t0 moves many high bits (c does not
            depend on t0).
  edge      pairs of crafted keys that pin where each of the four checks flips (`edge_pairs`).  Both rows of a pair
            sign the same message, searched from counter EDGE_FROM on among those whose first iteration passes
            under the honest key.  The first iteration of the at-threshold row fails that one check, with the
            bounded quantity exactly on the threshold; that of its twin ("twin": true) is one inside and passes all
            four, so the twin takes one iteration.  y, w and c of the first iteration do not depend on s1, s2 or
            t0, so one of those is edited (`edge_sk`, `spread`; every entry stays in its encodable range):
              edge_z  s1_j sparse, so that z_j[e] = y_j[e] + (c s1_j)[e] is "value": +-(gamma1 - beta), twin
                      +-(gamma1 - beta - 1).  The keys of a pair differ by one unit in one coefficient.
              edge_r  s2_i sparse, so that LowBits(w_i - c s2_i)[e] is +-(gamma2 - beta), twin one less.  Likewise.
              edge_t  ML-DSA-44 only: t0_0 sparse, (c t0_0)[255] = +-gamma2, twin +-(gamma2 - 1); the other
                      polynomials of t0 zero.  Likewise.
              edge_h  t0 = +a, -a, ... in its first m coefficients and zero after (a = 2000 for ML-DSA-44, to keep
                      ||c t0|| under gamma2, 2^12 - 1 otherwise): omega + 1 hints, twin (a smaller m) exactly omega,
                      so its hint bytes fill the index area up to the first count byte.  The count is close to
                      monotone in m: m is bisected to a crossing and EDGE_H_WINDOW values either side are scanned.
            Both signs of the signed quantities: 2 pairs each of edge_z and edge_r, 2 of edge_t for ML-DSA-44, 1 of
            edge_h.

The stored file holds inputs by rule (xi, counters, lengths, and for an edge row the integers of its rule), not keys
or signatures; `load()` rebuilds keys and messages, `derive(row)` recomputes a row's recorded results.  The search
costs minutes when "h" is rare; checking the stored rows costs seconds.  The edge search adds little:
test_fixture_regenerates_identically took 6.8 s before the edge rows and 9.0 s with them (one CPU core).
"""
from __future__ import annotations

import functools
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import mldsa_spec as spec  # noqa: E402

OUT = HERE / "mldsa_sign.json"
NAMES = ("ML-DSA-44", "ML-DSA-65", "ML-DSA-87")
CTX255 = bytes(range(255))
SEARCH_ROWS = 400
H_BUDGET = 20000
T0_MAX, T0_MIN = 1 << 12, -((1 << 12) - 1)
EDGE_KINDS = ("edge_z", "edge_r", "edge_t", "edge_h")
EDGE_QUANTITY = {"z": "z", "r": "r0", "t": "ct0"}  # the attribute of First a check bounds
EDGE_FROM = 3000                                   # the first message counter the threshold pairs are searched from
EDGE_H_AMPLITUDE = {"ML-DSA-44": 2000}             # keeps ||c t0|| under gamma2 there; 2^12 - 1 for the other two
EDGE_H_WINDOW = 32                                 # values of m scanned on either side of the crossing


def xi_of(name: str) -> bytes:
    return spec.H(b"qrkem mldsa_sign fixture xi " + name.encode(), 32)


def message(name: str, counter: int, length: int = None) -> bytes:
    if length is None:
        length = 32 + counter % 64
    return spec.H(name.encode() + b"-sign" + counter.to_bytes(4, "little"), length)


class Key:
    """A secret key decoded once: what every iteration of the loop reuses."""

    def __init__(self, name: str, sk: bytes, A=None):
        self.p = p = spec.PARAMS[name]
        self.sk = sk
        self.rho, self.K, self.tr, s1, s2, t0 = spec.sk_decode(p, sk)
        self.s1h, self.s2h, self.t0h = ([spec.ntt(s) for s in v] for v in (s1, s2, t0))
        self.A = A if A is not None else spec.expand_a(p, self.rho)  # A: that of another key with this rho


def prologue(key: Key, M: bytes, ctx: bytes = b"", rnd: bytes = bytes(32)):
    """mu and rho'' (Algorithm 7, lines 6 and 7)."""
    mu = spec.H(key.tr + spec.format_message(M, ctx), 64)
    return mu, spec.H(key.K + rnd + mu, 64)


def step(key: Key, mu: bytes, rho2: bytes, kappa: int):
    """Lines 11 to 21 of the iteration that starts at kappa: (y, w, c~, c, c_hat, z, r), before any check."""
    p, Q = key.p, spec.Q
    y = spec.expand_mask(p, rho2, kappa)
    yh = [spec.ntt(v) for v in y]
    w = [spec.ntt_inv(sum(key.A[i][j] * yh[j] for j in range(p.l)) % Q) for i in range(p.k)]
    ctilde = spec.H(mu + spec.w1_encode(p, [spec.high_bits(p, wi) for wi in w]), p.ctilde)
    c = spec.sample_in_ball(p, ctilde)
    ch = spec.ntt(c)
    cs1 = [spec.ntt_inv(ch * s % Q) for s in key.s1h]
    cs2 = [spec.ntt_inv(ch * s % Q) for s in key.s2h]
    z = [(y[j] + cs1[j]) % Q for j in range(p.l)]
    r = [(w[i] - cs2[i]) % Q for i in range(p.k)]
    return y, w, ctilde, c, ch, z, r


def hint_of(p, ch, r, t0h):
    """(c t0, h) for the NTT'd t0 given: lines 25 and 26."""
    ct0 = [spec.ntt_inv(ch * t % spec.Q) for t in t0h]
    return ct0, [spec.make_hint(p, -ct0[i], r[i] + ct0[i]) for i in range(p.k)]


CHECKS = ("z", "r", "t", "h")


def limits(p) -> dict:
    """Per check the smallest value that rejects: ||z||, ||LowBits(w - c s2)||, ||c t0||, the number of hints."""
    return {"z": p.gamma1 - p.beta, "r": p.gamma2 - p.beta, "t": p.gamma2, "h": p.omega + 1}


def trace(key: Key, M: bytes, ctx: bytes = b"", rnd: bytes = bytes(32), cap: int = None, keep_c: bool = False,
          off: dict = None):
    """(signature or None, iterations, reasons of the rejected ones[, c of the first iteration]).  `off` moves the
    right-hand side of a check ("z", "r", "t", "h") by that much: the off-by-one signers the fixture must tell
    from the spec's (test_mldsa_sign_golden.py); nothing else passes it."""
    p, Q = key.p, spec.Q
    lim = {x: v + (off or {}).get(x, 0) for x, v in limits(p).items()}
    mu, rho2 = prologue(key, M, ctx, rnd)
    kappa, reasons, first_c = 0, [], None
    while cap is None or len(reasons) < cap:
        y, w, ctilde, c, ch, z, r = step(key, mu, rho2, kappa)
        kappa += p.l
        if first_c is None:
            first_c = c
        zbad = spec.inf_norm(z) >= lim["z"]
        rbad = max(int(np.max(np.abs(spec.low_bits(p, ri)))) for ri in r) >= lim["r"]
        if zbad or rbad:
            reasons.append(("z" if zbad else "") + ("r" if rbad else ""))
            continue
        ct0, h = hint_of(p, ch, r, key.t0h)
        if spec.inf_norm(ct0) >= lim["t"]:
            reasons.append("t")
            continue
        if sum(int(hi.sum()) for hi in h) >= lim["h"]:
            reasons.append("h")
            continue
        sig = spec.sig_encode(p, ctilde, [spec.mod_pm(zi, Q) for zi in z], h)
        return (sig, len(reasons) + 1, reasons) + ((first_c,) if keep_c else ())
    return (None, len(reasons), reasons) + ((first_c,) if keep_c else ())


class First:
    """The first iteration in full, whatever its checks decide: y, LowBits(w) and c (which depend on rho, K, tr and
    the message alone), the centred z, LowBits(w - c s2) and c t0, and per check the quantity it bounds."""

    def __init__(self, key: Key, M: bytes):
        p, Q = key.p, spec.Q
        self.y, w, _, self.c, self.ch, z, self.r = step(key, *prologue(key, M), 0)
        self.w0 = [spec.low_bits(p, wi) for wi in w]
        self.z = [spec.mod_pm(zi, Q) for zi in z]
        self.r0 = [spec.low_bits(p, ri) for ri in self.r]
        ct0, h = hint_of(p, self.ch, self.r, key.t0h)
        self.ct0 = [spec.mod_pm(t, Q) for t in ct0]
        self.norms = {"z": spec.inf_norm(z), "r": max(int(np.max(np.abs(v))) for v in self.r0),
                      "t": spec.inf_norm(ct0), "h": sum(int(hi.sum()) for hi in h)}
        self.fails = [x for x in CHECKS if self.norms[x] >= limits(p)[x]]


def with_t0(name: str, sk: bytes, t0) -> bytes:
    p = spec.PARAMS[name]
    rho, K, tr, s1, s2, _ = spec.sk_decode(p, sk)
    return spec.sk_encode(p, rho, K, tr, s1, s2, t0)


@functools.lru_cache(maxsize=None)
def honest_key(name: str, sk: bytes) -> Key:
    return Key(name, sk)


def spread(c, e: int, total: int, cap: int) -> np.ndarray:
    """The sparse polynomial s with (c s)_e = total: for every c_i != 0 an entry at (e - i) mod 256 with the sign of
    c_i (negated where e < i: X^256 = -1) times the sign of total.  The magnitudes are |total| / tau, rounded up in
    the first |total| mod tau entries and down in the others, so total and total -+ 1 give polynomials that differ
    by one unit in one coefficient.  None may exceed cap."""
    at = np.nonzero(c)[0]
    low, ups = divmod(abs(total), len(at))
    assert low + (ups > 0) <= cap, (total, cap)
    s = np.zeros(spec.N, dtype=np.int64)
    for n, i in enumerate(at):
        s[(e - i) % spec.N] = int(np.sign(total)) * int(c[i]) * (1 if e >= i else -1) * (low + (n < ups))
    return s


def alternating(p, m: int, a: int) -> list:
    """t0 as +a, -a, +a, ... in its first m coefficients (polynomial after polynomial) and zero in the others."""
    e = np.arange(p.k * spec.N)
    return list((np.where(e % 2 == 0, a, -a) * (e < m)).reshape(p.k, spec.N))


def edge_sk(name: str, honest_sk: bytes, row: dict) -> bytes:
    """The key of a threshold row: the honest key with one secret vector edited.  y, w and c of the first iteration
    depend on rho, K, tr and the message alone, so they are the honest key's; "value" is what coefficient "coef" of
    polynomial "poly" of z, of LowBits(w - c s2) or of c t0 becomes in that iteration."""
    p = spec.PARAMS[name]
    rho, K, tr, s1, s2, t0 = spec.sk_decode(p, honest_sk)
    if row["kind"] == "edge_h":
        t0 = alternating(p, row["m"], row["a"])
    else:
        f = First(honest_key(name, honest_sk), row_message(name, row))
        j, e, v = row["poly"], row["coef"], row["value"]
        if row["kind"] == "edge_z":
            s1[j] = spread(f.c, e, v - int(f.y[j][e]), p.eta)
        elif row["kind"] == "edge_r":  # w0 - (c s2)_e stays inside (-gamma2, gamma2]: the high bits do not move
            s2[j] = spread(f.c, e, int(f.w0[j][e]) - v, p.eta)
        else:
            t0 = [np.zeros(spec.N, dtype=np.int64)] * p.k
            t0[j] = spread(f.c, e, v, -T0_MIN)
    return spec.sk_encode(p, rho, K, tr, s1, s2, t0)


def edge_rules(name: str, f: First, check: str, sign: int):
    """Candidate (at-threshold, twin) rules for a message whose first iteration under the honest key is f."""
    p = spec.PARAMS[name]
    lim = limits(p)[check]
    if check in ("z", "r"):  # a coefficient that an edit of at most beta - 1 puts on the threshold
        near = f.y if check == "z" else f.w0
        for j, v in enumerate(near):
            for e in np.nonzero(np.abs(sign * lim - v) <= p.beta - 1)[0]:
                yield tuple({"poly": j, "coef": int(e), "value": sign * x} for x in (lim, lim - 1))
    elif check == "t":  # coefficient 255: no wrap-around term, as for crafted_t
        yield tuple({"poly": 0, "coef": spec.N - 1, "value": sign * x} for x in (lim, lim - 1))
    else:
        a = EDGE_H_AMPLITUDE.get(name, -T0_MIN)

        def hints(m):
            ct0, h = hint_of(p, f.ch, f.r, [spec.ntt(t) for t in alternating(p, m, a)])
            return sum(int(hi.sum()) for hi in h) if spec.inf_norm(ct0) < p.gamma2 else -1

        lo, hi = 0, p.k * spec.N  # no hints at m = 0; the count is close to monotone in m: bisect to a crossing
        if hints(hi) <= p.omega:
            return
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if hints(mid) > p.omega else (mid, hi)
        got = {m: hints(m) for m in range(max(hi - EDGE_H_WINDOW, 0), min(hi + EDGE_H_WINDOW, p.k * spec.N) + 1)}
        for m_at in (m for m, n in got.items() if n == lim):
            for m_twin in (m for m, n in reversed(got.items()) if m < m_at and n == lim - 1):
                yield {"m": m_at, "a": a}, {"m": m_twin, "a": a}


def edge_first(name: str, sk: bytes, row: dict) -> First:
    return First(Key(name, edge_sk(name, sk, row), honest_key(name, sk).A), row_message(name, row))


def edge_pairs(name: str, sk: bytes) -> list:
    """The threshold pairs of a set, [(at-threshold row, twin)] without their recorded results: per check and sign
    the first message from EDGE_FROM on that passes under the honest key and has a rule under which the first
    iteration of the at-threshold row fails that check alone, with the bounded quantity on the threshold, and that
    of the twin passes all four, with it one below."""
    p = spec.PARAMS[name]
    pairs = []
    for check in CHECKS:
        if check == "t" and p.tau << 12 < p.gamma2:
            continue
        for sign in (1, -1) if check != "h" else (1,):
            for counter in range(EDGE_FROM, EDGE_FROM + 200):
                base = {"kind": "edge_" + check, "serves": [check], "counter": counter, "len": 32 + counter % 64,
                        "ctx_len": 0}
                f = First(honest_key(name, sk), row_message(name, base))
                if f.fails:
                    continue
                for rules in edge_rules(name, f, check, sign):
                    at, twin = (dict(base, twin=t, **rule) for t, rule in zip((False, True), rules))
                    if edge_pair_holds(name, sk, at, twin):
                        break
                else:
                    continue
                pairs.append((at, twin))
                break
            else:
                raise AssertionError((name, check, sign))
    return pairs


def edge_pair_holds(name: str, sk: bytes, at: dict, twin: dict) -> bool:
    check = at["serves"][0]
    lim = limits(spec.PARAMS[name])[check]
    fa, ft = edge_first(name, sk, at), edge_first(name, sk, twin)
    if check != "h":  # the signed value, where the rule says it is
        for f, row in ((fa, at), (ft, twin)):
            if int(getattr(f, EDGE_QUANTITY[check])[row["poly"]][row["coef"]]) != row["value"]:
                return False
    return fa.fails == [check] and fa.norms[check] == lim and ft.fails == [] and ft.norms[check] == lim - 1


def crafted_sk(name: str, honest_sk: bytes, row: dict) -> bytes:
    """The secret key of a crafted row, from the honest key and the row's own message."""
    p = spec.PARAMS[name]
    if row["kind"] == "crafted_h":
        alt = np.where(np.arange(spec.N) % 2 == 0, T0_MAX, T0_MIN)
        return with_t0(name, honest_sk, [alt] * p.k)
    if row["kind"] in EDGE_KINDS:
        return edge_sk(name, honest_sk, row)
    assert row["kind"] == "crafted_t"
    c = trace(Key(name, honest_sk), row_message(name, row), cap=1, keep_c=True)[3]
    t = np.zeros(spec.N, dtype=np.int64)
    for i in np.nonzero(c)[0]:
        t[255 - i] = T0_MAX if c[i] > 0 else T0_MIN  # (c t0)_255 = sum_i c_i t0_(255 - i): no wrap-around term
    return with_t0(name, honest_sk, [t] + [np.zeros(spec.N, dtype=np.int64)] * (p.k - 1))


def row_message(name: str, row: dict) -> bytes:
    return message(name, row["counter"], row["len"])


def derive(name: str, key: Key, row: dict) -> dict:
    """The recorded results of a row, recomputed."""
    sig, iters, reasons = trace(key, row_message(name, row), CTX255[:row["ctx_len"]])
    return {"iters": iters, "reasons": reasons, "sig_sha3": hashlib.sha3_256(sig).hexdigest(),
            "sk_sha3": hashlib.sha3_256(key.sk).hexdigest()}


def search(name: str, key: Key, have: set) -> list:
    """The searched rows: [(counter, tag)], tags as in the module docstring."""
    found, need = [], ["one", "ten", "z", "r", "zr", "h"]
    need = [t for t in need if t not in have]
    spent = 0
    for counter in range(1 << 20):
        if not need or (need == ["h"] and spent >= H_BUDGET) or (need != ["h"] and counter >= SEARCH_ROWS):
            break
        _, iters, reasons = trace(key, message(name, counter))
        spent += iters
        hit = [t for t in need if (t == "one" and iters == 1) or (t == "ten" and iters >= 10) or t in reasons]
        if hit:
            found.append((counter, hit))
            need = [t for t in need if t not in hit]
    assert need in ([], ["h"]), (name, need)
    return found


def build() -> dict:
    doc = {"note": "tests/golden/make_golden_mldsa_sign.py; spec signatures, rnd = 32 zero bytes, message(name, "
                   "counter, len) under the key of xi; ctx = bytes(range(ctx_len))", "sets": {}}
    for name in NAMES:
        p = spec.PARAMS[name]
        pk, sk = spec.keygen_internal(xi_of(name), name)
        key = Key(name, sk)
        rows = [{"kind": "honest", "serves": ["len"], "counter": 1000 + i, "len": ln, "ctx_len": cl}
                for i, (ln, cl) in enumerate([(0, 0), (1, 0), (69, 0), (70, 0), (71, 0), (0, 255), (33, 255)])]
        for row in rows:
            row.update(derive(name, key, row))
        have = {r for row in rows for r in row["reasons"]}
        have |= {"one"} if any(row["iters"] == 1 for row in rows) else set()
        have |= {"ten"} if any(row["iters"] >= 10 for row in rows) else set()
        for counter, tags in search(name, key, have):
            row = {"kind": "honest", "serves": tags, "counter": counter, "len": 32 + counter % 64, "ctx_len": 0}
            row.update(derive(name, key, row))
            rows.append(row)
        for row in rows:  # honest signatures verify
            sig = trace(key, row_message(name, row), CTX255[:row["ctx_len"]])[0]
            assert spec.verify(pk, row_message(name, row), sig, CTX255[:row["ctx_len"]])
        crafted = []
        if name == "ML-DSA-44":
            crafted.append("crafted_t")
        if not any("h" in row["reasons"] for row in rows):
            crafted.append("crafted_h")
        for kind in crafted:
            want = "t" if kind == "crafted_t" else "h"
            for counter in range(2000, 2400):
                row = {"kind": kind, "serves": [want], "counter": counter, "len": 32 + counter % 64, "ctx_len": 0}
                first = trace(key, row_message(name, row), cap=1)[2]
                if first and kind == "crafted_t":  # the source row's first iteration must pass z / r
                    continue
                got = derive(name, Key(name, crafted_sk(name, sk, row)), row)
                if want in got["reasons"]:
                    row.update(got)
                    rows.append(row)
                    break
            else:
                raise AssertionError((name, kind))
        for pair in edge_pairs(name, sk):
            for row in pair:
                row.update(derive(name, Key(name, edge_sk(name, sk, row), key.A), row))
                rows.append(row)
            assert pair[0]["reasons"][0] == pair[0]["serves"][0] and pair[1]["iters"] == 1, pair
        doc["sets"][name] = {"xi": xi_of(name).hex(), "pk_sha3": hashlib.sha3_256(pk).hexdigest(), "rows": rows}
    return doc


def load(path: Path = OUT) -> dict:
    """name -> {"pk", "sk", "rows"}; every row also carries its "msg", "ctx" and the "sk" it is signed with."""
    doc = json.loads(path.read_text())
    out = {}
    for name, s in doc["sets"].items():
        pk, sk = spec.keygen_internal(bytes.fromhex(s["xi"]), name)
        rows = []
        for row in s["rows"]:
            rsk = sk if row["kind"] == "honest" else crafted_sk(name, sk, row)
            rows.append(dict(row, msg=row_message(name, row), ctx=CTX255[:row["ctx_len"]], sk=rsk))
        out[name] = {"xi": bytes.fromhex(s["xi"]), "pk": pk, "sk": sk, "pk_sha3": s["pk_sha3"], "rows": rows}
    return out


def stored_pairs(rows: list) -> list:
    """[(at-threshold row, twin)] of a set's rows, in the order build() stores them."""
    edge = [r for r in rows if r["kind"] in EDGE_KINDS]
    pairs = list(zip(edge[0::2], edge[1::2]))
    assert len(edge) % 2 == 0 and all(not a["twin"] and t["twin"] and a["kind"] == t["kind"] for a, t in pairs)
    return pairs


if __name__ == "__main__":
    text = json.dumps(build(), indent=0, separators=(",", ":")) + "\n"
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
