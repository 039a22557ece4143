"""Writes tests/golden/mldsa_sign.json from tests/mldsa_spec.py (deterministic; regenerates bit-identically):

    python tests/golden/make_golden_mldsa_sign.py

Signing cases for the GPU signer (csrc/mldsa_sign.hip): per parameter set one honest key (xi stored), the
deterministic variant (rnd = 32 zero bytes), and for every row the iterations Sign_internal's loop runs, why each
rejected iteration was rejected, and the SHA3-256 of the signature.  `trace` below is the spec's loop
(mldsa_spec.sign_internal, line for line) with that bookkeeping added; `test_mldsa_sign_golden.py` checks it
against spec.sign.  Reasons: "z" ||z|| >= gamma1 - beta, "r" ||LowBits(w - c s2)|| >= gamma2 - beta, "zr" both,
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

The stored file holds inputs by rule (xi, counters, lengths), not signatures; `load()` rebuilds keys and
messages, `derive(row)` recomputes a row's recorded results.  The search costs minutes when "h" is rare; checking
the stored rows costs seconds.
"""
from __future__ import annotations

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


def xi_of(name: str) -> bytes:
    return spec.H(b"qrkem mldsa_sign fixture xi " + name.encode(), 32)


def message(name: str, counter: int, length: int = None) -> bytes:
    if length is None:
        length = 32 + counter % 64
    return spec.H(name.encode() + b"-sign" + counter.to_bytes(4, "little"), length)


class Key:
    """A secret key decoded once: what every iteration of the loop reuses."""

    def __init__(self, name: str, sk: bytes):
        self.p = p = spec.PARAMS[name]
        self.sk = sk
        self.rho, self.K, self.tr, s1, s2, t0 = spec.sk_decode(p, sk)
        self.s1h, self.s2h, self.t0h = ([spec.ntt(s) for s in v] for v in (s1, s2, t0))
        self.A = spec.expand_a(p, self.rho)


def trace(key: Key, M: bytes, ctx: bytes = b"", rnd: bytes = bytes(32), cap: int = None, keep_c: bool = False):
    """(signature or None, iterations, reasons of the rejected ones[, c of the first iteration])."""
    p, Q = key.p, spec.Q
    mu = spec.H(key.tr + spec.format_message(M, ctx), 64)
    rho2 = spec.H(key.K + rnd + mu, 64)
    kappa, reasons, first_c = 0, [], None
    while cap is None or len(reasons) < cap:
        y = spec.expand_mask(p, rho2, kappa)
        kappa += p.l
        yh = [spec.ntt(v) for v in y]
        w = [spec.ntt_inv(sum(key.A[i][j] * yh[j] for j in range(p.l)) % Q) for i in range(p.k)]
        ctilde = spec.H(mu + spec.w1_encode(p, [spec.high_bits(p, wi) for wi in w]), p.ctilde)
        c = spec.sample_in_ball(p, ctilde)
        if first_c is None:
            first_c = c
        ch = spec.ntt(c)
        cs1 = [spec.ntt_inv(ch * s % Q) for s in key.s1h]
        cs2 = [spec.ntt_inv(ch * s % Q) for s in key.s2h]
        z = [(y[j] + cs1[j]) % Q for j in range(p.l)]
        r = [(w[i] - cs2[i]) % Q for i in range(p.k)]
        zbad = spec.inf_norm(z) >= p.gamma1 - p.beta
        rbad = max(int(np.max(np.abs(spec.low_bits(p, ri)))) for ri in r) >= p.gamma2 - p.beta
        if zbad or rbad:
            reasons.append(("z" if zbad else "") + ("r" if rbad else ""))
            continue
        ct0 = [spec.ntt_inv(ch * t % Q) for t in key.t0h]
        h = [spec.make_hint(p, -ct0[i], r[i] + ct0[i]) for i in range(p.k)]
        if spec.inf_norm(ct0) >= p.gamma2:
            reasons.append("t")
            continue
        if sum(int(hi.sum()) for hi in h) > p.omega:
            reasons.append("h")
            continue
        sig = spec.sig_encode(p, ctilde, [spec.mod_pm(zi, Q) for zi in z], h)
        return (sig, len(reasons) + 1, reasons) + ((first_c,) if keep_c else ())
    return (None, len(reasons), reasons) + ((first_c,) if keep_c else ())


def with_t0(name: str, sk: bytes, t0) -> bytes:
    p = spec.PARAMS[name]
    rho, K, tr, s1, s2, _ = spec.sk_decode(p, sk)
    return spec.sk_encode(p, rho, K, tr, s1, s2, t0)


def crafted_sk(name: str, honest_sk: bytes, row: dict) -> bytes:
    """The secret key of a crafted row, from the honest key and the row's own message."""
    p = spec.PARAMS[name]
    if row["kind"] == "crafted_h":
        alt = np.where(np.arange(spec.N) % 2 == 0, T0_MAX, T0_MIN)
        return with_t0(name, honest_sk, [alt] * p.k)
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


if __name__ == "__main__":
    text = json.dumps(build(), indent=0, separators=(",", ":")) + "\n"
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
