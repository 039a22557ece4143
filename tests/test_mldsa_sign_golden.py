"""CPU: tests/golden/mldsa_sign.json regenerates identically from tests/mldsa_spec.py, the generator's loop with
bookkeeping is the spec's loop, and the fixture covers what its generator promises.  The threshold pairs are
recomputed here from mldsa_spec alone: each sits exactly on its threshold and one inside it, and a signer whose
comparison is off by one in either direction gives other results on them."""
import hashlib
import json

import numpy as np
import pytest

import make_golden_mldsa_sign as gold
import mldsa_spec as spec


@pytest.fixture(scope="module")
def sets():
    return gold.load()


def test_fixture_regenerates_identically():
    text = json.dumps(gold.build(), indent=0, separators=(",", ":")) + "\n"
    assert text == gold.OUT.read_text()
    assert len(text) < 64 * 1024  # hashes, not signatures


@pytest.mark.parametrize("name", gold.NAMES)
def test_trace_is_the_specs_loop(sets, name):
    s = sets[name]
    assert hashlib.sha3_256(s["pk"]).hexdigest() == s["pk_sha3"]
    row = min((r for r in s["rows"] if r["kind"] == "honest"), key=lambda r: (r["ctx_len"] == 0, r["iters"]))
    sig = spec.sign(row["sk"], row["msg"], row["ctx"])
    assert hashlib.sha3_256(sig).hexdigest() == row["sig_sha3"]
    assert spec.verify(s["pk"], row["msg"], sig, row["ctx"])
    # the loop stops at its cap
    capped = gold.trace(gold.Key(name, row["sk"]), row["msg"], row["ctx"], cap=row["iters"] - 1)
    assert capped[0] is None and capped[1] == row["iters"] - 1


@pytest.mark.parametrize("name", gold.NAMES)
def test_fixture_covers_what_it_promises(sets, name):
    p = spec.PARAMS[name]
    rows = sets[name]["rows"]
    for r in rows:
        assert r["iters"] == len(r["reasons"]) + 1 and len(r["msg"]) == r["len"] and len(r["ctx"]) == r["ctx_len"]
        assert set(r["reasons"]) <= {"z", "r", "zr", "t", "h"}
        assert r["kind"] in ("honest", "crafted_t", "crafted_h") + gold.EDGE_KINDS and len(r["sk"]) == p.sk
        assert (r["sk"] == sets[name]["sk"]) == (r["kind"] == "honest")  # crafted keys are marked as such
        assert hashlib.sha3_256(r["sk"]).hexdigest() == r["sk_sha3"]
    assert any(r["iters"] == 1 for r in rows) and any(r["iters"] >= 10 for r in rows)
    reasons = {x for r in rows for x in r["reasons"]}
    assert {"z", "r", "zr", "h"} <= reasons
    # tau 2^12 < gamma2 for ML-DSA-65 / 87: the branch exists for ML-DSA-44 alone, and only a crafted key reaches it
    assert ("t" in reasons) == (name == "ML-DSA-44") == (p.tau << 12 >= p.gamma2)
    assert all("t" not in r["reasons"] for r in rows if r["kind"] == "honest")
    if name == "ML-DSA-44":
        t = [r for r in rows if r["kind"] == "crafted_t"]
        assert len(t) == 1 and t[0]["reasons"][0] == "t"
        t0 = spec.sk_decode(p, t[0]["sk"])[5]
        assert p.gamma2 <= p.tau * ((1 << 12) - 1) == int(abs(t0[0]).sum()) - int((t0[0] == 1 << 12).sum())
    # message lengths: 0, 1, the mu absorb at 135 / 136 / 137 bytes, and both ends of the context length
    shapes = {(r["len"], r["ctx_len"]) for r in rows}
    assert {(0, 0), (1, 0), (69, 0), (70, 0), (71, 0), (0, 255), (33, 255)} <= shapes
    assert {64 + 2 + c + n for n, c in shapes} >= {135, 136, 137}


# ------------------------------------------------------------------ the threshold pairs
def first_iteration(p, A, sk, M):
    """Algorithm 7 up to its checks for kappa = 0, rnd = 32 zero bytes and no context, from mldsa_spec alone: the
    centred z, LowBits(w - c s2), the centred c t0, the hint, and the signature these encode to."""
    Q = spec.Q
    rho, K, tr, s1, s2, t0 = spec.sk_decode(p, sk)
    mu = spec.H(tr + spec.format_message(M), 64)
    y = spec.expand_mask(p, spec.H(K + bytes(32) + mu, 64), 0)
    yh = [spec.ntt(v) for v in y]
    w = [spec.ntt_inv(sum(A[i][j] * yh[j] for j in range(p.l)) % Q) for i in range(p.k)]
    ctilde = spec.H(mu + spec.w1_encode(p, [spec.high_bits(p, wi) for wi in w]), p.ctilde)
    ch = spec.ntt(spec.sample_in_ball(p, ctilde))
    z = [spec.mod_pm(y[j] + spec.ntt_inv(ch * spec.ntt(s1[j]) % Q), Q) for j in range(p.l)]
    r = [(w[i] - spec.ntt_inv(ch * spec.ntt(s2[i]) % Q)) % Q for i in range(p.k)]
    ct0 = [spec.ntt_inv(ch * spec.ntt(t0[i]) % Q) for i in range(p.k)]
    h = [spec.make_hint(p, -ct0[i], r[i] + ct0[i]) for i in range(p.k)]
    return {"z": z, "r": [spec.low_bits(p, ri) for ri in r], "t": [spec.mod_pm(t, Q) for t in ct0], "h": h,
            "sig": spec.sig_encode(p, ctilde, z, h)}


def measure(f):
    """What each of the four checks compares with its threshold."""
    return {x: (sum(int(v.sum()) for v in f[x]) if x == "h" else max(int(np.max(np.abs(v))) for v in f[x]))
            for x in gold.CHECKS}


@pytest.mark.parametrize("name", gold.NAMES)
def test_threshold_pairs_sit_on_their_thresholds(sets, name):
    p = spec.PARAMS[name]
    honest = spec.sk_decode(p, sets[name]["sk"])
    A = spec.expand_a(p, honest[0])
    lim = {"z": p.gamma1 - p.beta, "r": p.gamma2 - p.beta, "t": p.gamma2, "h": p.omega + 1}  # the least that rejects
    seen = []
    for at, twin in gold.stored_pairs(sets[name]["rows"]):
        check = at["kind"][len("edge_"):]
        assert at["msg"] == twin["msg"] and at["ctx"] == twin["ctx"] == b""
        assert at["iters"] >= 2 and at["reasons"][0] == check and (twin["iters"], twin["reasons"]) == (1, [])
        secrets = []
        for row, want in ((at, lim[check]), (twin, lim[check] - 1)):
            rho, K, tr, s1, s2, t0 = spec.sk_decode(p, row["sk"])
            assert (rho, K, tr) == honest[:3] and spec.sk_encode(p, rho, K, tr, s1, s2, t0) == row["sk"]
            # inside what skDecode accepts: the signer's refusal of a key is not what rejects the row
            assert all(int(np.max(np.abs(v))) <= p.eta for v in s1 + s2)
            assert all(-((1 << 12) - 1) <= int(v.min()) and int(v.max()) <= 1 << 12 for v in t0)
            f = first_iteration(p, A, row["sk"], row["msg"])
            got = measure(f)
            assert got[check] == want, (check, got)
            # the other three checks pass in that iteration: an at-threshold row is never "zr"
            assert [x for x in gold.CHECKS if got[x] >= lim[x]] == ([check] if row is at else []), got
            if check != "h":  # the signed value is where the rule puts it, and it is the one that decides
                assert int(f[check][row["poly"]][row["coef"]]) == row["value"] and abs(row["value"]) == want
            if row is twin:
                assert hashlib.sha3_256(f["sig"]).hexdigest() == row["sig_sha3"]
            secrets.append(np.concatenate(s1 + s2 + t0))
        if check == "h":
            # sigEncode at index == omega: the last index byte is written, no padding is left before the counts
            packed = f["sig"][-(p.omega + p.k):]
            assert packed[-1] == p.omega and int(spec.hint_bit_unpack(p, packed).sum()) == p.omega
            seen.append((check, 0))
        else:  # the two keys differ by one unit in one coefficient
            assert int(np.abs(secrets[0] - secrets[1]).sum()) == 1
            assert twin["value"] == at["value"] - np.sign(at["value"])
            seen.append((check, int(np.sign(at["value"]))))
    want = [(x, s) for x in "zrt" for s in (1, -1) if x != "t" or name == "ML-DSA-44"] + [("h", 0)]
    assert seen == want


@pytest.mark.parametrize("name", gold.NAMES)
def test_fixture_tells_off_by_one_signers(sets, name):
    """Each check moved by one in either direction (gold.trace's `off`) changes the iteration count or the
    signature of a stored row of that check's pairs; moved by nothing, it changes none."""
    A = spec.expand_a(spec.PARAMS[name], sets[name]["sk"][:32])
    pairs = gold.stored_pairs(sets[name]["rows"])
    for check in {at["kind"][len("edge_"):] for at, _ in pairs}:
        rows = [r for pair in pairs for r in pair if r["kind"] == "edge_" + check]
        keys = [gold.Key(name, r["sk"], A) for r in rows]

        def results(off):
            out = [gold.trace(k, r["msg"], off=off) for k, r in zip(keys, rows)]
            return [(it, hashlib.sha3_256(sig).hexdigest()) for sig, it, _ in out]

        stored = [(r["iters"], r["sig_sha3"]) for r in rows]
        assert results(None) == results({check: 0}) == stored
        for delta in (1, -1):
            assert results({check: delta}) != stored, (check, delta)
    assert {at["kind"] for at, _ in pairs} == set(gold.EDGE_KINDS) - ({"edge_t"} if name != "ML-DSA-44" else set())
