"""CPU: tests/golden/mldsa_sign.json regenerates identically from tests/mldsa_spec.py, the generator's loop with
bookkeeping is the spec's loop, and the fixture covers what its generator promises."""
import hashlib
import json

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
        assert r["kind"] in ("honest", "crafted_t", "crafted_h") and len(r["sk"]) == p.sk
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
