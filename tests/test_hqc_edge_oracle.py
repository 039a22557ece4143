"""HQC ring products at the edges of support and operand (CPU): the C oracle against the
pure-Python restatement on tests/golden/hqc_edge.json.

Each record carries one property honest traffic does not supply (tests/golden/make_golden_hqc_edge.py):
a sparse operand that contains position 0, position n - 1, a replaced duplicate or a position a
whole number of words from n; a dense operand that is zero, a single bit next to a word boundary,
all ones, only the stray bits above X^(n-1), ....  The fixture's digests were computed by the
Python spec; here the C oracle (oracle/src/hqc.c) is held to them record by record, the spec is
recomputed directly, and its product is checked against the closed form for single-bit operands.
The GPU path is held to the same records in tests/test_gpu_hqc_product.py.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import hqc_spec as H
import make_golden_hqc_edge as E
import oracle as orc

GOLD = json.loads((Path(__file__).parent / "golden" / "hqc_edge.json").read_text())
ALGS = ["HQC-128", "HQC-192", "HQC-256"]
SINGLE = ("x0", "xn1", "x31", "x32", "xw1", "xw")


def _rows(items):
    return np.stack([np.frombuffer(bytes(b), np.uint8) for b in items])


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.mark.parametrize("alg", ALGS)
def test_fixture_shape(alg):
    """One KeyGen record and one Decaps group per sparse property, one Encaps record per
    (dense operand, sparse property), counters for every theta class of the crafted keys."""
    g = GOLD[alg]
    assert [r["prop"] for r in g["kg"]] == list(E.PROPS) == [d["sk"] for d in g["decaps"]]
    assert [(r["pk"], r["prop"]) for r in g["enc"]] == [(d, q) for d in E.DENSE for q in E.PROPS]
    assert set(g["enc_counters"]) == {E.theta_class(alg, d) for d in E.DENSE}
    cts = E.ct_list(alg)
    assert ("ff", "zero") in cts and ("zero", "ff") in cts  # the u | v cut, both directions
    assert all(len(d["status"]) == len(cts) == len(E.DENSE) * len(E.V) for d in g["decaps"])


@pytest.mark.parametrize("alg", ALGS)
def test_dense_operands_are_what_their_labels_say(alg):
    p = H.params(alg)
    n, nb = p["n"], p["nb"]
    val = {d: int.from_bytes(E.dense(alg, d), "little") for d in E.DENSE}
    assert all(len(E.dense(alg, d)) == nb for d in E.DENSE)
    assert val["zero"] == 0 and val["ones"] == (1 << n) - 1 and val["ff"] == (1 << 8 * nb) - 1
    assert val["stray"] == val["ff"] ^ val["ones"] and val["stray"] >> n == (1 << (8 * nb - n)) - 1
    last = 32 * (n // 32)
    assert [val[d].bit_length() - 1 for d in SINGLE] == [0, n - 1, 31, 32, last - 1, last]
    assert all(bin(val[d]).count("1") == 1 for d in SINGLE) and last < n < last + 32
    assert E.dense(alg, "aa") == b"\xaa" * nb and len(set(val.values())) == len(E.DENSE)


@pytest.mark.parametrize("alg", ALGS)
def test_keygen_records(alg):
    """y of every KeyGen record has its property; keypair by the spec matches the digests and
    the C oracle byte for byte."""
    recs = GOLD[alg]["kg"]
    coins = [bytes.fromhex(r["kp_coins"]) for r in recs]
    opk, osk = orc.batch_keypair(alg, _rows(coins))
    n = H.params(alg)["n"]
    for i, (r, c) in enumerate(zip(recs, coins)):
        assert c == E.kg_coins(alg, r["c"])
        raw, y = E.y_of(alg, c)
        assert E.has_property(alg, r["prop"], raw, y), r["prop"]
        pk, sk = H.keypair(alg, c)
        assert (_sha(pk), _sha(sk)) == (r["pk"], r["sk"])
        assert opk[i].tobytes() == pk and osk[i].tobytes() == sk
        assert E.secret_y(alg, sk) == y
    named = {r["prop"]: E.y_of(alg, c)[1] for r, c in zip(recs, coins)}
    assert 0 in named["pos0"] and n - 1 in named["posn1"] and any((n - k) % 32 == 0 for k in named["align32"])


@pytest.mark.parametrize("alg", ALGS)
def test_encaps_records(alg):
    """r2 of every Encaps record has its property under its crafted key; Encaps by the spec
    matches the digests and the C oracle byte for byte."""
    g = GOLD[alg]
    recs = g["enc"]
    pks = [E.edge_pk(alg, r["pk"]) for r in recs]
    coins = [E.enc_coins(alg, E.theta_class(alg, r["pk"]), g["enc_counters"][E.theta_class(alg, r["pk"])][r["prop"]])
             for r in recs]
    oct_, oss = orc.batch_encaps(alg, _rows(pks), _rows(coins))
    for i, (r, pk, c) in enumerate(zip(recs, pks, coins)):
        assert E.has_property(alg, r["prop"], *E.r2_of(alg, pk, c)), (r["pk"], r["prop"])
        ct, ss = H.encaps(alg, pk, c)
        assert _sha(ct + ss) == r["ct_ss"], (r["pk"], r["prop"])
        assert oct_[i].tobytes() == ct and oss[i].tobytes() == ss, (r["pk"], r["prop"])


@pytest.mark.parametrize("alg", ALGS)
def test_decaps_records(alg):
    """Decaps of every crafted ciphertext with every sparse-edge secret key: the C oracle's ss and
    status give the fixture's digests and equal the spec's Decaps, run again in full; the decoder's
    word by the spec gives the fixture's."""
    g = GOLD[alg]
    cts = [E.edge_ct(alg, u, v) for u, v in E.ct_list(alg)]
    for r, d in zip(g["kg"], g["decaps"]):
        _, sk = H.keypair(alg, bytes.fromhex(r["kp_coins"]))
        y = E.secret_y(alg, sk)
        assert _sha(b"".join(E.decode_word(alg, y, c) for c in cts)) == d["t"]
        oss, ost = orc.batch_decaps(alg, _rows([sk] * len(cts)), _rows(cts), with_status=True)
        assert ost.tolist() == d["status"], d["sk"]
        assert _sha(oss.tobytes()) == d["ss"], d["sk"]
        spec = [H.decaps(alg, sk, c) for c in cts]
        assert [rc for _, rc in spec] == d["status"]
        assert [s for s, _ in spec] == [oss[i].tobytes() for i in range(len(cts))]


@pytest.mark.parametrize("alg", ALGS)
def test_single_bit_products_have_their_closed_form(alg):
    """X^j times a sparse vector is its support rotated by j: every position q goes to q + j, folded
    once (q + j - n when q + j >= n).  Checked for the single-bit dense operands against the y of
    every KeyGen record, position 0 and n - 1 among them."""
    n = H.params(alg)["n"]
    for r in GOLD[alg]["kg"]:
        y = E.y_of(alg, bytes.fromhex(r["kp_coins"]))[1]
        for d in SINGLE:
            j = int.from_bytes(E.dense(alg, d), "little").bit_length() - 1
            want = H.support_to_int([q + j - n if q + j >= n else q + j for q in y])
            assert H.mul_sparse(y, 1 << j, n) == want, (r["prop"], d)
        assert H.mul_sparse(y, 0, n) == 0
        # stray bits only: X^(n+i) folds to X^i, so the all-0xFF operand is `ones` plus `stray`
        ones, stray, ff = (int.from_bytes(E.dense(alg, d), "little") for d in ("ones", "stray", "ff"))
        assert H.mul_sparse(y, ff, n) == H.mul_sparse(y, ones, n) ^ H.mul_sparse(y, stray, n)
        assert H.mul_sparse(y, ones, n) == ((1 << n) - 1 if len(y) % 2 else 0)


def test_trace_hook_is_exported_and_declared_as_a_test_hook():
    """Exported, declared in the hook header (whose first line says what it holds) and not in the public one,
    and bound in the hooks' table."""
    from qrkem import _debug
    from test_abi import declared_functions, exported_symbols
    from test_debug_abi import DEBUG_HEADER
    name = "qrk_dbg_hqc_decaps_trace"
    assert name in exported_symbols() and name in declared_functions(DEBUG_HEADER)
    assert name not in declared_functions() and name in _debug.HOOKS
    assert "test hooks" in DEBUG_HEADER.read_text().splitlines()[0]
