"""CPU: the constructed inputs of tests/slhdsa_prim_cases.py are what they claim to be, from tests/slhdsa_spec.py
alone.  tests/test_gpu_slhdsa_prims.py runs the same inputs through the device header; every "occurs"
condition is asserted here, so that a shrinking input set fails on the CPU instead of silently covering less
on the GPU."""
import hashlib

import pytest

import slhdsa_prim_cases as cases
import slhdsa_spec as spec

NAMES = cases.NAMES


# ------------------------------------------------------------------ WOTS+ nodes
@pytest.mark.parametrize("n", cases.SIZES)
def test_wots_nodes_reach_every_digit_and_checksum_edge(n):
    p = cases.params_of(n)
    nodes = dict(cases.wots_nodes(n))
    assert len(nodes) == len(cases.wots_nodes(n))  # labels are unique
    assert sum(1 for k in nodes if k.startswith("random ")) == 64
    digits = {k: spec.wots_digits(p, v) for k, v in nodes.items()}
    csum = {k: sum(15 - d for d in v[:2 * n]) for k, v in digits.items()}
    for k, d in digits.items():
        assert len(nodes[k]) == n and len(d) == p.len
        assert d[2 * n:] == [csum[k] >> 8, (csum[k] >> 4) & 15, csum[k] & 15], k
    assert csum["all-zero digits"] == 30 * n == {16: 480, 24: 720, 32: 960}[n]
    assert csum["all-0xF digits"] == 0
    for pos in range(2 * n):
        d = digits[f"digit 0 at {pos} among 0xF"][:2 * n]
        assert d[pos] == 0 and d.count(15) == 2 * n - 1
        d = digits[f"digit 0xF at {pos} among 0"][:2 * n]
        assert d[pos] == 15 and d.count(0) == 2 * n - 1
    want = [t for t in cases.CSUM_TARGETS + (30 * n - 1,) if t <= 30 * n]
    assert {15, 16, 255, 256, 30 * n - 1} <= set(want) and (n == 16 or {511, 512} <= set(want))
    for t in want:
        assert csum[f"checksum {t}"] == t
    # every message digit value at every position
    for pos in range(2 * n):
        assert {d[pos] for d in digits.values()} == set(range(16)), pos
    # every value each checksum digit can reach
    top = {16: 1, 24: 2, 32: 3}[n]
    assert 30 * n >> 8 == top
    assert {d[2 * n] for d in digits.values()} == set(range(top + 1))
    assert {d[2 * n + 1] for d in digits.values()} == set(range(16))
    assert {d[2 * n + 2] for d in digits.values()} == set(range(16))


# ------------------------------------------------------------------ md patterns
@pytest.mark.parametrize("name", NAMES)
def test_md_patterns_reach_every_index_value_and_ignore_the_tail(name):
    p = spec.PARAMS[name]
    pats = cases.md_patterns(name)
    assert len(pats) == 2 + 2 * 8 * p.md + 64 and all(len(v) == p.md for _, v in pats)
    idx = {k: spec._fors_indices(p, v) for k, v in pats}
    assert all(len(v) == p.k and all(0 <= x < 1 << p.a for x in v) for v in idx.values())
    top = (1 << p.a) - 1
    assert idx["zeros"] == [0] * p.k and idx["ones"] == [top] * p.k
    need = {0, top} | {1 << j for j in range(p.a)}
    for i in range(p.k):
        assert need <= {v[i] for v in idx.values()}, i
    # a walked bit either moves exactly one index by one power of two or, in the unused tail, none
    unused = []
    for b in range(8 * p.md):
        one, zero = idx[f"one at bit {b}"], idx[f"zero at bit {b}"]
        moved = [i for i in range(p.k) if one[i]]
        if not moved:
            unused.append(b)
            assert zero == [top] * p.k
            continue
        assert len(moved) == 1 and one[moved[0]] & (one[moved[0]] - 1) == 0
        assert zero == [top ^ one[i] for i in range(p.k)]
    spare = 8 * p.md - p.k * p.a
    assert spare == {16: 2, 24: 0, 32: 5}[p.n] and len(unused) == spare
    if p.fips:  # base_2b reads most significant bit first: the low bits of the last byte are left over
        assert unused == list(range(8 * p.md - spare, 8 * p.md))
    else:  # round 3.1 reads least significant bit first: the high bits of the last byte are left over
        assert unused == list(range(8 * p.md - 8, 8 * p.md - 8 + spare))


# ------------------------------------------------------------------ tree and leaf indices
@pytest.mark.parametrize("name", NAMES)
def test_index_digests_show_what_happens_to_the_top_bit(name):
    p = spec.PARAMS[name]
    dg = dict(cases.index_digests(name))
    assert len(dg) == 2 + 2 * 72 + 64 and all(len(v) == p.m for v in dg.values())
    got = {k: cases.layer_indices(p, v) for k, v in dg.items()}
    for k, layers in got.items():
        assert len(layers) == p.d
        tree, leaf = layers[0]
        assert tree < 1 << (p.h - p.hp) and leaf < 1 << p.hp
        whole = (tree << p.hp) | leaf  # the h-bit index the layers take apart, h' bits at a time
        for j, (t, l) in enumerate(layers):
            assert l == (whole >> (p.hp * j)) & ((1 << p.hp) - 1) and t == whole >> (p.hp * (j + 1)), (k, j)
        assert layers[-1][0] == 0
    assert got["zeros"][0] == (0, 0)
    assert got["ones"][0] == ((1 << (p.h - p.hp)) - 1, (1 << p.hp) - 1)
    if p.n == 32:  # h - h' = 64: the top bit of the 8-byte field is kept
        assert got["one at bit 0"][0] == (1 << 63, 0)
        assert got["zero at bit 0"][0] == ((1 << 63) - 1, (1 << p.hp) - 1)
    else:  # h - h' = 63: it is dropped
        assert got["one at bit 0"][0] == (0, 0)
        assert got["zero at bit 0"][0] == got["ones"][0]
        assert got["one at bit 1"][0] == (1 << 62, 0)
    for b in range(64, 72):  # the leaf byte: its low h' bits count
        assert got[f"one at bit {b}"][0] == (0, (1 << (71 - b)) & ((1 << p.hp) - 1))


# ------------------------------------------------------------------ addresses
@pytest.mark.parametrize("n", cases.SIZES)
def test_addresses_cover_every_field_edge(n):
    p = cases.params_of(n)
    adrs = dict(cases.addresses(n))
    assert len(adrs) == len(cases.addresses(n))
    assert {adrs[f"type {t}"].type for t in range(7)} == set(range(7))
    assert adrs["layer d - 1"].layer == p.d - 1
    assert adrs["largest tree"].tree == (1 << (p.h - p.hp)) - 1
    if n == 32:
        assert adrs["tree 2^64 - 1"].tree == 2**64 - 1
    big = adrs["largest words"]
    assert (big.w1, big.w2, big.w3) == ((1 << p.hp) - 1, p.len - 1, (p.k << p.a) - 1)
    assert adrs["largest chain"].w3 == 14
    # the compressed address: 22 bytes, each field in its own bytes and nowhere else
    at = ((0, 1), (1, 9), (9, 10), (10, 14), (14, 18), (18, 22))
    for f, (lo, hi) in zip(cases.Address._fields, at):
        b = cases.adrs_bytes(adrs[f"only {f} all-ones"])
        assert len(b) == 22 and b == bytes(lo) + b"\xff" * (hi - lo) + bytes(22 - hi)
        b = cases.adrs_bytes(adrs[f"only {f} zero"])
        assert b == b"\xff" * lo + bytes(hi - lo) + b"\xff" * (22 - hi)
    for tag, nodes in (("f", 1), ("h", 2), ("tk", p.k), ("tlen", p.len)):
        hc = cases.hash_cases(n, nodes, tag)
        assert len(hc) == len(adrs) and all(len(c.seed) == n and len(c.nodes) == nodes * n for c in hc)
        assert len({c.seed for c in hc}) == len(hc)
    assert p.len > 64 if n == 32 else p.len <= 64  # n = 32: the lanes write the len nodes in two passes


# ------------------------------------------------------------------ H_msg
@pytest.mark.parametrize("name", NAMES)
def test_h_msg_cases_cross_every_block_edge(name):
    p = spec.PARAMS[name]
    ctxs = cases.h_msg_contexts(name)
    assert [len(c) for c in ctxs] == ([0, 1, 255] if p.fips else [0])
    block = 64 if p.n == 16 else 128
    for ctx in ctxs:
        rows = cases.h_msg_cases(name, ctx)
        assert [len(m) for _, _, m in rows] == list(range(301))
        assert all(len(r) == p.n and len(pkr) == 2 * p.n for r, pkr, _ in rows)
        totals = [3 * p.n + len(spec._frame(p, m, ctx)) for _, _, m in rows]
        # the padding of the inner hash turns over at block - 9 (SHA-256) or block - 17 (SHA-512)
        edge = block - (9 if block == 64 else 17)
        crossed = [t for t in totals if t % block in (edge, edge + 1)]
        assert len(crossed) >= 4 and blocks_spread(totals, block) >= 2
        assert len(cases.h_msg_expected(name, ctx, *rows[0])) == p.m
    if not p.fips:
        with pytest.raises(ValueError):
            cases.h_msg_expected(name, b"x", *cases.h_msg_cases(name, b"")[0])


def blocks_spread(totals, block) -> int:
    return max(totals) // block - min(totals) // block


# ------------------------------------------------------------------ SHA-2 tails
@pytest.mark.parametrize("big", (False, True))
def test_plain_python_sha2_agrees_with_hashlib(big):
    h = cases.SHA512 if big else cases.SHA256
    ref = hashlib.sha512 if big else hashlib.sha256
    for k in list(range(0, 300, 7)) + [h.block - 1, h.block, 2 * h.block, 1000]:
        data = cases.rand(f"sha2-check/{k}", k)
        assert h.digest(data) == ref(data).digest(), k
    # a tail from the state after whole blocks is the rest of the same message
    data = cases.rand("sha2-check/split", 3 * h.block + 77)
    state = h.iv()
    for b in range(2):
        state = h.compress(state, data[b * h.block:(b + 1) * h.block])
    got = h.tail(state, 2 * h.block, data[2 * h.block:])
    assert b"".join(v.to_bytes(h.bits // 8, "big") for v in got) == ref(data).digest()


@pytest.mark.parametrize("big", (False, True))
def test_tail_cases_cover_the_length_axis_and_the_high_length_word(big):
    h = cases.SHA512 if big else cases.SHA256
    tc = cases.tail_cases(big)
    first = [c for c in tc if c.state == h.iv() and c.prefix == 0 and not c.over]
    assert [len(c.data) for c in first] == list(range(201))
    rest = [c for c in tc if c.prefix and not c.over]
    lens = {0, 1, 55, 56, 63, 64, 119} | ({111, 112, 127, 128} if big else set())
    assert {c.prefix for c in rest} == {h.block, 2**29 - h.block, 2**29, 2**31}
    for prefix in {c.prefix for c in rest}:
        assert {len(c.data) for c in rest if c.prefix == prefix} == lens
    # bits 32 and up of the bit length (w[14] of the last SHA-256 block) are zero, one and four
    assert {(8 * (c.prefix + len(c.data))) >> 32 for c in rest} == {0, 1, 4}
    assert all(c.state != h.iv() for c in rest)
    over = [c for c in tc if c.over]
    assert len(over) == 3 and len(first) + len(rest) + len(over) == len(tc)
    last = len(h.padded(0, over[1].data)) // h.block - 1
    assert last == 0 and not {14, 15} & set(over[1].over)  # one block: the length words are left alone
    for c in over:  # a replaced word changes the result
        assert h.tail(c.state, c.prefix, c.data, c.over) != h.tail(c.state, c.prefix, c.data)
    assert all(c.prefix + len(c.data) < 2**32 for c in tc)


# ------------------------------------------------------------------ row_span
def test_row_span_table():
    rows = {c.label: c for c in cases.ROW_SPANS}
    assert len(rows) == 10
    for c in rows.values():
        assert 0 <= c.o0 < 2**64 and 0 <= c.o1 < 2**64
        assert c.accepted == (c.o1 >= c.o0 and c.o1 - c.o0 < 2**31), c.label
    assert rows["largest accepted span"].o1 - rows["largest accepted span"].o0 == 2**31 - 1
    assert rows["smallest refused span"].o1 - rows["smallest refused span"].o0 == 2**31
    assert rows["largest accepted span, offset"].o0 == rows["smallest refused span, offset"].o0 == 7
    assert rows["large start, small row"].o0 == 2**40 and rows["wrap"].o0 == 2**64 - 1
