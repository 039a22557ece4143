"""The SLH-DSA device primitives (csrc/slhdsa_common.cuh, csrc/sha2.cuh) alone, at the edges of their domains.

tests/slhdsa_probe.hip (its own shared object, built by csrc/Makefile from the headers the kernels include)
runs each primitive as compiled for the GPU on the constructed inputs of tests/slhdsa_prim_cases.py and copies
nothing back itself; every comparison here is byte-exact or integer-exact against tests/slhdsa_spec.py,
hashlib or plain Python integers.  Output buffers are prefilled with a non-zero byte, so an unwritten result
fails.  tests/test_slhdsa_prim_cases.py asserts on the CPU that the inputs reach the edges they are built for.

WOTS+ digits: wots_csum, wots_msg_digit and wots_csum_digit are pinned.  The core kernel's select of the
node's word c >> 3 from registers is written inside k_slhdsa_core, not in the header, so the probe indexes the
word directly and that select stays covered by the whole-signature tests.

row_span reads only the two offsets, never a message byte, so the 2^31-byte threshold is exercised here with
no memory behind the offsets."""
import ctypes as ct
import hashlib
from pathlib import Path

import numpy as np
import pytest

import slhdsa_prim_cases as cases
import slhdsa_spec as spec

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NAMES = cases.NAMES
FILL = 0xA5


@pytest.fixture(scope="module")
def probe():
    path = Path(__file__).resolve().parent / "libslhdsa_probe.so"
    assert path.exists(), f"{path} is missing: the default target of csrc/Makefile builds it"
    lib = ct.CDLL(str(path))
    P, SZ, I, U = ct.c_void_p, ct.c_size_t, ct.c_int, ct.c_uint32
    lib.slhp_sha_tail.argtypes = [I, SZ, P, P, P, P, P, P, P, P]
    lib.slhp_h_msg.argtypes = [I, SZ, P, P, P, P, P, U, P]
    lib.slhp_hash_f.argtypes = [I, SZ, P, P, P, P]
    lib.slhp_hash_h.argtypes = [I, SZ, P, P, P, P, P, P]
    lib.slhp_t_lds.argtypes = [I, SZ, I, P, P, P, P]
    lib.slhp_fors_index.argtypes = [I, SZ, P, P]
    lib.slhp_indices.argtypes = [I, SZ, P, P, P]
    lib.slhp_wots_digits.argtypes = [I, SZ, P, P, P]
    lib.slhp_row_span.argtypes = [SZ, P, P, P, P]
    return lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(parts, pad=1):
    """Byte strings joined into one device buffer (never empty: an all-empty list still gets `pad` bytes)."""
    data = b"".join(parts)
    return _dev(np.frombuffer(data if data else bytes(pad), np.uint8))


def _u64(values):
    return _dev(np.array(values, dtype=np.uint64).view(np.int64))


def _u32(values):
    return _dev(np.array(values, dtype=np.uint32).view(np.int32))


def _out(shape, dtype):
    """A device buffer whose every byte is FILL."""
    width = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((int(np.prod(shape)) * width,), FILL, dtype=torch.uint8, device="cuda")
    return raw.view(dtype).reshape(shape)


def _rows(t):
    return [r.tobytes() for r in t.cpu().numpy()]


def _adrs(hc):
    return _u64([list(c.adrs) for c in hc])


# ------------------------------------------------------------------ sha::tail / sha::tail512
@pytest.mark.parametrize("big", (False, True), ids=("sha256", "sha512"))
def test_sha_tail(probe, big):
    h = cases.SHA512 if big else cases.SHA256
    ref = hashlib.sha512 if big else hashlib.sha256
    tc = cases.tail_cases(big)
    n = len(tc)
    boff = np.cumsum([0] + [len(c.data) for c in tc])
    over = np.zeros((n, 16), np.uint64)
    for i, c in enumerate(tc):
        for t, v in c.over.items():
            over[i, t] = v
    out = _out((n, 8), torch.int64)
    args = [_u64([c.state for c in tc]), _u32([c.prefix for c in tc]), _u32([len(c.data) for c in tc]),
            _u32(boff[:-1]), _bytes(c.data for c in tc), _u32([sum(1 << t for t in c.over) for c in tc]),
            _dev(over.view(np.int64))]
    assert probe.slhp_sha_tail(int(big), n, *(a.data_ptr() for a in args), out.data_ptr()) == 0
    got = out.cpu().numpy().view(np.uint64)
    wb = h.bits // 8
    for i, c in enumerate(tc):
        state = [int(v) for v in got[i]]
        if c.prefix == 0 and not c.over:  # a whole message: hashlib
            assert b"".join(v.to_bytes(wb, "big") for v in state) == ref(c.data).digest(), c.label
        assert state == h.tail(c.state, c.prefix, c.data, c.over), c.label


# ------------------------------------------------------------------ H_msg
@pytest.mark.parametrize("name", NAMES)
def test_h_msg_over_every_length(probe, name):
    p = spec.PARAMS[name]
    for ctx in cases.h_msg_contexts(name):
        rows = cases.h_msg_cases(name, ctx)
        n = len(rows)
        moff = np.cumsum([0] + [len(m) for _, _, m in rows])
        r, pkr, msg = _bytes(x[0] for x in rows), _bytes(x[1] for x in rows), _bytes(x[2] for x in rows)
        cs = _bytes([ctx])
        out = _out((n, p.m), torch.uint8)
        assert probe.slhp_h_msg(cases.ps_of(name), n, r.data_ptr(), pkr.data_ptr(), msg.data_ptr(),
                                _u32(moff).data_ptr(), cs.data_ptr() if ctx else None, len(ctx),
                                out.data_ptr()) == 0
        got = _rows(out)
        for i, row in enumerate(rows):
            assert got[i] == cases.h_msg_expected(name, ctx, *row), (len(ctx), i)


# ------------------------------------------------------------------ F, H and T_l over the address edges
@pytest.mark.parametrize("n", cases.SIZES)
def test_hash_f(probe, n):
    p = cases.params_of(n)
    hc = cases.hash_cases(n, 1, "f")
    out = _out((len(hc), n), torch.uint8)
    assert probe.slhp_hash_f(n, len(hc), _bytes(c.seed for c in hc).data_ptr(), _adrs(hc).data_ptr(),
                             _bytes(c.nodes for c in hc).data_ptr(), out.data_ptr()) == 0
    got = _rows(out)
    for i, c in enumerate(hc):
        assert got[i] == spec.Hasher(p, c.seed).F(cases.adrs_bytes(c.adrs), c.nodes), c.label


@pytest.mark.parametrize("n", cases.SIZES)
def test_hash_h_with_the_node_on_both_sides(probe, n):
    p = cases.params_of(n)
    hc = cases.hash_cases(n, 2, "h")
    m = len(hc)
    # x is the left node of c.nodes (right = 0), then the right node (right = 1)
    x = [c.nodes[:n] for c in hc] + [c.nodes[n:] for c in hc]
    au = [c.nodes[n:] for c in hc] + [c.nodes[:n] for c in hc]
    right = np.array([0] * m + [1] * m, np.uint8)
    out = _out((2 * m, n), torch.uint8)
    assert probe.slhp_hash_h(n, 2 * m, _bytes(c.seed for c in hc + hc).data_ptr(), _adrs(hc + hc).data_ptr(),
                             _bytes(x).data_ptr(), _bytes(au).data_ptr(), _dev(right).data_ptr(),
                             out.data_ptr()) == 0
    got = _rows(out)
    for i, c in enumerate(hc):
        want = spec.Hasher(p, c.seed).T(cases.adrs_bytes(c.adrs), c.nodes)
        assert got[i] == want and got[m + i] == want, c.label
        swapped = spec.Hasher(p, c.seed).T(cases.adrs_bytes(c.adrs), c.nodes[n:] + c.nodes[:n])
        assert swapped != want  # so the side matters


@pytest.mark.parametrize("n", cases.SIZES)
def test_t_lds_over_k_and_len_nodes(probe, n):
    p = cases.params_of(n)
    for tag, l in (("tk", p.k), ("tlen", p.len)):
        hc = cases.hash_cases(n, l, tag)
        out = _out((len(hc), n), torch.uint8)
        assert probe.slhp_t_lds(n, len(hc), l, _bytes(c.seed for c in hc).data_ptr(), _adrs(hc).data_ptr(),
                                _bytes(c.nodes for c in hc).data_ptr(), out.data_ptr()) == 0
        got = _rows(out)
        for i, c in enumerate(hc):
            assert got[i] == spec.Hasher(p, c.seed).T(cases.adrs_bytes(c.adrs), c.nodes), (l, c.label)


# ------------------------------------------------------------------ indices
@pytest.mark.parametrize("name", NAMES)
def test_fors_indices(probe, name):
    p = spec.PARAMS[name]
    pats = cases.md_patterns(name)
    out = _out((len(pats), p.k), torch.int32)
    assert probe.slhp_fors_index(cases.ps_of(name), len(pats), _bytes(v for _, v in pats).data_ptr(),
                                 out.data_ptr()) == 0
    got = out.cpu().numpy().view(np.uint32).tolist()
    for i, (label, md) in enumerate(pats):
        assert got[i] == spec._fors_indices(p, md), label


@pytest.mark.parametrize("name", NAMES)
def test_tree_and_leaf_indices_of_every_layer(probe, name):
    p = spec.PARAMS[name]
    dgs = cases.index_digests(name)
    trees, leaves = _out((len(dgs), p.d), torch.int64), _out((len(dgs), p.d), torch.int32)
    assert probe.slhp_indices(cases.ps_of(name), len(dgs), _bytes(v for _, v in dgs).data_ptr(), trees.data_ptr(),
                              leaves.data_ptr()) == 0
    t, l = trees.cpu().numpy().view(np.uint64).tolist(), leaves.cpu().numpy().view(np.uint32).tolist()
    for i, (label, dg) in enumerate(dgs):
        assert list(zip(t[i], l[i])) == cases.layer_indices(p, dg), label


# ------------------------------------------------------------------ WOTS+ digits
@pytest.mark.parametrize("n", cases.SIZES)
def test_wots_digits_and_checksum(probe, n):
    p = cases.params_of(n)
    nodes = cases.wots_nodes(n)
    csum, digits = _out((len(nodes),), torch.int32), _out((len(nodes), p.len), torch.int32)
    assert probe.slhp_wots_digits(n, len(nodes), _bytes(v for _, v in nodes).data_ptr(), csum.data_ptr(),
                                  digits.data_ptr()) == 0
    cs, dg = csum.cpu().numpy().view(np.uint32).tolist(), digits.cpu().numpy().view(np.uint32).tolist()
    for i, (label, node) in enumerate(nodes):
        want = spec.wots_digits(p, node)
        assert cs[i] == sum(15 - d for d in want[:2 * n]), label
        assert dg[i] == want, label


# ------------------------------------------------------------------ row_span
def test_row_span_at_the_threshold(probe):
    rows = cases.ROW_SPANS
    n = len(rows)
    ok, o0, mlen = _out((n,), torch.int32), _out((n,), torch.int64), _out((n,), torch.int32)
    off = _u64([[c.o0, c.o1] for c in rows])
    assert probe.slhp_row_span(n, off.data_ptr(), ok.data_ptr(), o0.data_ptr(), mlen.data_ptr()) == 0
    ok, o0 = ok.cpu().numpy().tolist(), o0.cpu().numpy().view(np.uint64).tolist()
    mlen = mlen.cpu().numpy().view(np.uint32).tolist()
    for i, c in enumerate(rows):
        assert ok[i] == int(c.accepted), c.label
        assert o0[i] == c.o0, c.label  # returned whole, above 2^32 too
        if c.accepted:
            assert mlen[i] == c.o1 - c.o0, c.label
