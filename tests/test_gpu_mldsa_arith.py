"""The ML-DSA device primitives (csrc/mldsa_arith.cuh) alone, at the edges of their documented domains.

tests/mldsa_arith_probe.hip (its own shared object, built by csrc/Makefile from the header the kernels
include) runs each primitive as compiled for the GPU:

  sweep mode  whole ranges compared on the device against plain 64-bit integer C++: modmul and reduce
              over every int32 first factor, Decompose and UseHint over every r in [0, q) for both
              gamma2 and h in {0, 1}
  raw mode    outputs copied back and compared here with numpy or tests/mldsa_spec.py; every sweep also
              runs raw on a sub-range straddling an edge, and a deliberately wrong expectation must be
              counted, so the device comparator itself is checked

Figures (domain swept, mismatches) are printed; run with -s to see them.
"""
import ctypes as ct
from pathlib import Path

import numpy as np
import pytest

import make_golden_mldsa as gold
import mldsa_spec as spec

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

Q = spec.Q
HALFQ = (Q + 1) // 2
OP_MODMUL, OP_REDUCE, OP_CANON, OP_DECOMPOSE, OP_USEHINT = range(5)
G2 = {0: (Q - 1) // 88, 1: (Q - 1) // 32}
P_OF = {0: spec.PARAMS["ML-DSA-44"], 1: spec.PARAMS["ML-DSA-65"]}
I32 = (-2**31, 2**31)


@pytest.fixture(scope="module")
def probe():
    path = Path(__file__).resolve().parent / "libmldsa_arith_probe.so"
    assert path.exists(), f"{path} is missing: the default target of csrc/Makefile builds it"
    lib = ct.CDLL(str(path))
    P, SZ, LL, I = ct.c_void_p, ct.c_size_t, ct.c_longlong, ct.c_int
    lib.mldp_raw.argtypes = [I, I, SZ, P, P, P]
    lib.mldp_sweep.argtypes = [I, I, LL, LL, P]
    lib.mldp_ntt.argtypes = [I, I, P, P]
    lib.mldp_unpack.argtypes = [I, P, P]
    lib.mldp_rej.argtypes = [I, I, P, P, P]
    lib.mldp_sib.argtypes = [I, I, I, I, P, P, P]
    lib.mldp_hint.argtypes = [I, I, I, P, P, P]
    lib.mldp_w1.argtypes = [I, P, P]
    lib.mldp_tables.argtypes = [P]
    return lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(probe, op, arg, x, second=False):
    xd = _dev(np.asarray(x, np.int64).astype(np.int32))
    out = torch.zeros(len(x), dtype=torch.int32, device="cuda")
    out2 = torch.zeros(len(x), dtype=torch.int32, device="cuda")
    assert probe.mldp_raw(op, arg, len(x), xd.data_ptr(), out.data_ptr(), out2.data_ptr()) == 0
    o, o2 = out.cpu().numpy().astype(np.int64), out2.cpu().numpy().astype(np.int64)
    return (o, o2) if second else o


def sweep(probe, op, arg, lo, hi):
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert probe.mldp_sweep(op, arg, lo, hi, res.data_ptr()) == 0
    r = res.cpu().numpy()
    out = {"tested": int(r[0]), "bad": int(r[1]), "min_bad": int(r[2]), "max_bad": int(r[3])}
    print(f"sweep op={op} arg={arg} [{lo}, {hi}): {out}")
    assert out["tested"] == hi - lo
    return out


def edge(lo, hi, width=4096):
    return np.concatenate([np.arange(lo, lo + width), np.arange(-width, width), np.arange(hi - width, hi)])


def test_twiddles_are_derived_on_the_device(probe):
    out = torch.zeros(257, dtype=torch.float64, device="cuda")
    assert probe.mldp_tables(out.data_ptr()) == 0
    t = out.cpu().numpy()
    assert np.array_equal(t, np.rint(t)) and np.all(np.abs(t[:256]) <= (Q - 1) // 2)
    assert np.array_equal(t[:256].astype(np.int64) % Q, spec.ZETAS)
    assert int(t[256]) % Q == spec.INV256


# second factors: 1, the extreme twiddles, zeta, 256^-1 and a mid-size value
FACTORS = (1, -1, (Q - 1) // 2, -(Q - 1) // 2, 1753, -32736, 4808194 - Q, 2**22 - 1)


@pytest.mark.parametrize("b", FACTORS)
def test_modmul_over_every_int32_first_factor(probe, b):
    assert sweep(probe, OP_MODMUL, b, *I32)["bad"] == 0  # |a b| < 2^31 2^22 = 2^53: the stated domain, edges included
    x = edge(*I32)
    r = raw(probe, OP_MODMUL, b, x)
    assert np.all(np.abs(r) <= HALFQ) and np.array_equal(r % Q, x * b % Q)


def test_modmul_with_both_factors_at_the_ntt_output_bound(probe):
    """The pointwise products of the core kernel: both factors up to 5 q < 2^25.4 in magnitude."""
    bound = Q + 8 * HALFQ  # ntt_fwd's output bound for inputs below q
    assert bound < 2**25.4
    for b in (bound, -bound, bound - 1):
        assert sweep(probe, OP_MODMUL, b, -bound, bound + 1)["bad"] == 0
        x = edge(-bound, bound + 1)
        assert np.array_equal(raw(probe, OP_MODMUL, b, x) % Q, x * b % Q)


def test_reduce_and_canon(probe):
    assert sweep(probe, OP_REDUCE, 0, *I32)["bad"] == 0
    x = edge(*I32)
    r = raw(probe, OP_REDUCE, 0, x)
    assert np.all(np.abs(r) <= HALFQ) and np.array_equal(r % Q, x % Q)
    assert sweep(probe, OP_CANON, 0, -2 * Q + 1, 2 * Q)["bad"] == 0
    x = np.arange(-2 * Q + 1, 2 * Q, 997)
    assert np.array_equal(raw(probe, OP_CANON, 0, x), x % Q)


def test_the_device_comparator_counts_what_is_wrong(probe):
    """canon outside its stated domain is wrong, and the sweep must say so exactly where numpy does."""
    lo, hi = 2 * Q - 100, 2 * Q + 100
    x = np.arange(lo, hi)
    wrong = x[raw(probe, OP_CANON, 0, x) != x % Q]
    s = sweep(probe, OP_CANON, 0, lo, hi)
    assert len(wrong) == 100 and s["bad"] == 100 and (s["min_bad"], s["max_bad"]) == (int(wrong[0]), int(wrong[-1]))


@pytest.mark.parametrize("g", (0, 1))
def test_decompose_and_use_hint_for_every_r(probe, g):
    p = P_OF[g]
    assert sweep(probe, OP_DECOMPOSE, g, 0, Q)["bad"] == 0
    for h in (0, 1):
        assert sweep(probe, OP_USEHINT, g | (h << 1), 0, Q)["bad"] == 0
    # raw, straddling both ends of [0, q) and every multiple of gamma2 (where r0 and r1 change)
    x = np.unique(np.concatenate([np.arange(0, 2048), np.arange(Q - 2048, Q)] +
                                 [np.arange(m * G2[g] - 3, m * G2[g] + 4) for m in range(1, (Q - 1) // G2[g])]))
    r1, r0 = raw(probe, OP_DECOMPOSE, g, x, second=True)
    w1, w0 = spec.decompose(p, x)
    assert np.array_equal(r1, w1) and np.array_equal(r0, w0)
    for h in (0, 1):
        assert np.array_equal(raw(probe, OP_USEHINT, g | (h << 1), x), spec.use_hint(p, np.full_like(x, h), x))


def _ntt_inputs():
    rng = np.random.default_rng(204)
    spike = np.zeros((3, 256), dtype=np.int64)
    spike[0, 0], spike[1, 255], spike[2, 128] = 1, Q - 1, 1 << 22
    return np.concatenate([np.full((1, 256), Q - 1), np.zeros((1, 256), np.int64), spike,
                           rng.integers(0, Q, (3, 256))])


def test_ntt_forward_and_inverse_against_the_spec(probe):
    x = _ntt_inputs()
    out = torch.zeros(x.shape, dtype=torch.int32, device="cuda")
    assert probe.mldp_ntt(0, len(x), _dev(x.astype(np.int32)).data_ptr(), out.data_ptr()) == 0
    f = out.cpu().numpy().astype(np.int64)
    assert np.array_equal(f % Q, np.stack([spec.ntt(r) for r in x]))
    assert np.abs(f).max() <= Q - 1 + 8 * HALFQ  # the stated output bound
    print("ntt_fwd max |X| =", np.abs(f).max(), "bound", Q - 1 + 8 * HALFQ)
    # inverse of the unreduced forward outputs (what the core kernel's sums look like), and of inputs
    # at the stated input bound
    back = torch.zeros(x.shape, dtype=torch.int32, device="cuda")
    assert probe.mldp_ntt(1, len(x), out.data_ptr(), back.data_ptr()) == 0
    b = back.cpu().numpy().astype(np.int64)
    assert np.array_equal(b % Q, x % Q) and np.abs(b).max() <= HALFQ
    big = np.stack([np.full(256, 2**30 - 1), np.full(256, -(2**30 - 1)), np.where(np.arange(256) % 2, 2**30 - 1, 1 - 2**30)])
    assert probe.mldp_ntt(1, 3, _dev(big.astype(np.int32)).data_ptr(), back.data_ptr()) == 0
    b = back.cpu().numpy().astype(np.int64)[:3]
    assert np.array_equal(b % Q, np.stack([spec.ntt_inv(r) for r in big])) and np.abs(b).max() <= HALFQ


def test_bit_unpack_of_z_and_t1(probe):
    rng = np.random.default_rng(5)
    out = torch.zeros(256, dtype=torch.int32, device="cuda")
    for bits, gamma1 in ((18, 1 << 17), (20, 1 << 19)):
        for data in (bytes([255]) * (32 * bits), bytes(32 * bits), rng.integers(0, 256, 32 * bits, dtype=np.uint8).tobytes()):
            assert probe.mldp_unpack(bits, _dev(np.frombuffer(data, np.uint8)).data_ptr(), out.data_ptr()) == 0
            got = out.cpu().numpy().astype(np.int64)
            assert np.array_equal(got, spec.bit_unpack(data, gamma1 - 1, gamma1))
            assert got.min() >= -(gamma1 - 1) and got.max() <= gamma1
    for data in (bytes([255]) * 320, bytes(320), rng.integers(0, 256, 320, dtype=np.uint8).tobytes()):
        assert probe.mldp_unpack(10, _dev(np.frombuffer(data, np.uint8)).data_ptr(), out.data_ptr()) == 0
        got = out.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, spec.simple_bit_unpack(data, 1023) << 13) and got.max() <= Q - 1


class Bytes:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        self.pos += n
        out = self.data[self.pos - n:self.pos]
        return out + bytes(n - len(out))  # zeros once the stream runs out, as the probe delivers


def _cand(v):
    return bytes([v & 255, (v >> 8) & 255, v >> 16])


def test_rejection_sampler_on_crafted_streams(probe):
    rng = np.random.default_rng(7)
    nblocks = 7
    streams = []
    # 0: the edges q - 1 (accepted), q (rejected), 0x7FFFFF (rejected), and the ignored top bit
    edges = [Q - 1, Q, 0x7FFFFF, 0, (Q - 1) | 0x800000, Q | 0x800000, 0xFFFFFF, 1]
    streams.append(b"".join(_cand(v) for v in edges) + rng.integers(0, 256, 168 * nblocks, dtype=np.uint8).tobytes())
    # 1: 25 rejected candidates first, so 5 blocks (280 candidates) bring fewer than 256: a sixth block is needed
    streams.append(_cand(Q) * 25 + b"".join(_cand(int(v)) for v in rng.integers(0, Q, 56 * nblocks)))
    # 2: a whole block rejected; 3: random bytes (about 2^-10 rejected); 4: every candidate accepted
    streams.append(_cand(0x7FFFFF) * 56 + b"".join(_cand(int(v)) for v in rng.integers(0, Q, 56 * nblocks)))
    streams.append(rng.integers(0, 256, 168 * nblocks, dtype=np.uint8).tobytes())
    streams.append(b"".join(_cand(int(v)) for v in rng.integers(0, Q, 56 * nblocks)))
    data = b"".join(s[:168 * nblocks] for s in streams)
    coeffs = torch.full((len(streams), 256), -1, dtype=torch.int32, device="cuda")
    blocks = torch.zeros(len(streams), dtype=torch.int32, device="cuda")
    assert probe.mldp_rej(len(streams), nblocks, _dev(np.frombuffer(data, np.uint8)).data_ptr(), coeffs.data_ptr(),
                          blocks.data_ptr()) == 0
    got, used = coeffs.cpu().numpy(), blocks.cpu().numpy().tolist()
    for i, s in enumerate(streams):
        src = Bytes(s[:168 * nblocks])
        assert np.array_equal(got[i], spec.rej_ntt_poly_stream(src)), i
        assert used[i] == -(-src.pos // 168), i
    assert got[0][:4].tolist() == [Q - 1, 0, Q - 1, 1]
    assert used[1] == 6 and used[2] == 6 and used[4] == 5
    print("blocks used:", used)


@pytest.mark.parametrize("name", sorted(spec.PARAMS))
def test_sample_in_ball_for_the_fixture_ctilde_values(probe, name):
    p = spec.PARAMS[name]
    f = gold.load()[name]
    seeds = [s[:p.ctilde] for s in f["sigs"]] + [bytes(p.ctilde), bytes([255]) * p.ctilde]
    c = torch.full((len(seeds), 256), 9, dtype=torch.int8, device="cuda")
    blocks = torch.zeros(len(seeds), dtype=torch.int32, device="cuda")
    assert probe.mldp_sib(len(seeds), p.tau, p.ctilde, 0, _dev(np.frombuffer(b"".join(seeds), np.uint8)).data_ptr(),
                          c.data_ptr(), blocks.data_ptr()) == 0
    got = c.cpu().numpy().astype(np.int64)
    used = blocks.cpu().numpy().tolist()
    for i, s in enumerate(seeds):
        src = spec.Xof(256, s)
        want = spec.sample_in_ball(p, s, stream=src)
        assert np.array_equal(want, spec.sample_in_ball(p, s))
        assert np.array_equal(got[i], want) and np.count_nonzero(want) == p.tau
        assert used[i] == -(-src.pos // 136)


def test_sample_in_ball_reaches_a_second_block_on_crafted_bytes(probe):
    p = spec.PARAMS["ML-DSA-87"]
    rng = np.random.default_rng(11)
    nblocks = 3
    # row 0: 128 candidates of 255 (rejected while i < 255) use up the first block; row 1: random bytes
    rows = [bytes([0x5A] * 8) + bytes([255]) * 128 + rng.integers(0, 196, 136 * 2, dtype=np.uint8).tobytes(),
            rng.integers(0, 256, 136 * nblocks, dtype=np.uint8).tobytes()]
    c = torch.full((2, 256), 9, dtype=torch.int8, device="cuda")
    blocks = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert probe.mldp_sib(2, p.tau, 0, nblocks, _dev(np.frombuffer(b"".join(rows), np.uint8)).data_ptr(), c.data_ptr(),
                          blocks.data_ptr()) == 0
    got = c.cpu().numpy().astype(np.int64)
    used = blocks.cpu().numpy().tolist()
    for i, r in enumerate(rows):
        src = Bytes(r)
        assert np.array_equal(got[i], spec.sample_in_ball(p, b"", stream=src)), i
        assert used[i] == -(-src.pos // 136), i
    assert used[0] == 2


@pytest.mark.parametrize("name", sorted(spec.PARAMS))
def test_hint_bit_unpack_classes(probe, name):
    p = spec.PARAMS[name]
    f = gold.load()[name]
    hint = p.sig - p.omega - p.k
    rows = [s[hint:] for s in f["sigs"]]
    for e in f["tampers"]:
        if "set" in e or ("flip" in e and e["flip"][0] == "sig" and e["flip"][1] >= hint):
            rows.append(gold.apply_tamper(e, f["pk"], f["msgs"], f["sigs"])[2][hint:])
    full = np.zeros((p.k, 256), dtype=np.int64)
    full[p.k - 1][256 - p.omega:] = 1
    rows += [spec.hint_bit_pack(p, full), bytes(p.omega + p.k), bytes([255]) * (p.omega + p.k)]
    bits = torch.full((len(rows), 64), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((len(rows),), 9, dtype=torch.int32, device="cuda")
    assert probe.mldp_hint(p.k, p.omega, len(rows), _dev(np.frombuffer(b"".join(rows), np.uint8)).data_ptr(),
                           bits.data_ptr(), ok.data_ptr()) == 0
    got = bits.cpu().numpy().view(np.uint32)
    oks = ok.cpu().numpy().tolist()
    assert 0 in oks and 1 in oks
    for i, y in enumerate(rows):
        want = spec.hint_bit_unpack(p, y)
        assert oks[i] == (want is not None), i
        if want is not None:
            packed = np.packbits(want.astype(np.uint8), axis=1, bitorder="little").view(np.uint32)
            assert np.array_equal(got[i][:p.k * 8].reshape(p.k, 8), packed), i


@pytest.mark.parametrize("bits", (6, 4))
def test_w1_encode(probe, bits):
    top = 43 if bits == 6 else 15
    rng = np.random.default_rng(3)
    out = torch.zeros(32 * bits, dtype=torch.uint8, device="cuda")
    for w in (np.full(256, top), np.zeros(256, np.int64), rng.integers(0, top + 1, 256), np.arange(256) % (top + 1)):
        assert probe.mldp_w1(bits, _dev(w.astype(np.uint8)).data_ptr(), out.data_ptr()) == 0
        assert out.cpu().numpy().tobytes() == spec.simple_bit_pack(w, top)
