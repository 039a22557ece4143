"""The ML-KEM device primitives (csrc/mlkem_arith.cuh) alone, at the edges of their documented domains.

The kernels of mlkem.hip do their modular arithmetic in fp32 with exact-integer tricks whose
correctness rests on hand-derived input bounds; honest KeyGen / Encaps / Decaps on pseudo-random
coins essentially never reaches those bounds.  tests/mlkem_arith_probe.hip (its own shared object,
built by csrc/Makefile from the header the kernels include) runs each primitive as compiled for the
GPU:

  raw mode    outputs copied back and compared here with numpy int64 arithmetic, or with
              oracle/py/mlkem_spec.py for the NTTs and the base-case multiplication
  sweep mode  whole ranges compared on the device against plain 64-bit integer C++; every sweep
              operation also runs in raw mode on a sub-range (straddling the edge of its domain
              where it has one), and the device comparator must agree with numpy there

Figures (domain swept, mismatches, largest values seen) are printed; run with -s to see them.
"""
import ctypes as ct
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

Q = 3329
(OP_REDUCE, OP_MODMUL_F, OP_MODMUL_LF, OP_COMPRESS_F, OP_COMPRESS, OP_DECOMPRESS, OP_CANON_F, OP_I2F, OP_F2I,
 OP_F2BITS, OP_ACC_TO_F) = range(11)
FLOAT_OPS = {OP_REDUCE, OP_MODMUL_F, OP_MODMUL_LF, OP_I2F, OP_ACC_TO_F}
NTW = 258
# bounds the source states (mlkem_arith.cuh): ntt_fwd_f<false>, ntt_fwd_f<true>, ntt_inv_f outputs
FWD_BOUND, MIDRED_BOUND, INV_BOUND = 11658, 4 * 1665, 1665
ACC_BOUND = 4 * 2 * 3328 * 11658  # basemul_acc, k = 4


@pytest.fixture(scope="module")
def probe():
    path = Path(__file__).resolve().parent / "libmlkem_arith_probe.so"
    assert path.exists(), f"{path} is missing: the default target of csrc/Makefile builds it"
    lib = ct.CDLL(str(path))
    P, SZ, LL = ct.c_void_p, ct.c_size_t, ct.c_longlong
    lib.mlkp_raw.argtypes = [ct.c_int, ct.c_int, SZ, P, P, P]
    lib.mlkp_sweep.argtypes = [ct.c_int, ct.c_int, LL, LL, ct.c_int, ct.c_int, P]
    lib.mlkp_tables.argtypes = [P]
    lib.mlkp_decode12.argtypes = [ct.c_int, SZ, P, P, P]
    lib.mlkp_cbd.argtypes = [ct.c_int, SZ, P, P]
    lib.mlkp_ntt.argtypes = [ct.c_int, SZ, P, P]
    lib.mlkp_basemul.argtypes = [ct.c_int, ct.c_int, SZ, P, P, P, P]
    return lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def raw(probe, op, x, zi=None, d=0):
    """op over int64 inputs x (and twiddle indices zi) -> numpy float32 or int32 results."""
    x = np.asarray(x, np.int64)
    assert np.all(np.abs(x) < 2**31)
    xd = _dev(x.astype(np.int32))
    zd = _dev(np.asarray(zi, np.int32)) if zi is not None else None
    out = torch.zeros(len(x), dtype=torch.int32, device="cuda")
    rc = probe.mlkp_raw(op, d, len(x), xd.data_ptr(), zd.data_ptr() if zd is not None else None, out.data_ptr())
    assert rc == 0, rc
    o = _host(out)
    return o.view(np.float32) if op in FLOAT_OPS else o


def sweep(probe, op, lo, hi, z0=0, z1=1, d=0):
    res = torch.zeros(20, dtype=torch.int64, device="cuda")
    rc = probe.mlkp_sweep(op, d, lo, hi, z0, z1, res.data_ptr())
    assert rc == 0, rc
    r = _host(res)
    bad = int(r[1])
    return {"tested": int(r[0]), "bad": bad, "min_bad": int(r[2]) if bad else None,
            "max_bad": int(r[3]) if bad else None, "samples": [tuple(map(int, s)) for s in r[4:].reshape(8, 2)[:min(bad, 8)]]}


@pytest.fixture(scope="module")
def tables(probe):
    out = torch.zeros(386, dtype=torch.float32, device="cuda")
    assert probe.mlkp_tables(out.data_ptr()) == 0
    t = _host(out)
    tw = np.concatenate([t[:128], t[128:256], t[384:386]]).astype(np.int64)  # twiddle index -> value
    assert np.array_equal(tw, np.concatenate([t[:128], t[128:256], t[384:386]]))  # exact integers
    return t, tw


def _centered(x):
    x = np.asarray(x, np.int64) % Q
    return np.where(x > Q // 2, x - Q, x)


def centered_bad(r, want):
    """numpy restatement of the device comparator: an exact integer, |r| <= 1665, r = want (mod q)."""
    r = r.astype(np.float64)
    ri = np.rint(r).astype(np.int64)
    ok = (ri == r) & (np.abs(ri) <= 1665) & ((np.asarray(want, np.int64) - ri) % Q == 0)
    return ~ok


def compress_ref(d, x):
    x = np.asarray(x, np.int64) % Q
    return (((x << d) + Q // 2) // Q) & ((1 << d) - 1)


def numpy_bad(op, x, got, d=0, z=None):
    x = np.asarray(x, np.int64)
    if op in (OP_REDUCE, OP_ACC_TO_F):
        return centered_bad(got, x)
    if op in (OP_MODMUL_F, OP_MODMUL_LF):
        return centered_bad(got, x * z)
    if op == OP_COMPRESS_F:
        return got.astype(np.int64) != compress_ref(d, x)
    if op == OP_CANON_F:
        return got.astype(np.int64) != x % Q
    if op == OP_I2F:
        return got.astype(np.float64) != x
    if op == OP_F2I:
        return got.astype(np.int64) != x
    raise AssertionError(op)


def cross_check(probe, op, lo, hi, d=0):
    """The device comparator against numpy on [lo, hi]: the same mismatch count and extremes."""
    x = np.arange(lo, hi + 1, dtype=np.int64)
    bad = numpy_bad(op, x, raw(probe, op, x, d=d), d=d)
    s = sweep(probe, op, lo, hi, d=d)
    assert s["tested"] == len(x)
    assert s["bad"] == int(bad.sum()), (op, lo, hi, s, int(bad.sum()))
    if s["bad"]:
        assert (s["min_bad"], s["max_bad"]) == (int(x[bad].min()), int(x[bad].max()))
        assert all(bad[sx - lo] for sx, _ in s["samples"])
    return s


def test_probe_rejects_bad_arguments(probe):
    """Every entry validates its sizes and returns an error code instead of launching."""
    buf = torch.zeros(1024, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    assert probe.mlkp_raw(99, 0, 4, p, p, p) == -1
    assert probe.mlkp_raw(OP_REDUCE, 0, 0, p, None, p) == -1
    assert probe.mlkp_raw(OP_REDUCE, 0, (1 << 22) + 1, p, None, p) == -1
    assert probe.mlkp_raw(OP_REDUCE, 0, 4, None, None, p) == -1
    assert probe.mlkp_raw(OP_MODMUL_F, 0, 4, p, None, p) == -1
    assert probe.mlkp_raw(OP_COMPRESS_F, 7, 4, p, None, p) == -1
    assert probe.mlkp_sweep(OP_REDUCE, 0, 5, 4, 0, 1, p) == -1
    assert probe.mlkp_sweep(OP_REDUCE, 0, 0, 1 << 31, 0, 1, p) == -1
    assert probe.mlkp_sweep(OP_MODMUL_F, 0, 0, 4, 0, NTW + 1, p) == -1
    assert probe.mlkp_sweep(OP_COMPRESS, 4, 0, 4, 0, 1, p) == -1
    assert probe.mlkp_sweep(OP_REDUCE, 0, 0, 4, 0, 1, None) == -1
    assert probe.mlkp_tables(None) == -1
    assert probe.mlkp_decode12(3, 4, p, p, p) == -1
    assert probe.mlkp_decode12(1, 4, p, p, None) == -1
    assert probe.mlkp_cbd(4, 4, p, p) == -1
    assert probe.mlkp_ntt(5, 1, p, p) == -1
    assert probe.mlkp_ntt(0, 0, p, p) == -1
    assert probe.mlkp_basemul(0, 5, 1, p, p, p, p) == -1
    assert probe.mlkp_basemul(2, 4, 1, p, p, p, p) == -1


def test_tables_match_spec(tables):
    import mlkem_spec as spec
    t, tw = tables
    assert np.array_equal(tw[:128], _centered(spec.ZETAS))
    assert np.array_equal(tw[128:256], _centered(spec.GAMMAS))
    assert tw[256] == -26 and tw[257] == _centered(spec.ZETAS[1] * 3303)
    assert np.array_equal(t[256:384], (t[:128].astype(np.float64) / 3329.0).astype(np.float32))


def test_reduce_f_full_domain(probe):
    """Every integer |x| < 2^24: an integer, congruent to x, |r| <= 1665."""
    m = (1 << 24) - 1
    s = sweep(probe, OP_REDUCE, -m, m)
    print(f"reduce_f: |x| < 2^24, {s['tested']} inputs, {s['bad']} mismatches {s['samples']}")
    assert s["tested"] == 2 * m + 1 and s["bad"] == 0, s
    # raw mode at both ends of the domain, around zero and around the first multiples of q / 2
    for lo, hi in [(-m, -m + 70000), (m - 70000, m), (-70000, 70000)]:
        assert cross_check(probe, OP_REDUCE, lo, hi)["bad"] == 0
    # past the domain (fp32 no longer holds every integer): comparator and numpy still agree
    s = cross_check(probe, OP_REDUCE, m - 1000, m + 200000)
    print(f"reduce_f past 2^24: {s['bad']} mismatches, first {s['min_bad']}")


@pytest.mark.parametrize("op,name", [(OP_MODMUL_F, "modmul_f"), (OP_MODMUL_LF, "modmul_lf")])
def test_modmul_every_twiddle(probe, tables, op, name):
    """Every x in [-10081, 10081] against the 128 zeta, 128 gamma, INV128F and Z1INV128F, pairs with
    |x z| < 2^24: congruent to x z, |r| <= 1665."""
    _, tw = tables
    X = 10081
    x = np.arange(-X, X + 1, dtype=np.int64)
    in_domain = np.abs(x[None, :] * tw[:, None]) < (1 << 24)
    s = sweep(probe, op, -X, X, 0, NTW)
    print(f"{name}: x in [-{X}, {X}] x {NTW} twiddles, {s['tested']} pairs inside |x z| < 2^24 "
          f"(of {in_domain.size}), {s['bad']} mismatches {s['samples']}")
    assert s["tested"] == int(in_domain.sum()) and s["bad"] == 0, s
    assert in_domain[np.abs(tw) <= 1664].all()  # |z| <= 1664: the whole x range is inside the domain
    # raw mode: the outer 1100 values of x on both sides, every twiddle, checked with numpy
    xe = np.concatenate([np.arange(-X, -X + 1100), np.arange(X - 1099, X + 1)])
    xx, zz = np.meshgrid(xe, np.arange(NTW))
    xx, zz = xx.ravel(), zz.ravel()
    keep = np.abs(xx * tw[zz]) < (1 << 24)
    xx, zz = xx[keep], zz[keep]
    got = raw(probe, op, xx, zz)
    bad = centered_bad(got, xx * tw[zz])
    assert not bad.any(), (xx[bad][:8], zz[bad][:8], got[bad][:8])
    # the device comparator on the same sub-range, one twiddle class at a time
    for z0, z1 in [(0, 128), (128, 256), (256, 258)]:
        for lo, hi in [(-X, -X + 1099), (X - 1099, X)]:
            sw = sweep(probe, op, lo, hi, z0, z1)
            want = int((np.abs(np.arange(lo, hi + 1)[None, :] * tw[z0:z1, None]) < (1 << 24)).sum())
            assert sw["tested"] == want and sw["bad"] == 0, sw


@pytest.mark.parametrize("d", [1, 4, 5, 10, 11])
def test_compress_decompress(probe, d):
    """compress_f<D> on every v in [-4091, 4091] (no reduction first), compress<D> on [0, q),
    decompress<D> on [0, 2^D), against round(2^D (v mod q) / q) mod 2^D."""
    v = np.arange(-4091, 4092, dtype=np.int64)
    got = raw(probe, OP_COMPRESS_F, v, d=d).astype(np.int64)
    bad = got != compress_ref(d, v)
    print(f"compress_f<{d}>: v in [-4091, 4091], {int(bad.sum())} mismatches {v[bad][:8]}")
    assert not bad.any(), (v[bad][:8], got[bad][:8])
    s = cross_check(probe, OP_COMPRESS_F, -4091, 4091, d=d)
    assert s["bad"] == 0
    # past the stated bound the comparator and numpy still agree (whatever the count is)
    cross_check(probe, OP_COMPRESS_F, -3 * Q, 3 * Q, d=d)
    x = np.arange(Q, dtype=np.int64)
    assert np.array_equal(raw(probe, OP_COMPRESS, x, d=d), compress_ref(d, x))
    y = np.arange(1 << d, dtype=np.int64)
    dec = raw(probe, OP_DECOMPRESS, y, d=d).astype(np.int64)
    assert np.array_equal(dec, (Q * y + (1 << (d - 1))) >> d)
    assert np.array_equal(compress_ref(d, dec), y)  # Compress_d(Decompress_d(y)) = y (FIPS 203 4.2.1)


def test_canon_and_int_float_conversions(probe):
    m24, m22 = (1 << 24) - 1, (1 << 22) - 1
    for op, name, m in [(OP_CANON_F, "canon_f", m24), (OP_I2F, "i2f", m22), (OP_F2I, "f2i", m22)]:
        s = sweep(probe, op, -m, m)
        print(f"{name}: |x| <= {m}, {s['tested']} inputs, {s['bad']} mismatches {s['samples']}")
        assert s["tested"] == 2 * m + 1 and s["bad"] == 0, (name, s)
        for lo, hi in [(-m, -m + 50000), (-50000, 50000), (m - 50000, m)]:
            assert cross_check(probe, op, lo, hi)["bad"] == 0
    # i2f / f2i past 2^22 (outside their domain): comparator and numpy agree
    cross_check(probe, OP_I2F, m22 - 100, m22 + 50000)
    cross_check(probe, OP_F2I, -m22 - 50000, -m22 + 100)
    # f2bits: the low 16 bits are x as int16 (make_bop_f packs them)
    x = np.arange(-32768, 32768, dtype=np.int64)
    assert np.array_equal(raw(probe, OP_F2BITS, x).astype(np.int64), x & 0xFFFF)


def test_acc_to_f_domain_and_first_failure(probe):
    """Every |acc| <= 2^29 (the kernels' analytic worst case is 4 * 2 * 3328 * 11658 = 3.10e8) is
    reduced exactly.  Control: acc_to_f is not exact on all of int32 -- lo - 1044 hi leaves fp32's
    exact-integer range at hi = 16071 -- so the sweep over [1 053 229 000, 1 053 230 000] must report
    mismatches; a plain-C IEEE model puts the first at 1 053 229 057 and, on the negative side, at
    -1 049 034 753."""
    m = 1 << 29
    s = sweep(probe, OP_ACC_TO_F, -m, m)
    print(f"acc_to_f: |acc| <= 2^29, {s['tested']} inputs, {s['bad']} mismatches {s['samples']}")
    assert s["tested"] == 2 * m + 1 and s["bad"] == 0, s
    for lo, hi in [(-m, -m + 60000), (-70000, 70000), (m - 60000, m), (ACC_BOUND - 60000, ACC_BOUND + 60000),
                   (-ACC_BOUND - 60000, -ACC_BOUND + 60000)]:
        assert cross_check(probe, OP_ACC_TO_F, lo, hi)["bad"] == 0
    pos = cross_check(probe, OP_ACC_TO_F, 1_053_229_000, 1_053_230_000)
    neg = cross_check(probe, OP_ACC_TO_F, -1_049_035_753, -1_049_033_753)
    print(f"acc_to_f control: first failing acc on the GPU +{pos['min_bad']} ({pos['bad']} in the range; "
          f"CPU model +1053229057), {neg['max_bad']} ({neg['bad']} in the range; CPU model -1049034753)")
    assert pos["bad"] >= 1, "the comparator cannot fail"
    assert pos["min_bad"] == 1_053_229_057
    assert neg["bad"] >= 1 and neg["max_bad"] == -1_049_034_753
    # nothing fails between the swept range and those first failures either (one more sweep each side)
    assert sweep(probe, OP_ACC_TO_F, m, 1_053_229_056)["bad"] == 0
    assert sweep(probe, OP_ACC_TO_F, -1_049_034_752, -m)["bad"] == 0


def _pack12(fields):
    """[n, 16] 12-bit fields -> [n, 3] uint64 (ByteEncode_12 of a lane's 24 bytes)."""
    f = np.asarray(fields, np.uint32)
    a, b = f[:, 0::2], f[:, 1::2]
    by = np.stack([a & 0xFF, (a >> 8) | ((b & 0xF) << 4), b >> 4], axis=2).astype(np.uint8)
    return np.ascontiguousarray(by.reshape(len(f), 24)).view(np.uint64)


def test_decode12_every_field_every_value(probe):
    """Every 12-bit value in each of a lane's 16 positions, the other positions zero and 0xFFF:
    split12 / unpack12 return the fields, decode12_w returns v mod q (FIPS 203 Alg. 6) and sets
    `bad` exactly when some field is >= q."""
    rows = []
    for fill in (0, 0xFFF, Q - 1):
        f = np.full((16, 4096, 16), fill, np.int64)
        for p in range(16):
            f[p, :, p] = np.arange(4096)
        rows.append(f.reshape(-1, 16))
    fields = np.concatenate(rows)
    n = len(fields)
    src = _dev(_pack12(fields))
    out = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
    bad = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for mode, want in [(0, fields), (2, fields), (1, fields % Q)]:
        out.zero_()
        assert probe.mlkp_decode12(mode, n, src.data_ptr(), out.data_ptr(), bad.data_ptr()) == 0
        got = _host(out).astype(np.int64)
        assert np.array_equal(got, want), (mode, np.argwhere(got != want)[:4])
    assert np.array_equal(_host(bad), (fields >= Q).any(axis=1).astype(np.int32))
    third = fields[2 * 16 * 4096:]  # fill q - 1: the flag follows the one varying field alone
    assert np.array_equal(_host(bad)[2 * 16 * 4096:], (third.max(axis=1) >= Q).astype(np.int32))
    print(f"split12 / unpack12 / decode12_w: {n} lanes, 0 mismatches")


@pytest.mark.parametrize("eta", [2, 3])
def test_cbd_every_field_every_value(probe, eta):
    """Every value of every 2 eta-bit field (the others zero / all ones), words of all ones, and a
    random PRF output against the spec's SamplePolyCBD."""
    import mlkem_spec as spec
    w = 2 * eta  # bits per coefficient
    rows = []
    for fill in (0, (1 << w) - 1):
        f = np.full((16, 1 << w, 16), fill, np.int64)
        for p in range(16):
            f[p, :, p] = np.arange(1 << w)
        rows.append(f.reshape(-1, 16))
    rows.append(np.full((1, 16), (1 << w) - 1, np.int64))
    fields = np.concatenate(rows)
    bits = np.zeros(len(fields), dtype=object)
    for t in range(16):
        bits += fields[:, t].astype(object) << (w * t)
    words = np.array([[(int(b) >> (32 * i)) & 0xFFFFFFFF for i in range(3)] for b in bits], np.uint32)
    rng = np.random.default_rng(eta)
    B = rng.integers(0, 256, 64 * eta, dtype=np.uint8).tobytes()
    lanes = np.zeros((16, 3), np.uint32)
    lanes[:, :w * 16 // 32] = np.frombuffer(B, np.uint32).reshape(16, -1)  # lane L: coefficients 16L .. 16L+15
    words = np.concatenate([words, lanes])
    if eta == 2:
        words[:len(fields), 2] = 0xFFFFFFFF  # eta = 2 reads two words; the third must not matter
    out = torch.zeros((len(words), 16), dtype=torch.float32, device="cuda")
    assert probe.mlkp_cbd(eta, len(words), _dev(words).data_ptr(), out.data_ptr()) == 0
    got = _host(out)

    def popc(v):
        return sum((v >> i) & 1 for i in range(eta))
    want = popc(fields) - popc(fields >> eta)
    assert np.array_equal(got[:len(fields)], want.astype(np.float32))
    assert np.array_equal(got[len(fields):].reshape(256), _centered(spec.sample_cbd(eta, B)).astype(np.float32))


# ---------------------------------------------------------------------------- NTT inputs
def _greedy_signs():
    """A sign pattern that follows each twiddle's sign, layer by layer: wherever the product
    zeta * f[j + len] (centered, as modmul_f returns it) opposes f[j], the inputs feeding f[j + len]
    are flipped, so the sums f[j] + t keep growing.  Flips reach earlier butterflies of the same
    residue class, so the pattern is a heuristic: its growth is whatever the device shows."""
    import mlkem_spec as spec
    s = np.ones(256, np.int64)
    cur = np.ones(256, np.int64) * 3
    i, length = 1, 128
    while length >= 2:
        for start in range(0, 256, 2 * length):
            z = spec.ZETAS[i]
            i += 1
            for j in range(start, start + length):
                t = int(_centered(z * cur[j + length]))
                if t * cur[j] < 0:
                    s[np.arange(256) % (2 * length) == (j + length) % (2 * length)] *= -1
                    t, cur[j + length] = -t, -cur[j + length]
                cur[j], cur[j + length] = cur[j] + t, cur[j] - t
        length //= 2
    return s


def _signed_polys(amp, seed):
    """|f| <= amp: both constants, alternating signs at every power-of-two period, the greedy
    pattern (and its negative), 256 seeded random polynomials (half of them at +-amp only)."""
    j = np.arange(256)
    polys = [np.full(256, amp), np.full(256, -amp)]
    for p in (1, 2, 4, 8, 16, 32, 64, 128):
        alt = np.where((j // p) % 2 == 0, amp, -amp)
        polys += [alt, -alt]
    g = _greedy_signs() * amp
    polys += [g, -g]
    rng = np.random.default_rng(seed)
    polys += list(rng.integers(-amp, amp + 1, (128, 256)))
    polys += list(rng.choice([-amp, amp], (128, 256)))
    return np.array(polys, np.int64)


def _unsigned_polys(seed):
    """f in [0, q]: the constants 0 and q, 0 / q (and 0 / every Decompress maximum) alternating at
    every power-of-two period, 256 seeded random polynomials."""
    j = np.arange(256)
    tops = [Q] + [(Q * ((1 << d) - 1) + (1 << (d - 1))) >> d for d in (10, 11, 4, 5)]
    polys = [np.zeros(256, np.int64)]
    for top in tops:
        polys.append(np.full(256, top))
        for p in (1, 2, 4, 8, 16, 32, 64, 128):
            alt = np.where((j // p) % 2 == 0, top, 0)
            polys += [alt, top - alt]
    g = _greedy_signs()
    polys += [np.where(g > 0, Q, 0), np.where(g > 0, 0, Q)]
    rng = np.random.default_rng(seed)
    polys += list(rng.integers(0, Q + 1, (128, 256)))
    polys += list(rng.choice([0, Q], (128, 256)))
    return np.array(polys, np.int64)


def run_ntt(probe, mode, polys):
    out = torch.zeros(polys.shape, dtype=torch.float32, device="cuda")
    assert probe.mlkp_ntt(mode, len(polys), _dev(polys.astype(np.float32)).data_ptr(), out.data_ptr()) == 0
    got = _host(out)
    gi = np.rint(got).astype(np.int64)
    assert np.array_equal(gi, got), "NTT outputs are not exact integers"
    return gi


@pytest.fixture(scope="module")
def ntt_cases(probe):
    """The forward-NTT inputs, their device outputs and the spec's transforms, computed once."""
    import mlkem_spec as spec
    cbd = _signed_polys(3, seed=203)
    dec = _unsigned_polys(seed=204)
    return {
        "cbd": cbd, "cbd_hat": np.array([spec.ntt(list(map(int, f % Q))) for f in cbd], np.int64),
        "dec": dec, "dec_hat": np.array([spec.ntt(list(map(int, f % Q))) for f in dec], np.int64),
    }


def test_ntt_forward_plain_worst_cases(probe, ntt_cases):
    """ntt_fwd_f<false> on |f| <= 3: congruent to the spec's NTT, |output| <= 11658."""
    f = ntt_cases["cbd"]
    got = run_ntt(probe, 0, f)
    assert np.array_equal(got % Q, ntt_cases["cbd_hat"])
    print(f"ntt_fwd_f<false>: {len(f)} polynomials with |f| <= 3, largest |output| {np.abs(got).max()} "
          f"(bound {FWD_BOUND}; greedy pattern {np.abs(got[18]).max()})")
    assert np.abs(got).max() <= FWD_BOUND
    back = run_ntt(probe, 3, f)
    assert np.array_equal(back % Q, f % Q) and np.abs(back).max() <= INV_BOUND


def test_ntt_forward_midred_worst_cases(probe, ntt_cases):
    """ntt_fwd_f<true> on f in [0, q] (every Decompress maximum included): congruent to the spec,
    |output| <= 4 * 1665."""
    f = ntt_cases["dec"]
    got = run_ntt(probe, 1, f)
    assert np.array_equal(got % Q, ntt_cases["dec_hat"])
    print(f"ntt_fwd_f<true>: {len(f)} polynomials in [0, q], largest |output| {np.abs(got).max()} (bound {MIDRED_BOUND})")
    assert np.abs(got).max() <= MIDRED_BOUND
    back = run_ntt(probe, 4, f)
    assert np.array_equal(back % Q, f % Q) and np.abs(back).max() <= INV_BOUND


def test_ntt_inverse_worst_cases(probe):
    """ntt_inv_f on |f| <= 1665: congruent to the spec's inverse NTT, |output| <= 1665."""
    import mlkem_spec as spec
    f = np.concatenate([_signed_polys(1665, seed=205), _signed_polys(1664, seed=206)[:20]])
    got = run_ntt(probe, 2, f)
    want = np.array([spec.ntt_inv(list(map(int, p % Q))) for p in f], np.int64)
    assert np.array_equal(got % Q, want)
    print(f"ntt_inv_f: {len(f)} polynomials with |f| <= 1665, largest |output| {np.abs(got).max()} (bound {INV_BOUND})")
    assert np.abs(got).max() <= INV_BOUND


@pytest.mark.parametrize("midred", [0, 1])
def test_basemul_accumulated_over_four_terms(probe, ntt_cases, midred):
    """make_bop_f, basemul_acc summed over k = 4 terms, acc_to_f: a all 3328, all 0, alternating
    0 / 3328 and random in [0, q); b = the forward NTT of the extreme inputs above (plain for
    KeyGen / Encaps, MIDRED for Decaps).  Congruent to the spec's MultiplyNTTs summed over the
    terms; |acc| inside the bound the source derives."""
    import mlkem_spec as spec
    b_all, bhat_all = (ntt_cases["dec"], ntt_cases["dec_hat"]) if midred else (ntt_cases["cbd"], ntt_cases["cbd_hat"])
    rng = np.random.default_rng(207 + midred)
    n_ext = len(b_all) - 256  # the structured cases come first
    pick = [[i] * 4 for i in range(n_ext)] + [list(rng.integers(0, len(b_all), 4)) for _ in range(24)]
    j = np.arange(256)
    a_pat = [np.full(256, 3328), np.zeros(256, np.int64), np.where(j % 2 == 0, 0, 3328), np.where(j % 2 == 0, 3328, 0)]
    a_rows, b_idx = [], []
    for r, idx in enumerate(pick):
        for ap in a_pat if r < n_ext else []:
            a_rows.append(np.stack([ap] * 4))
            b_idx.append(idx)
        a_rows.append(rng.integers(0, Q, (4, 256)))
        b_idx.append(idx)
    a = np.array(a_rows, np.int64)
    b_idx = np.array(b_idx)
    n = len(a)
    acc = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
    res = torch.zeros((n, 256), dtype=torch.float32, device="cuda")
    assert probe.mlkp_basemul(midred, 4, n, _dev(a.astype(np.int32)).data_ptr(),
                              _dev(b_all[b_idx].astype(np.float32)).data_ptr(), acc.data_ptr(), res.data_ptr()) == 0
    acc, res = _host(acc).astype(np.int64), _host(res)
    want = np.zeros((n, 256), np.int64)
    for r in range(n):
        for t in range(4):
            want[r] += spec.multiply_ntts(list(map(int, a[r, t])), list(map(int, bhat_all[b_idx[r, t]])))
    want %= Q
    assert np.array_equal(acc % Q, want)
    assert not centered_bad(res, want).any()
    print(f"basemul (MIDRED={midred}): {n} rows of k = 4 terms, largest |acc| {np.abs(acc).max()} "
          f"(derived bound {ACC_BOUND}, acc_to_f swept to {1 << 29})")
    assert np.abs(acc).max() <= ACC_BOUND
