// Test-only device probe of the ML-KEM primitives in csrc/mlkem_arith.cuh.
//
// Built by csrc/Makefile into tests/libmlkem_arith_probe.so with the library's flags; it includes
// the header the kernels of mlkem.hip include, so it runs the functions the kernels compile, not
// copies of them.  Not part of libqrkem.so and not part of the qrkem package.
//
// Every entry takes device pointers, launches on the default stream, synchronises and returns 0,
// -1 for a bad argument (nothing is launched) or -2 for a HIP error.
//
//   raw mode    outputs are written to device arrays and checked on the host (numpy / the spec)
//   sweep mode  whole ranges checked on the device against plain 64-bit integer arithmetic
//               (`%`, no floats); returns the mismatch count, the smallest and the largest
//               mismatching input and a few samples
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "mlkem_arith.cuh"

using namespace qrk::mlkem;

namespace {

constexpr size_t RAW_MAX = (size_t)1 << 22;  // raw-mode rows per call

enum Op : int {
  OP_REDUCE = 0,      // float reduce_f((float)x)
  OP_MODMUL_F = 1,    // float modmul_f((float)x, tw[zi], fl(tw[zi] / q))
  OP_MODMUL_LF = 2,   // float modmul_lf((float)x, tw[zi])
  OP_COMPRESS_F = 3,  // int   compress_f<D>((float)x)
  OP_COMPRESS = 4,    // int   compress<D>(x)
  OP_DECOMPRESS = 5,  // int   decompress<D>(x)
  OP_CANON_F = 6,     // int   canon_f((float)x)
  OP_I2F = 7,         // float i2f(x)
  OP_F2I = 8,         // int   f2i((float)x)
  OP_F2BITS = 9,      // int   f2bits((float)x) & 0xFFFF
  OP_ACC_TO_F = 10,   // float acc_to_f(x)
  OP_COUNT = 11
};
constexpr int NTW = 258;  // twiddles: 128 zeta, 128 gamma, INV128F, Z1INV128F

// twiddle zi and its z / q constant, from the tables the kernels read
__device__ __forceinline__ void twiddle(int zi, float& z, float& zq) {
  if (zi < 128) {
    z = TABFD.z[zi], zq = TABFD.zq[zi];
  } else {
    z = zi < 256 ? TABFD.g[zi - 128] : (zi == 256 ? INV128F : Z1INV128F);
    zq = (float)((double)z / 3329.0);
  }
}

template <int D>
__device__ __forceinline__ int by_d(int op, int x) {
  if (op == OP_COMPRESS_F) return compress_f<D>((float)x);
  if (op == OP_COMPRESS) return compress<D>(x);
  return decompress<D>(x);
}

// one primitive on one input; float results are returned as their bit pattern
__device__ __forceinline__ uint32_t eval(int op, int d, int x, int zi) {
  float z, zq;
  switch (op) {
    case OP_REDUCE:
      return __float_as_uint(reduce_f((float)x));
    case OP_MODMUL_F:
      twiddle(zi, z, zq);
      return __float_as_uint(modmul_f((float)x, z, zq));
    case OP_MODMUL_LF:
      twiddle(zi, z, zq);
      return __float_as_uint(modmul_lf((float)x, z));
    case OP_COMPRESS_F:
    case OP_COMPRESS:
    case OP_DECOMPRESS:
      switch (d) {
        case 1: return (uint32_t)by_d<1>(op, x);
        case 4: return (uint32_t)by_d<4>(op, x);
        case 5: return (uint32_t)by_d<5>(op, x);
        case 10: return (uint32_t)by_d<10>(op, x);
        default: return (uint32_t)by_d<11>(op, x);
      }
    case OP_CANON_F:
      return (uint32_t)canon_f((float)x);
    case OP_I2F:
      return __float_as_uint(i2f(x));
    case OP_F2I:
      return (uint32_t)f2i((float)x);
    case OP_F2BITS:
      return f2bits((float)x) & 0xFFFFu;
    default:
      return __float_as_uint(acc_to_f(x));
  }
}

__device__ __forceinline__ long long mod_q(long long x) {
  const long long r = x % Q;
  return r < 0 ? r + Q : r;
}
// an exact integer r with |r| <= 1665 and r = want (mod q)
__device__ __forceinline__ bool centered_ok(float r, long long want) {
  if (!(r >= -1665.0f && r <= 1665.0f)) return false;
  const long long ri = (long long)r;
  return (float)ri == r && mod_q(want - ri) == 0;
}
// the device comparator: plain 64-bit integers
__device__ __forceinline__ bool check(int op, int d, long long x, float z, uint32_t got) {
  switch (op) {
    case OP_REDUCE:
    case OP_ACC_TO_F:
      return centered_ok(__uint_as_float(got), x);
    case OP_MODMUL_F:
    case OP_MODMUL_LF:
      return centered_ok(__uint_as_float(got), x * (long long)z);
    case OP_COMPRESS_F:
      return (long long)got == ((((mod_q(x) << d) + Q / 2) / Q) & ((1ll << d) - 1));
    case OP_CANON_F:
      return (long long)got == mod_q(x);
    case OP_I2F:
      return __uint_as_float(got) == (float)x && (long long)__uint_as_float(got) == x;
    case OP_F2I:
      return (long long)(int)got == x;
    default:
      return false;
  }
}

bool d_ok(int op, int d) {
  if (op != OP_COMPRESS_F && op != OP_COMPRESS && op != OP_DECOMPRESS) return true;
  return d == 1 || d == 4 || d == 5 || d == 10 || d == 11;
}

__global__ __launch_bounds__(256) void k_raw(int op, int d, size_t n, const int32_t* __restrict__ x,
                                             const int32_t* __restrict__ zi, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int z = zi ? zi[i] : 0;
  z = z < 0 ? 0 : (z >= NTW ? NTW - 1 : z);
  out[i] = eval(op, d, x[i], z);
}

struct SweepOut {
  unsigned long long tested, bad;
  long long min_bad, max_bad;  // smallest / largest mismatching x
  long long sample[8][2];      // (x, twiddle index) of the first mismatches to arrive
};

// x in [lo, hi] against twiddles [z0, z1) (one twiddle for the unary ops); modmul pairs with
// |x z| >= 2^24 are outside the documented domain and skipped
__global__ __launch_bounds__(256) void k_sweep(int op, int d, long long lo, long long hi, int z0, int z1,
                                               SweepOut* __restrict__ o) {
  const unsigned long long nx = (unsigned long long)(hi - lo) + 1, total = nx * (unsigned)(z1 - z0);
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  unsigned long long tested = 0, bad = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const long long x = lo + (long long)(i % nx);
    const int zi = z0 + (int)(i / nx);
    float z = 0.0f, zq;
    if (op == OP_MODMUL_F || op == OP_MODMUL_LF) {
      twiddle(zi, z, zq);
      const long long p = x * (long long)z;
      if (p >= (1ll << 24) || p <= -(1ll << 24)) continue;
    }
    ++tested;
    if (!check(op, d, x, z, eval(op, d, (int)x, zi))) {
      ++bad;
      atomicMin(&o->min_bad, x);
      atomicMax(&o->max_bad, x);
    }
  }
  // few mismatches are expected: per-thread counters, then one atomic each
  if (tested) atomicAdd(&o->tested, tested);
  if (bad) {
    const unsigned long long slot = atomicAdd(&o->bad, bad);
    if (slot < 8) {
      // this thread's first mismatch again, for the sample list
      for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long x = lo + (long long)(i % nx);
        const int zi = z0 + (int)(i / nx);
        float z = 0.0f, zq;
        if (op == OP_MODMUL_F || op == OP_MODMUL_LF) {
          twiddle(zi, z, zq);
          const long long p = x * (long long)z;
          if (p >= (1ll << 24) || p <= -(1ll << 24)) continue;
        }
        if (!check(op, d, x, z, eval(op, d, (int)x, zi))) {
          o->sample[slot][0] = x, o->sample[slot][1] = zi;
          break;
        }
      }
    }
  }
}

__global__ void k_tables(float* __restrict__ out) {  // z[128] g[128] zq[128] INV128F Z1INV128F
  const int i = threadIdx.x;
  if (i < 128) out[i] = TABFD.z[i], out[128 + i] = TABFD.g[i], out[256 + i] = TABFD.zq[i];
  if (i == 0) out[384] = INV128F, out[385] = Z1INV128F;
}

// mode 0: split12 twice, 1: decode12_w (+ bad), 2: unpack12; out[i][16], one lane per row
__global__ __launch_bounds__(256) void k_dec12(int mode, size_t n, const uint64_t* __restrict__ in,
                                               int32_t* __restrict__ out, int32_t* __restrict__ bad_out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = in[3 * i], b = in[3 * i + 1], c = in[3 * i + 2];
  int v[16];
  if (mode == 0) {
    split12((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, v);
    split12((uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), v + 8);
  } else {
    PK8 r;
    if (mode == 1) {
      bool bad = false;
      r = decode12_w(a, b, c, bad);
      bad_out[i] = bad ? 1 : 0;
    } else {
      const U3 u{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b}, w{(uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
      r = unpack12(u, w);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) v[2 * t] = (int)(r.w[t] & 0xFFFFu), v[2 * t + 1] = (int)(r.w[t] >> 16);
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) out[16 * i + t] = v[t];
}

template <int ETA>
__global__ __launch_bounds__(256) void k_cbd(size_t n, const uint32_t* __restrict__ in, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  CbdRaw r;
  r.d[0] = in[3 * i], r.d[1] = in[3 * i + 1], r.d[2] = in[3 * i + 2];
  PF16 p;
  cbd_f<ETA>(p, r);
#pragma unroll
  for (int t = 0; t < 16; ++t) out[16 * i + t] = p.v[t];
}

// ---- 16-lane groups, one polynomial (or one basemul row) per group, 16 groups per workgroup
constexpr int GROUPS = 16, PBUF = 272;

__device__ __forceinline__ PF16 load_stride(const float* __restrict__ f, int L) {
  PF16 p;
#pragma unroll
  for (int m = 0; m < 16; ++m) p.v[m] = f[L + 16 * m];
  return p;
}
__device__ __forceinline__ PF16 load_contig(const float* __restrict__ f, int L) {
  PF16 p;
#pragma unroll
  for (int t = 0; t < 16; ++t) p.v[t] = f[16 * L + t];
  return p;
}
__device__ __forceinline__ void store_stride(const PF16& p, float* __restrict__ f, int L) {
#pragma unroll
  for (int m = 0; m < 16; ++m) f[L + 16 * m] = p.v[m];
}
__device__ __forceinline__ void store_contig(const PF16& p, float* __restrict__ f, int L) {
#pragma unroll
  for (int t = 0; t < 16; ++t) f[16 * L + t] = p.v[t];
}

// mode 0: ntt_fwd_f<false>, 1: ntt_fwd_f<true>, 2: ntt_inv_f,
//      3 / 4: forward (plain / MIDRED), reduce_f, inverse.  in / out: [n][256] in natural order
__global__ __launch_bounds__(256) void k_ntt(int mode, size_t n, const float* __restrict__ in, float* __restrict__ out) {
  __shared__ float lds[GROUPS][PBUF];
  const int gi = threadIdx.x >> 4, L = threadIdx.x & 15;
  const size_t raw = (size_t)blockIdx.x * GROUPS + gi;
  const bool active = raw < n;
  const size_t i = active ? raw : n - 1;
  const float* f = in + 256 * i;
  float* buf = lds[gi];
  PF16 p;
  if (mode == 2) {
    p = load_contig(f, L);
    ntt_inv_f(p, buf, L);
    if (active) store_stride(p, out + 256 * i, L);
    return;
  }
  p = load_stride(f, L);
  if (mode == 0 || mode == 3)
    ntt_fwd_f<false>(p, buf, L);
  else
    ntt_fwd_f<true>(p, buf, L);
  if (mode < 2) {
    if (active) store_contig(p, out + 256 * i, L);
    return;
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) p.v[t] = reduce_f(p.v[t]);
  ntt_inv_f(p, buf, L);
  if (active) store_stride(p, out + 256 * i, L);
}

// acc = sum over j < k of a_j o NTT(b_j) as the cores compute it: b_j (time domain) through
// ntt_fwd_f<MIDRED> and make_bop_f, a_j in [0, q) as packed int16 pairs, basemul_acc; then acc_to_f.
// a: [n][k][256] int32, b: [n][k][256] float, acc / res: [n][256]
__global__ __launch_bounds__(256) void k_basemul(int midred, int k, size_t n, const int32_t* __restrict__ a,
                                                 const float* __restrict__ b, int32_t* __restrict__ acc_out,
                                                 float* __restrict__ res) {
  __shared__ float lds[GROUPS][PBUF];
  const int gi = threadIdx.x >> 4, L = threadIdx.x & 15;
  const size_t raw = (size_t)blockIdx.x * GROUPS + gi;
  const bool active = raw < n;
  const size_t i = active ? raw : n - 1;
  int acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0;
  for (int j = 0; j < k; ++j) {
    PF16 p = load_stride(b + 256 * (i * k + j), L);
    if (midred)
      ntt_fwd_f<true>(p, lds[gi], L);
    else
      ntt_fwd_f<false>(p, lds[gi], L);
    const BOp bo = make_bop_f(p, L);
    const int32_t* aj = a + 256 * (i * k + j) + 16 * L;
    PK8 ap;
#pragma unroll
    for (int u = 0; u < 8; ++u) ap.w[u] = pack16(aj[2 * u], aj[2 * u + 1]);
    basemul_acc(acc, ap, bo);
  }
  if (active) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      acc_out[256 * i + 16 * L + t] = acc[t];
      res[256 * i + 16 * L + t] = acc_to_f(acc[t]);
    }
  }
}

int finish() {
  if (hipGetLastError() != hipSuccess) return -2;
  return hipDeviceSynchronize() == hipSuccess ? 0 : -2;
}
unsigned blocks(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

// Raw mode, elementwise: out[i] = op(x[i]) (twiddle zi[i] for the modmul ops; zi may be null
// otherwise).  out holds float32 for the float-valued ops and int32 for the others.
int mlkp_raw(int op, int d, size_t n, const int32_t* x, const int32_t* zi, void* out) {
  if (op < 0 || op >= OP_COUNT || !d_ok(op, d) || n == 0 || n > RAW_MAX || !x || !out) return -1;
  if ((op == OP_MODMUL_F || op == OP_MODMUL_LF) && !zi) return -1;
  hipLaunchKernelGGL(k_raw, dim3(blocks(n, 256)), dim3(256), 0, 0, op, d, n, x, zi, (uint32_t*)out);
  return finish();
}

// Sweep mode: every x in [lo, hi] (against twiddles [z0, z1) for the modmul ops), compared on the
// device.  res (device, 20 x int64): tested, mismatches, smallest and largest mismatching x,
// then 8 (x, twiddle) samples.
int mlkp_sweep(int op, int d, long long lo, long long hi, int z0, int z1, long long* res) {
  const bool mm = op == OP_MODMUL_F || op == OP_MODMUL_LF;
  const bool known = op == OP_REDUCE || mm || op == OP_COMPRESS_F || op == OP_CANON_F || op == OP_I2F ||
                     op == OP_F2I || op == OP_ACC_TO_F;
  if (!known || !d_ok(op, d) || !res || lo > hi || lo < -(1ll << 31) || hi > (1ll << 31) - 1) return -1;
  if (!mm) z0 = 0, z1 = 1;
  if (z0 < 0 || z1 > NTW || z0 >= z1) return -1;
  static_assert(sizeof(SweepOut) == 20 * 8, "res layout");
  SweepOut init{};
  init.min_bad = INT64_MAX, init.max_bad = INT64_MIN;
  if (hipMemcpy(res, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) return -2;
  const unsigned long long total = ((unsigned long long)(hi - lo) + 1) * (unsigned)(z1 - z0);
  const unsigned long long want = (total + 255) / 256;
  hipLaunchKernelGGL(k_sweep, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, 0, op, d, lo, hi, z0, z1,
                     (SweepOut*)res);
  return finish();
}

// z[128], g[128], zq[128], INV128F, Z1INV128F as the device holds them (386 floats)
int mlkp_tables(float* out) {
  if (!out) return -1;
  hipLaunchKernelGGL(k_tables, dim3(1), dim3(128), 0, 0, out);
  return finish();
}

// in [n][3] uint64 (a lane's 24 bytes), out [n][16] int32; mode 0 split12, 1 decode12_w (bad [n]
// int32 required), 2 unpack12
int mlkp_decode12(int mode, size_t n, const uint64_t* in, int32_t* out, int32_t* bad) {
  if (mode < 0 || mode > 2 || n == 0 || n > RAW_MAX || !in || !out || (mode == 1 && !bad)) return -1;
  hipLaunchKernelGGL(k_dec12, dim3(blocks(n, 256)), dim3(256), 0, 0, mode, n, in, out, bad);
  return finish();
}

// in [n][3] uint32 (eta = 2 reads two of them), out [n][16] float
int mlkp_cbd(int eta, size_t n, const uint32_t* in, float* out) {
  if ((eta != 2 && eta != 3) || n == 0 || n > RAW_MAX || !in || !out) return -1;
  if (eta == 2)
    hipLaunchKernelGGL(k_cbd<2>, dim3(blocks(n, 256)), dim3(256), 0, 0, n, in, out);
  else
    hipLaunchKernelGGL(k_cbd<3>, dim3(blocks(n, 256)), dim3(256), 0, 0, n, in, out);
  return finish();
}

// in / out [n][256] float in natural coefficient order; modes: see k_ntt
int mlkp_ntt(int mode, size_t n, const float* in, float* out) {
  if (mode < 0 || mode > 4 || n == 0 || n > (RAW_MAX >> 8) || !in || !out) return -1;
  hipLaunchKernelGGL(k_ntt, dim3(blocks(n, GROUPS)), dim3(256), 0, 0, mode, n, in, out);
  return finish();
}

// a [n][k][256] int32 in [0, q), b [n][k][256] float (time domain), acc [n][256] int32, res [n][256] float
int mlkp_basemul(int midred, int k, size_t n, const int32_t* a, const float* b, int32_t* acc, float* res) {
  if ((midred != 0 && midred != 1) || k < 1 || k > 4 || n == 0 || n > (RAW_MAX >> 10) || !a || !b || !acc || !res)
    return -1;
  hipLaunchKernelGGL(k_basemul, dim3(blocks(n, GROUPS)), dim3(256), 0, 0, midred, k, n, a, b, acc, res);
  return finish();
}

}  // extern "C"
