// Test-only probe of the ML-DSA device primitives (csrc/mldsa_arith.cuh), its own shared object built
// by csrc/Makefile with the library's flags; tests/test_gpu_mldsa_arith.py drives it.  Raw mode copies a
// primitive's outputs back for numpy; sweep mode compares whole ranges on the device against plain
// 64-bit integer C++ and returns counts.  All pointers are device pointers.
#include <hip/hip_runtime.h>

#include "keccak.cuh"
#include "mldsa_arith.cuh"

using namespace qrk;
using namespace qrk::mldsa;

enum { OP_MODMUL = 0, OP_REDUCE = 1, OP_CANON = 2, OP_DECOMPOSE = 3, OP_USEHINT = 4 };

__device__ __forceinline__ long long mod_q(long long x) {
  x %= Q;
  return x < 0 ? x + Q : x;
}
// Decompose and UseHint as FIPS 204 writes them, in 64-bit integers with % and /
__device__ void ref_decompose(long long r, long long g2, long long& r1, long long& r0) {
  r0 = r % (2 * g2);
  if (r0 > g2) r0 -= 2 * g2;
  if (r - r0 == Q - 1) {
    r1 = 0;
    r0 -= 1;
  } else {
    r1 = (r - r0) / (2 * g2);
  }
}
__device__ long long ref_use_hint(int h, long long r, long long g2) {
  const long long m = (Q - 1) / (2 * g2);
  long long r1, r0;
  ref_decompose(r, g2, r1, r0);
  if (!h) return r1;
  return r0 > 0 ? (r1 + 1) % m : (r1 - 1 + m) % m;
}

// out (int32) of op at x; arg: the second factor (OP_MODMUL), gamma2 selector 0 = (q-1)/88, 1 = (q-1)/32,
// plus 2 h for OP_USEHINT.  OP_DECOMPOSE returns r1 in out and r0 in out2.
__device__ __forceinline__ void apply(int op, int arg, int x, int& out, int& out2) {
  out2 = 0;
  switch (op) {
    case OP_MODMUL: out = modmul(x, (double)arg); break;
    case OP_REDUCE: out = reduce(x); break;
    case OP_CANON: out = canon(x); break;
    case OP_DECOMPOSE:
      if (arg & 1) decompose<(Q - 1) / 32>(x, out, out2);
      else decompose<(Q - 1) / 88>(x, out, out2);
      break;
    default: out = (arg & 1) ? use_hint<(Q - 1) / 32>(arg >> 1, x) : use_hint<(Q - 1) / 88>(arg >> 1, x); break;
  }
}
__device__ __forceinline__ bool good(int op, int arg, int x, int out, int out2) {
  const long long g2 = (arg & 1) ? (Q - 1) / 32 : (Q - 1) / 88;
  switch (op) {
    case OP_MODMUL: return (out < 0 ? -out : out) <= HALFQ && mod_q(out) == mod_q((long long)x * arg);
    case OP_REDUCE: return (out < 0 ? -out : out) <= HALFQ && mod_q(out) == mod_q(x);
    case OP_CANON: return out >= 0 && out < Q && out == mod_q(x);
    case OP_DECOMPOSE: {
      long long r1, r0;
      ref_decompose(x, g2, r1, r0);
      return out == r1 && out2 == r0;
    }
    default: return out == ref_use_hint(arg >> 1, x, g2);
  }
}

__global__ void k_raw(int op, int arg, size_t n, const int* x, int* out, int* out2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int a, b;
  apply(op, arg, x[i], a, b);
  out[i] = a;
  if (out2) out2[i] = b;
}
// res: [0] tested, [1] mismatches, [2] smallest and [3] largest mismatching x (res[2] starts at LLONG_MAX,
// res[3] at LLONG_MIN)
__global__ void k_sweep(int op, int arg, long long lo, long long hi, unsigned long long* res) {
  unsigned long long tested = 0, bad = 0;
  for (long long x = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x; x < hi;
       x += (long long)gridDim.x * blockDim.x) {
    int a, b;
    apply(op, arg, (int)x, a, b);
    ++tested;
    if (!good(op, arg, (int)x, a, b)) {
      ++bad;
      atomicMin((long long*)&res[2], x);
      atomicMax((long long*)&res[3], x);
    }
  }
  atomicAdd(&res[0], tested);
  if (bad) atomicAdd(&res[1], bad);
}

__global__ __launch_bounds__(256) void k_ntt(int inverse, const int* in, int* out) {
  __shared__ int a[N];
  const int tid = threadIdx.x;
  a[tid] = in[blockIdx.x * N + tid];
  if (inverse) ntt_inv(a, 1, tid, 256);
  else ntt_fwd(a, 1, tid, 256);
  out[blockIdx.x * N + tid] = a[tid];
}

// kind 18 / 20: z with gamma1 = 2^17 / 2^19; kind 10: t1 2^d
__global__ void k_unpack(int kind, const uint8_t* in, int* out) {
  const int i = threadIdx.x;
  out[i] = kind == 10 ? t1_coeff_2d(in, i) : z_coeff(in, kind, kind == 18 ? 1 << 17 : 1 << 19, i);
}

// one lane per stream of nblocks 168-byte blocks (zeros, all accepted, once a stream runs out)
__global__ __launch_bounds__(64) void k_rej(int nstreams, int nblocks, const uint8_t* bytes, int* coeffs, int* blocks) {
  const int s = threadIdx.x;
  const bool live = s < nstreams;
  int b = 0;
  const int used = rej_ntt_poly(
      [&](uint64_t(&w)[21]) {
        for (int x = 0; x < 21; ++x) {
          uint64_t v = 0;
          if (live && b < nblocks)
            for (int y = 0; y < 8; ++y) v |= (uint64_t)bytes[((size_t)s * nblocks + b) * 168 + 8 * x + y] << (8 * y);
          w[x] = v;
        }
        ++b;
      },
      [&](int i, int v) {
        if (live) coeffs[s * N + i] = v;
      },
      [&](int) {});
  if (live) blocks[s] = used;
}

// SampleInBall, one lane per row.  CW > 0: the stream is SHAKE256 of the CW-word seed at seeds + row * 8 * CW;
// CW = 0: crafted 136-byte blocks, nblocks per row (zeros once they run out).
template <int CW>
__global__ __launch_bounds__(64) void k_sib(int rows, int tau, int nblocks, const uint8_t* seeds, int8_t* c,
                                            int* blocks) {
  __shared__ uint32_t cs[64][64];
  __shared__ uint64_t sb[64][17];
  const int lane = threadIdx.x;
  if (lane >= rows) return;
  KState s;
  kzero(s);
  int b = 0;
  const int used = sample_in_ball(tau, (int8_t*)cs[lane], (uint8_t*)sb[lane], [&](uint8_t* buf) {
    if constexpr (CW > 0) {
      if (b == 0) {
#pragma unroll
        for (int w = 0; w < CW; ++w) {
          uint64_t v = 0;
          for (int y = 0; y < 8; ++y) v |= (uint64_t)seeds[(size_t)lane * 8 * CW + 8 * w + y] << (8 * y);
          kxor(s, w, v);
        }
        s.a[CW].lo ^= DS_SHAKE;
        s.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
      }
      keccak_f(s);
#pragma unroll
      for (int w = 0; w < 17; ++w) sb[lane][w] = kword(s, w);
    } else {
      for (int y = 0; y < 136; ++y) buf[y] = b < nblocks ? seeds[((size_t)lane * nblocks + b) * 136 + y] : 0;
    }
    ++b;
  });
  for (int i = 0; i < N; ++i) c[lane * N + i] = ((int8_t*)cs[lane])[i];
  blocks[lane] = used;
}

__global__ void k_hint(int k, int omega, int rows, const uint8_t* y, uint32_t* bits, int* ok) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  for (int i = 0; i < k * 8; ++i) bits[r * 64 + i] = 0;
  ok[r] = hint_unpack(y + (size_t)r * (omega + k), k, omega, bits + r * 64) ? 1 : 0;
}

__global__ void k_w1(int bits, const uint8_t* w, uint8_t* out) {
  const int b = threadIdx.x;
  if (b < 32 * bits) out[b] = w1_byte(w, bits, b);
}

__global__ void k_tables(double* out) {
  const int i = threadIdx.x;
  out[i] = TAB.z[i];
  if (i == 0) out[N] = INV256;
}

static int done() { return (int)hipDeviceSynchronize() | (int)hipGetLastError(); }

extern "C" {
int mldp_raw(int op, int arg, size_t n, const int* x, int* out, int* out2) {
  if (n) hipLaunchKernelGGL(k_raw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, arg, n, x, out, out2);
  return done();
}
int mldp_sweep(int op, int arg, long long lo, long long hi, unsigned long long* res) {
  const unsigned long long init[4] = {0, 0, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull};
  if (hipMemcpy(res, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_sweep, dim3(4096), dim3(256), 0, 0, op, arg, lo, hi, res);
  return done();
}
int mldp_ntt(int inverse, int polys, const int* in, int* out) {
  hipLaunchKernelGGL(k_ntt, dim3(polys), dim3(256), 0, 0, inverse, in, out);
  return done();
}
int mldp_unpack(int kind, const uint8_t* in, int* out) {
  hipLaunchKernelGGL(k_unpack, dim3(1), dim3(256), 0, 0, kind, in, out);
  return done();
}
int mldp_rej(int nstreams, int nblocks, const uint8_t* bytes, int* coeffs, int* blocks) {
  if (nstreams < 1 || nstreams > 64) return -1;
  hipLaunchKernelGGL(k_rej, dim3(1), dim3(64), 0, 0, nstreams, nblocks, bytes, coeffs, blocks);
  return done();
}
int mldp_sib(int rows, int tau, int seed_bytes, int nblocks, const uint8_t* seeds, int8_t* c, int* blocks) {
  if (rows < 1 || rows > 64) return -1;
  switch (seed_bytes) {
    case 0: hipLaunchKernelGGL(k_sib<0>, dim3(1), dim3(64), 0, 0, rows, tau, nblocks, seeds, c, blocks); break;
    case 32: hipLaunchKernelGGL(k_sib<4>, dim3(1), dim3(64), 0, 0, rows, tau, nblocks, seeds, c, blocks); break;
    case 48: hipLaunchKernelGGL(k_sib<6>, dim3(1), dim3(64), 0, 0, rows, tau, nblocks, seeds, c, blocks); break;
    case 64: hipLaunchKernelGGL(k_sib<8>, dim3(1), dim3(64), 0, 0, rows, tau, nblocks, seeds, c, blocks); break;
    default: return -1;
  }
  return done();
}
int mldp_hint(int k, int omega, int rows, const uint8_t* y, uint32_t* bits, int* ok) {
  hipLaunchKernelGGL(k_hint, dim3((rows + 63) / 64), dim3(64), 0, 0, k, omega, rows, y, bits, ok);
  return done();
}
int mldp_w1(int bits, const uint8_t* w, uint8_t* out) {
  hipLaunchKernelGGL(k_w1, dim3(1), dim3(256), 0, 0, bits, w, out);
  return done();
}
int mldp_tables(double* out) {
  hipLaunchKernelGGL(k_tables, dim3(1), dim3(256), 0, 0, out);
  return done();
}
}
