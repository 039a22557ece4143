// What ML-DSA verification (mldsa.hip) and key generation / signing (mldsa_sign.hip) share: the parameter
// set as a template argument, the byte-wise SHAKE absorb and the body of ExpandA.  All three work on public
// data only (pk, rho, the message): secret bytes never pass through absorb_bytes' data-dependent loop
// bound, and rho is public.  The kernels themselves stay in their own files, so that each launch keeps
// its own name in a context's profile.
#pragma once

#include "keccak.cuh"
#include "mldsa_arith.cuh"

namespace qrk {
namespace mldsa {

template <int PS>
struct Set;
template <>
struct Set<0> {
  static constexpr Params P = P44;
};
template <>
struct Set<1> {
  static constexpr Params P = P65;
};
template <>
struct Set<2> {
  static constexpr Params P = P87;
};

// Absorbs the `len` bytes at(0) .. at(len - 1) into a sponge of RW rate words whose current block
// already holds SW words, pads (SHAKE) and permutes: on return s holds the first output block.
template <int RW, int SW, class At>
__device__ __forceinline__ void absorb_bytes(KState& s, uint32_t len, At at) {
  auto word = [&](uint32_t p) -> uint64_t {
    uint64_t r = 0;
    if (p + 8 <= len) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r |= (uint64_t)at(p + j) << (8 * j);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t i = p + j;
        const uint32_t b = i < len ? at(i) : (i == len ? DS_SHAKE : 0u);
        r |= (uint64_t)b << (8 * j);
      }
    }
    return r;
  };
  uint32_t pos = 0;
#pragma unroll
  for (int w = SW; w < RW; ++w) {
    kxor(s, w, word(pos));
    pos += 8;
  }
  while (pos <= len) {  // the padding byte (stream index len) is not in yet
    keccak_f(s);
#pragma unroll
    for (int w = 0; w < RW; ++w) {
      kxor(s, w, word(pos));
      pos += 8;
    }
  }
  s.a[RW - 1].hi ^= 0x80000000u;
  keccak_f(s);
}

// A_hat = ExpandA(rho) of n rows, the body of a kernel of 64 lanes per workgroup: one lane per polynomial
// (grid: ceil(n k l / 64) workgroups), five SHAKE128 blocks (a general loop), coefficients staged per
// block in `tile` (64 * EXPAND_STRIDE ints of LDS) so that the global stores are contiguous runs.  Row r's
// rho is the 32 bytes at rho + r * stride (a public key or a secret key starts with it); A: k l KiB per row.
constexpr int EXPAND_STRIDE = 57;  // the coefficients a lane accepts from one block (<= 56), padded
template <int PS>
__device__ __forceinline__ void expand_a_block(size_t n, const uint8_t* __restrict__ rho0, size_t stride,
                                               int32_t* __restrict__ A, int* tile) {
  constexpr Params P = Set<PS>::P;
  constexpr int KL = P.k * P.l, STRIDE = EXPAND_STRIDE;
  const int lane = threadIdx.x;
  const size_t npoly = n * KL, first = (size_t)blockIdx.x * 64, gid = first + lane;
  const size_t row = gid < npoly ? gid / KL : 0;
  const int e = (int)(gid % KL), i = e / P.l, j = e % P.l;
  const uint8_t* rho = rho0 + row * stride;
  KState s;
  kzero(s);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint64_t v = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= (uint64_t)rho[8 * w + b] << (8 * b);
    kxor(s, w, v);
  }
  // rho || column || row, then the SHAKE padding
  s.a[4].lo ^= (uint32_t)j | ((uint32_t)i << 8) | (DS_SHAKE << 16);
  s.a[RW_SHAKE128 - 1].hi ^= 0x80000000u;
  int cnt = 0, written = 0;
  rej_ntt_poly(
      [&](uint64_t(&w)[21]) {
        keccak_f(s);
#pragma unroll
        for (int x = 0; x < 21; ++x) w[x] = kword(s, x);
      },
      [&](int, int v) { tile[lane * STRIDE + cnt++] = v; },
      [&](int) {
        // Lane r's run goes out as one contiguous store of up to 56 lanes.  written + cnt <= 256, so
        // every store stays inside polynomial first + r, and polynomials past npoly store nothing.
        __syncthreads();
        for (int r = 0; r < 64 && first + r < npoly; ++r) {
          const int nr = __builtin_amdgcn_readlane(cnt, r), wr = __builtin_amdgcn_readlane(written, r);
          if (lane < nr) A[(first + r) * N + wr + lane] = tile[r * STRIDE + lane];
        }
        written += cnt;
        cnt = 0;
        __syncthreads();
      });
}

}  // namespace mldsa
}  // namespace qrk
