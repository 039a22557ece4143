// Test-only probe of the SLH-DSA device primitives (csrc/slhdsa_common.cuh, csrc/sha2.cuh), its own shared
// object built by csrc/Makefile with the library's flags; tests/test_gpu_slhdsa_prims.py drives it.  Raw mode
// only: every entry point takes device pointers, runs the header's own templates as compiled for the GPU and
// copies nothing back; the test compares on the host.  Nothing of the header is written again here.
#include <hip/hip_runtime.h>

#include "slhdsa_common.cuh"

using namespace qrk;
using namespace qrk::slhdsa;

// An address travels as six 64-bit values: layer, tree, type, w1, w2, w3.
__device__ __forceinline__ Adrs adrs_of(const uint64_t* a) {
  return Adrs{(uint32_t)a[0], a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5]};
}

// ------------------------------------------------------------------ sha::tail / sha::tail512
// One lane per case: state (8 values; SHA-256 uses their low halves), prefix, len, the bytes at bytes + boff.
// Word t of tail block 0 is replaced from a register copy of ow[16 i + t] where bit t of omask is set.
template <bool BIG>
__global__ __launch_bounds__(64) void k_tail(size_t n, const uint64_t* state, const uint32_t* prefix,
                                             const uint32_t* len, const uint32_t* boff, const uint8_t* bytes,
                                             const uint32_t* omask, const uint64_t* ow, uint64_t* out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* m = bytes + boff[i];
  const uint32_t mask = omask[i];
  uint64_t r[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) r[t] = ow[i * 16 + t];
  auto byte_at = [&](uint32_t p) -> uint32_t { return m[p]; };
  if constexpr (BIG) {
    sha::H8x64 s;
#pragma unroll
    for (int j = 0; j < 8; ++j) s.h[j] = state[i * 8 + j];
    sha::tail512(s, prefix[i], len[i], byte_at,
                 [&](uint32_t b, int t, uint64_t x) { return (b == 0 && ((mask >> t) & 1)) ? r[t] : x; });
#pragma unroll
    for (int j = 0; j < 8; ++j) out[i * 8 + j] = s.h[j];
  } else {
    sha::H8 s;
#pragma unroll
    for (int j = 0; j < 8; ++j) s.h[j] = (uint32_t)state[i * 8 + j];
    sha::tail(s, prefix[i], len[i], byte_at,
              [&](uint32_t b, int t, uint32_t x) { return (b == 0 && ((mask >> t) & 1)) ? (uint32_t)r[t] : x; });
#pragma unroll
    for (int j = 0; j < 8; ++j) out[i * 8 + j] = s.h[j];
  }
}

// ------------------------------------------------------------------ H_msg
// One lane per case: R (n bytes), PK.seed || PK.root (2 n), the message at msg + moff[i] .. moff[i + 1]; one
// context for the launch, as in k_slhdsa_front.
template <int PS>
__global__ __launch_bounds__(64) void k_hmsg(size_t n, const uint8_t* r, const uint8_t* pkr, const uint8_t* msg,
                                             const uint32_t* moff, const uint8_t* ctx, uint32_t ctx_len,
                                             uint8_t* out) {
  constexpr Params P = make(PS);
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  h_msg<PS>(r + i * P.n, pkr + i * P.pk(), msg + moff[i], moff[i + 1] - moff[i], ctx, ctx_len, out + i * P.m);
}

// ------------------------------------------------------------------ F and H
template <int N>
__global__ __launch_bounds__(64) void k_hash_f(size_t n, const uint8_t* seed, const uint64_t* adrs, const uint8_t* x,
                                               uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const Seeds<N> sd = seed_states<N>(seed + i * N);
  uint32_t v[N / 4];
  load_node<N>(x + i * N, v);
  hash_f<N>(sd, adrs_of(adrs + 6 * i), v);
  store_node<N>(out + i * N, v);
}
template <int N>
__global__ __launch_bounds__(64) void k_hash_h(size_t n, const uint8_t* seed, const uint64_t* adrs, const uint8_t* x,
                                               const uint8_t* au, const uint8_t* right, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const Seeds<N> sd = seed_states<N>(seed + i * N);
  uint32_t v[N / 4], w[N / 4];
  load_node<N>(x + i * N, v);
  load_node<N>(au + i * N, w);
  hash_h<N>(sd, adrs_of(adrs + 6 * i), v, w, right[i] != 0);
  store_node<N>(out + i * N, v);
}

// ------------------------------------------------------------------ T_l through LDS
// One wave per case, four to a workgroup with a slice of LDS each, as in k_slhdsa_core: the lanes write the
// l nodes (two passes when l > 64), lane 0 the address, then every lane reads the stream back.
template <int N>
__global__ __launch_bounds__(256) void k_tlds(size_t n, int l, const uint8_t* seed, const uint64_t* adrs,
                                              const uint8_t* nodes, uint8_t* out) {
  constexpr int NW = N / 4, MAXL = 2 * N + 3;
  constexpr int SLICE = (22 + MAXL * N + 2 + 15) / 16 * 8;  // uint16 units
  __shared__ __attribute__((aligned(16))) uint16_t lds[4][SLICE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t i = (size_t)blockIdx.x * 4 + wv;
  if (i >= n) return;
  uint16_t* slice = lds[wv];
  const Seeds<N> sd = seed_states<N>(seed + i * N);
  for (int c = lane; c < l; c += 64) {
    uint32_t x[NW];
    load_node<N>(nodes + (i * l + c) * N, x);
    lds_put_node<N>(slice, c, x);
  }
  if (lane == 0) lds_put_adrs(slice, adrs_of(adrs + 6 * i));
  wave_sync();
  uint32_t node[NW];
  t_lds<N>(sd, slice, 22 + l * N, node);
  wave_sync();
  if (lane == 0) store_node<N>(out + i * N, node);
}

// ------------------------------------------------------------------ indices
template <int PS>
__global__ __launch_bounds__(64) void k_fors(size_t n, const uint8_t* md, uint32_t* out) {
  constexpr Params P = make(PS);
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < P.k; ++j) out[i * P.k + j] = fors_index<PS>(md + i * P.md(), j);
}
template <int PS>
__global__ __launch_bounds__(64) void k_indices(size_t n, const uint8_t* dg, uint64_t* trees, uint32_t* leaves) {
  constexpr Params P = make(PS);
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t tree;
  uint32_t leaf;
  digest_indices<PS>(dg + i * P.m, tree, leaf);
  for (int j = 0; j < P.d; ++j) {
    trees[i * P.d + j] = tree;
    leaves[i * P.d + j] = leaf;
    next_layer<PS>(tree, leaf);
  }
}

// ------------------------------------------------------------------ WOTS+ digits
// The checksum and the len digits as k_slhdsa_core takes them; the word of chain c is picked by index here
// (the core kernel's select over registers is part of that kernel, not of the header).
template <int N>
__global__ __launch_bounds__(64) void k_wots(size_t n, const uint8_t* nodes, uint32_t* csums, uint32_t* digits) {
  constexpr int LEN = 2 * N + 3;
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t node[N / 4];
  load_node<N>(nodes + i * N, node);
  const uint32_t csum = wots_csum<N>(node);
  csums[i] = csum;
  for (int c = 0; c < LEN; ++c)
    digits[i * LEN + c] = c < 2 * N ? wots_msg_digit(c, node[c >> 3]) : wots_csum_digit<N>(c, csum);
}

// ------------------------------------------------------------------ row_span
// off: a two-entry offset table per case.  Only the offsets are read; mlen keeps 0xffffffff when refused.
__global__ __launch_bounds__(64) void k_row_span(size_t n, const uint64_t* off, int32_t* ok, uint64_t* o0,
                                                 uint32_t* mlen) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t a = 0;
  uint32_t l = 0xffffffffu;
  ok[i] = row_span(off + 2 * i, 0, a, l) ? 1 : 0;
  o0[i] = a;
  mlen[i] = l;
}

static int done() { return (int)hipDeviceSynchronize() | (int)hipGetLastError(); }
static dim3 lanes(size_t n) { return dim3((unsigned)((n + 63) / 64)); }

#define FOR_PS(ps, X) \
  switch (ps) {       \
    case 0: X(0);     \
    case 1: X(1);     \
    case 2: X(2);     \
    case 3: X(3);     \
    case 4: X(4);     \
    case 5: X(5);     \
    default: return -1; \
  }
#define FOR_N(nb, X) \
  switch (nb) {      \
    case 16: X(16);  \
    case 24: X(24);  \
    case 32: X(32);  \
    default: return -1; \
  }

extern "C" {
int slhp_sha_tail(int big, size_t n, const uint64_t* state, const uint32_t* prefix, const uint32_t* len,
                  const uint32_t* boff, const uint8_t* bytes, const uint32_t* omask, const uint64_t* ow,
                  uint64_t* out) {
  if (!n) return 0;
  if (big) hipLaunchKernelGGL(k_tail<true>, lanes(n), dim3(64), 0, 0, n, state, prefix, len, boff, bytes, omask, ow, out);
  else hipLaunchKernelGGL(k_tail<false>, lanes(n), dim3(64), 0, 0, n, state, prefix, len, boff, bytes, omask, ow, out);
  return done();
}
int slhp_h_msg(int ps, size_t n, const uint8_t* r, const uint8_t* pkr, const uint8_t* msg, const uint32_t* moff,
               const uint8_t* ctx, uint32_t ctx_len, uint8_t* out) {
  if (!n) return 0;
#define X(PS) \
  hipLaunchKernelGGL(k_hmsg<PS>, lanes(n), dim3(64), 0, 0, n, r, pkr, msg, moff, ctx, ctx_len, out); \
  return done()
  FOR_PS(ps, X)
#undef X
}
int slhp_hash_f(int nb, size_t n, const uint8_t* seed, const uint64_t* adrs, const uint8_t* x, uint8_t* out) {
  if (!n) return 0;
#define X(N) \
  hipLaunchKernelGGL(k_hash_f<N>, lanes(n), dim3(64), 0, 0, n, seed, adrs, x, out); \
  return done()
  FOR_N(nb, X)
#undef X
}
int slhp_hash_h(int nb, size_t n, const uint8_t* seed, const uint64_t* adrs, const uint8_t* x, const uint8_t* au,
                const uint8_t* right, uint8_t* out) {
  if (!n) return 0;
#define X(N) \
  hipLaunchKernelGGL(k_hash_h<N>, lanes(n), dim3(64), 0, 0, n, seed, adrs, x, au, right, out); \
  return done()
  FOR_N(nb, X)
#undef X
}
int slhp_t_lds(int nb, size_t n, int l, const uint8_t* seed, const uint64_t* adrs, const uint8_t* nodes,
               uint8_t* out) {
  if (!n) return 0;
  if (l < 1 || l > 2 * nb + 3) return -1;  // the slice holds at most len nodes
#define X(N) \
  hipLaunchKernelGGL(k_tlds<N>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, n, l, seed, adrs, nodes, out); \
  return done()
  FOR_N(nb, X)
#undef X
}
int slhp_fors_index(int ps, size_t n, const uint8_t* md, uint32_t* out) {
  if (!n) return 0;
#define X(PS) \
  hipLaunchKernelGGL(k_fors<PS>, lanes(n), dim3(64), 0, 0, n, md, out); \
  return done()
  FOR_PS(ps, X)
#undef X
}
int slhp_indices(int ps, size_t n, const uint8_t* dg, uint64_t* trees, uint32_t* leaves) {
  if (!n) return 0;
#define X(PS) \
  hipLaunchKernelGGL(k_indices<PS>, lanes(n), dim3(64), 0, 0, n, dg, trees, leaves); \
  return done()
  FOR_PS(ps, X)
#undef X
}
int slhp_wots_digits(int nb, size_t n, const uint8_t* nodes, uint32_t* csums, uint32_t* digits) {
  if (!n) return 0;
#define X(N) \
  hipLaunchKernelGGL(k_wots<N>, lanes(n), dim3(64), 0, 0, n, nodes, csums, digits); \
  return done()
  FOR_N(nb, X)
#undef X
}
int slhp_row_span(size_t n, const uint64_t* off, int32_t* ok, uint64_t* o0, uint32_t* mlen) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_row_span, lanes(n), dim3(64), 0, 0, n, off, ok, o0, mlen);
  return done();
}
}
