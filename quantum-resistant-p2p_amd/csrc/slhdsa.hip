// Batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple verification, the "f" parameter sets, for gfx950.
//
// The reference's SPHINCSSignature.verify (quantum_resistant_p2p/crypto/signatures.py:294-315, called like
// ML-DSA's from app/messaging.py:721, 933, 1174, 1480) over n rows at once.  Two names per parameter set:
// "SPHINCS+-SHA2-{128,192,256}f-simple" is the round-3.1 submission as liboqs ships it,
// "SLH-DSA-SHA2-{128,192,256}f" is FIPS 205 pure SLH-DSA (Algorithm 24 over Algorithm 20).  For SHA2
// "simple" verification they differ in two places only (Params::fips): the message framing in
// k_slhdsa_front (FIPS 205: M' = 0 || len(ctx) || ctx || M; round 3.1: M) and the FORS index extraction in
// fors_index (FIPS 205: base_2b, most significant bit first; round 3.1 message_to_indices: least
// significant bit first within each byte).  Everything else is shared.
//
// Two stream-ordered launches per chunk:
//
//   k_slhdsa_front  one lane per row: digest = H_msg(R, PK.seed, PK.root, M') = MGF1-SHA-X(R || PK.seed ||
//                   SHA-X(R || PK.seed || PK.root || M'), m), X = 256 for n = 16 and 512 otherwise; a row
//                   of 2^31 bytes or more (or with decreasing offsets) gets FLAG_LONG and nothing else
//   k_slhdsa_core   one 64-lane wave per row, four rows per workgroup: the SHA-256 (and for n > 16 the
//                   SHA-512) state after the PK.seed block once, so that every F, H and short T_l is one
//                   compression; FORS with lane i < k on tree i (F, then a H-steps), the k roots through
//                   LDS to T_k; then per hypertree layer the len WOTS+ chains over the lanes (67 > 64
//                   for n = 32: the lanes loop), each a uniform 15-step loop `if (s >= digit) x = F(x)`,
//                   the chain ends through LDS to T_len, h' H-steps to the layer's root; finally the
//                   comparison with PK.root
//
// The waves of a workgroup serve different rows and some lie past n, so the core kernel has no
// workgroup-wide barrier at all: each wave owns one slice of LDS and orders its own writes and reads
// (wave_sync).  T_k, T_len and the H-steps run redundantly in every lane of the wave (uniform values, so
// nothing is broadcast).  k_slhdsa_core is the only writer of status and writes every row exactly once:
// 0 when the flag word is 0, else -1.  Every input of verification is public, so the kernels branch on
// data.  Nothing here may be copied into a signing path.
#include <cstring>

#include "qrkem_internal.h"
#include "sha2.cuh"

namespace qrk {
namespace slhdsa {

enum : uint32_t { FLAG_ROOT = 1, FLAG_LONG = 2 };
enum : uint32_t { WOTS_HASH = 0, WOTS_PK = 1, TREE = 2, FORS_TREE = 3, FORS_ROOTS = 4 };

struct Params {
  int n, h, d, hp, a, k, m;
  bool fips;
  constexpr int len1() const { return 2 * n; }
  constexpr int len() const { return 2 * n + 3; }  // lg_w = 4: len2 = 3
  constexpr int md() const { return (k * a + 7) / 8; }
  constexpr int pk() const { return 2 * n; }
  constexpr int sk() const { return 4 * n; }
  constexpr int fors_bytes() const { return k * (a + 1) * n; }
  constexpr int xmss_bytes() const { return (hp + len()) * n; }
  constexpr int sig() const { return n + fors_bytes() + d * xmss_bytes(); }
};
// which = 2 set + flavour: set 0, 1, 2 = 128f, 192f, 256f; flavour 0 = SPHINCS+ round 3.1, 1 = FIPS 205
constexpr Params make(int which) {
  const bool f = which & 1;
  return (which >> 1) == 0   ? Params{16, 66, 22, 3, 6, 33, 34, f}
         : (which >> 1) == 1 ? Params{24, 66, 22, 3, 8, 33, 42, f}
                             : Params{32, 68, 17, 4, 9, 35, 49, f};
}

__device__ __forceinline__ uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// ------------------------------------------------------------------ H_msg
template <int PS>
__global__ __launch_bounds__(64) void k_slhdsa_front(size_t n, const uint8_t* __restrict__ pk,
                                                     const uint8_t* __restrict__ msg,
                                                     const uint64_t* __restrict__ off,
                                                     const uint8_t* __restrict__ sig,
                                                     const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                                     uint8_t* __restrict__ digest, uint32_t* __restrict__ flags) {
  using namespace sha;
  constexpr Params P = make(PS);
  constexpr uint32_t N = P.n;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  const uint64_t o0 = off[row], o1 = off[row + 1];
  if (o1 < o0 || o1 - o0 >= (1ull << 31)) {
    flags[row] = FLAG_LONG;
    return;
  }
  const uint32_t mlen = (uint32_t)(o1 - o0);
  const uint32_t pre = P.fips ? 2 + ctx_len : 0;  // FIPS 205 Algorithm 24: M' = 0 || len(ctx) || ctx || M
  const uint8_t* r = sig + row * P.sig();
  const uint8_t* pkr = pk + row * P.pk();
  const uint8_t* m = msg + o0;
  uint8_t* out = digest + row * P.m;
  auto none32 = [](uint32_t, int, uint32_t x) { return x; };
  auto none64 = [](uint32_t, int, uint64_t x) { return x; };
  // R || PK.seed || PK.root || M'
  auto inner_at = [&](uint32_t p) -> uint32_t {
    if (p < N) return r[p];
    if (p < 3 * N) return pkr[p - N];
    uint32_t q = p - 3 * N;
    if (P.fips) {
      if (q < 2) return q ? ctx_len : 0u;
      q -= 2;
      if (q < ctx_len) return ctx[q];
      q -= ctx_len;
    }
    return m[q];
  };
  const uint32_t total = 3 * N + pre + mlen;  // below 2^31 + 353
  if constexpr (N == 16) {
    H8 in = init();
    tail(in, 0, total, inner_at, none32);
    // MGF1: SHA-256(R || PK.seed || inner || counter), counter 0 and 1 (m = 34); inner is words 8..15
#pragma unroll 1
    for (uint32_t c = 0; c < (P.m + 31) / 32; ++c) {
      H8 g = init();
      tail(
          g, 0, 2 * N + 32 + 4,
          [&](uint32_t p) -> uint32_t {
            if (p < N) return r[p];
            if (p < 2 * N) return pkr[p - N];
            return p == 2 * N + 32 + 3 ? c : 0u;
          },
          [&](uint32_t b, int t, uint32_t x) { return (b == 0 && t >= 8) ? in.h[t & 7] : x; });
#pragma unroll
      for (int t = 0; t < 8; ++t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t p = 32 * c + 4 * t + k;
          if (p < (uint32_t)P.m) out[p] = (uint8_t)(g.h[t] >> (24 - 8 * k));
        }
      }
    }
  } else {
    H8x64 in = init512();
    tail512(in, 0, total, inner_at, none64);
    // MGF1: one SHA-512 output (m <= 64) with counter 0; inner is 64-bit words W0 .. W0 + 7
    constexpr int W0 = 2 * N / 8;
    H8x64 g = init512();
    tail512(
        g, 0, 2 * N + 64 + 4,
        [&](uint32_t p) -> uint32_t {
          if (p < N) return r[p];
          if (p < 2 * N) return pkr[p - N];
          return 0u;
        },
        [&](uint32_t b, int t, uint64_t x) { return (b == 0 && t >= W0 && t < W0 + 8) ? in.h[(t - W0) & 7] : x; });
#pragma unroll
    for (int t = 0; t < 8; ++t) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t p = 8 * t + k;
        if (p < (uint32_t)P.m) out[p] = (uint8_t)(g.h[t] >> (56 - 8 * k));
      }
    }
  }
  flags[row] = 0;
}

// ------------------------------------------------------------------ tweakable hashes
struct Adrs {  // the 22-byte compressed address: layer (1) || tree (8) || type (1) || w1 w2 w3 (4 each)
  uint32_t layer;
  uint64_t tree;
  uint32_t type, w1, w2, w3;
};
// Its big-endian words 0 .. 4, and in the upper half of w[5] its last two bytes.
__device__ __forceinline__ void adrs_words(const Adrs& A, uint32_t w[6]) {
  w[0] = (A.layer << 24) | (uint32_t)(A.tree >> 40);
  w[1] = (uint32_t)(A.tree >> 8);
  w[2] = ((uint32_t)A.tree << 24) | (A.type << 16) | (A.w1 >> 16);
  w[3] = (A.w1 << 16) | (A.w2 >> 16);
  w[4] = (A.w2 << 16) | (A.w3 >> 16);
  w[5] = A.w3 << 16;
}

// W[0 .. 6 + NW): ADRSc || the NW words x || 0x80, the message words straddling W's (22 = 5.5 words).
template <int NW, int TOTAL>
__device__ __forceinline__ void short_block(const Adrs& A, const uint32_t* x, uint32_t w[TOTAL]) {
  adrs_words(A, w);
#pragma unroll
  for (int t = 6; t < TOTAL; ++t) w[t] = 0;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    w[5 + j] |= x[j] >> 16;
    w[6 + j] = x[j] << 16;
  }
  w[5 + NW] |= 0x8000u;
}

template <int N>
struct Seeds {  // the states after the PK.seed block
  sha::H8 s256;
  sha::H8x64 s512;  // n > 16 only
};

// x = F(PK.seed, ADRS, x) = Trunc_n(SHA-256(PK.seed || 0^(64 - n) || ADRSc || x)): one compression.
template <int N>
__device__ __forceinline__ void hash_f(const Seeds<N>& sd, const Adrs& A, uint32_t x[N / 4]) {
  constexpr int NW = N / 4;
  uint32_t w[16];
  short_block<NW, 16>(A, x, w);
  w[15] = (64 + 22 + N) * 8;
  sha::H8 s = sd.s256;
  sha::compress(s, w);
#pragma unroll
  for (int j = 0; j < NW; ++j) x[j] = s.h[j];
}

// x = H(PK.seed, ADRS, left || right) with x on the side `x_is_right` says and au on the other: SHA-256 for
// n = 16, SHA-512 otherwise; one compression either way (22 + 2 n + padding fits the block).
template <int N>
__device__ __forceinline__ void hash_h(const Seeds<N>& sd, const Adrs& A, uint32_t x[N / 4], const uint32_t au[N / 4],
                                       bool x_is_right) {
  constexpr int NW = N / 4;
  uint32_t m[2 * NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    m[j] = x_is_right ? au[j] : x[j];
    m[NW + j] = x_is_right ? x[j] : au[j];
  }
  if constexpr (N == 16) {
    uint32_t w[16];
    short_block<2 * NW, 16>(A, m, w);
    w[15] = (64 + 22 + 2 * N) * 8;
    sha::H8 s = sd.s256;
    sha::compress(s, w);
#pragma unroll
    for (int j = 0; j < NW; ++j) x[j] = s.h[j];
  } else {
    uint32_t v[32];
    short_block<2 * NW, 32>(A, m, v);
    v[31] = (128 + 22 + 2 * N) * 8;
    uint64_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = ((uint64_t)v[2 * t] << 32) | v[2 * t + 1];
    sha::H8x64 s = sd.s512;
    sha::compress512(s, w);
#pragma unroll
    for (int j = 0; j < NW; ++j) x[j] = (uint32_t)(s.h[j >> 1] >> ((j & 1) ? 0 : 32));
  }
}

// A wave's slice of LDS holds the stream ADRSc || node_0 || node_1 ... as big-endian 32-bit words W[t]
// (read whole by t_lds); a node starts 22 bytes in, so it is written in 16-bit halves.
typedef uint32_t __attribute__((may_alias)) lds_word;

template <int N>
__device__ __forceinline__ void lds_put_node(uint16_t* slice, int i, const uint32_t x[N / 4]) {
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
    const int g = i * (N / 4) + j;
    slice[2 * (5 + g)] = (uint16_t)(x[j] >> 16);      // low half of W[5 + g]
    slice[2 * (6 + g) + 1] = (uint16_t)(x[j] & 0xffff);  // high half of W[6 + g]
  }
}
__device__ __forceinline__ void lds_put_adrs(uint16_t* slice, const Adrs& A) {
  uint32_t w[6];
  adrs_words(A, w);
  lds_word* W = (lds_word*)slice;
#pragma unroll
  for (int t = 0; t < 5; ++t) W[t] = w[t];
  slice[11] = (uint16_t)(w[5] >> 16);
}

// A wave's LDS writes become visible to its own later reads in program order (one wave issues its DS
// instructions in order); the fences keep the compiler from moving either across.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// out = T_l(PK.seed, ADRS, nodes) over the slice's stream of `len` bytes (len = 22 + l n, so len % 4 = 2).
template <int N>
__device__ __forceinline__ void t_lds(const Seeds<N>& sd, const uint16_t* slice, uint32_t len, uint32_t out[N / 4]) {
  const lds_word* W = (const lds_word*)slice;
  auto word = [&](uint32_t i) -> uint32_t {
    const uint32_t pos = 4 * i;
    if (pos + 4 <= len) return W[i];
    if (pos < len) return (W[i] & 0xffff0000u) | 0x8000u;
    return 0u;
  };
  if constexpr (N == 16) {
    const uint32_t nblk = (len + 9 + 63) / 64;
    sha::H8 s = sd.s256;
#pragma unroll 1
    for (uint32_t b = 0; b < nblk; ++b) {
      uint32_t w[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) w[t] = word(16 * b + t);
      if (b == nblk - 1) {
        w[14] = 0;
        w[15] = (64 + len) * 8;
      }
      sha::compress(s, w);
    }
#pragma unroll
    for (int j = 0; j < N / 4; ++j) out[j] = s.h[j];
  } else {
    const uint32_t nblk = (len + 17 + 127) / 128;
    sha::H8x64 s = sd.s512;
#pragma unroll 1
    for (uint32_t b = 0; b < nblk; ++b) {
      uint64_t w[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) w[t] = ((uint64_t)word(32 * b + 2 * t) << 32) | word(32 * b + 2 * t + 1);
      if (b == nblk - 1) {
        w[14] = 0;
        w[15] = (uint64_t)(128 + len) * 8;
      }
      sha::compress512(s, w);
    }
#pragma unroll
    for (int j = 0; j < N / 4; ++j) out[j] = (uint32_t)(s.h[j >> 1] >> ((j & 1) ? 0 : 32));
  }
}

template <int N>
__device__ __forceinline__ void load_node(const uint8_t* p, uint32_t x[N / 4]) {
#pragma unroll
  for (int j = 0; j < N / 4; ++j) x[j] = be32(p + 4 * j);
}
template <int N>
__device__ __forceinline__ void store_node(uint8_t* p, const uint32_t x[N / 4]) {
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) p[4 * j + k] = (uint8_t)(x[j] >> (24 - 8 * k));
  }
}

// Index i of the k FORS indices in md.  FIPS 205 Algorithm 17 line 1, base_2b(md, a, k): bit strings of a
// bits, most significant first.  Round 3.1 fors.c message_to_indices: bit j of index i is bit
// (i a + j) & 7 of byte (i a + j) >> 3.
template <int PS>
__device__ __forceinline__ uint32_t fors_index(const uint8_t* md, int i) {
  constexpr Params P = make(PS);
  uint32_t idx = 0;
#pragma unroll
  for (int j = 0; j < P.a; ++j) {
    const uint32_t pos = (uint32_t)(i * P.a + j);
    if (P.fips)
      idx = (idx << 1) | ((md[pos >> 3] >> (7 - (pos & 7))) & 1u);
    else
      idx |= ((md[pos >> 3] >> (pos & 7)) & 1u) << j;
  }
  return idx;
}

// The trace outputs (tests: qrk_dbg_slhdsa_verify_trace) are stored only by the TRACE instantiation.
template <int PS, bool TRACE>
__global__ __launch_bounds__(256) void k_slhdsa_core(size_t n, const uint8_t* __restrict__ pk,
                                                     const uint8_t* __restrict__ sig,
                                                     const uint8_t* __restrict__ digest,
                                                     const uint32_t* __restrict__ flags, int32_t* __restrict__ status,
                                                     SlhdsaTrace tr) {
  constexpr Params P = make(PS);
  constexpr int N = P.n, NW = N / 4, LEN = P.len();
  constexpr int MAXL = LEN > P.k ? LEN : P.k;
  constexpr int SLICE = (22 + MAXL * N + 2 + 15) / 16 * 8;  // uint16 units, slices 16-byte aligned
  __shared__ __attribute__((aligned(16))) uint16_t lds[4][SLICE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wv;
  if (row >= n) return;  // no barrier follows: the other waves of the workgroup go on alone
  uint16_t* slice = lds[wv];
  if (flags[row] & FLAG_LONG) {
    if (lane == 0) status[row] = -1;
    if (TRACE) {
      for (int b = lane; b < P.m; b += 64) tr.digest[row * P.m + b] = 0;
      for (int b = lane; b < N; b += 64) tr.fors_pk[row * N + b] = 0;
      for (int b = lane; b < P.d * N; b += 64) tr.roots[row * P.d * N + b] = 0;
      if (lane == 0) tr.flags[row] = FLAG_LONG;
    }
    return;
  }
  const uint8_t* pkr = pk + row * P.pk();
  const uint8_t* sg = sig + row * P.sig();
  const uint8_t* dg = digest + row * P.m;

  Seeds<N> sd;
  {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = t < NW ? be32(pkr + 4 * t) : 0u;
    sd.s256 = sha::init();
    sha::compress(sd.s256, w);
    if constexpr (N > 16) {
      uint64_t v[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) v[t] = t < NW / 2 ? ((uint64_t)w[2 * t] << 32) | w[2 * t + 1] : 0ull;
      sd.s512 = sha::init512();
      sha::compress512(sd.s512, v);
    }
  }

  // md | idx_tree (8 bytes, big-endian, mod 2^(h - h')) | idx_leaf (1 byte, mod 2^h')
  uint64_t tree = ((uint64_t)be32(dg + P.md()) << 32) | be32(dg + P.md() + 4);
  if constexpr (P.h - P.hp < 64) tree &= (1ull << (P.h - P.hp)) - 1;  // 256f: all 64 bits, no shift by 64
  uint32_t leaf = dg[P.md() + 8] & ((1u << P.hp) - 1);

  // ---- FORS: lane i < k reconstructs root i
  if (lane < P.k) {
    const uint32_t idx = fors_index<PS>(dg, lane);
    const uint8_t* fs = sg + N + (size_t)lane * (P.a + 1) * N;
    uint32_t x[NW], au[NW];
    load_node<N>(fs, x);
    Adrs A{0, tree, FORS_TREE, leaf, 0, ((uint32_t)lane << P.a) + idx};
    hash_f<N>(sd, A, x);
#pragma unroll 1
    for (int j = 0; j < P.a; ++j) {
      load_node<N>(fs + (j + 1) * N, au);
      A.w2 = j + 1;
      A.w3 = ((uint32_t)lane << (P.a - j - 1)) + (idx >> (j + 1));
      hash_h<N>(sd, A, x, au, (idx >> j) & 1);
    }
    lds_put_node<N>(slice, lane, x);
  }
  if (lane == 0) lds_put_adrs(slice, Adrs{0, tree, FORS_ROOTS, leaf, 0, 0});
  wave_sync();
  uint32_t node[NW];
  t_lds<N>(sd, slice, 22 + P.k * N, node);
  wave_sync();
  if (TRACE && lane == 0) store_node<N>(tr.fors_pk + row * N, node);

  // ---- hypertree
  const uint8_t* xs = sg + N + P.fors_bytes();
#pragma unroll 1
  for (int layer = 0; layer < P.d; ++layer, xs += P.xmss_bytes()) {
    uint32_t csum = 0;  // sum of 15 - digit over the 2 n message digits, below 2^12
#pragma unroll
    for (int j = 0; j < NW; ++j) {
#pragma unroll
      for (int q = 0; q < 8; ++q) csum += 15 - ((node[j] >> (4 * q)) & 15);
    }
    for (int c = lane; c < LEN; c += 64) {
      uint32_t digit;
      if (c < P.len1()) {
        uint32_t wsel = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) wsel = (c >> 3) == j ? node[j] : wsel;
        digit = (wsel >> (28 - 4 * (c & 7))) & 15;
      } else {
        digit = (csum >> (4 * (LEN - 1 - c))) & 15;
      }
      uint32_t x[NW];
      load_node<N>(xs + (size_t)c * N, x);
      Adrs A{(uint32_t)layer, tree, WOTS_HASH, leaf, (uint32_t)c, 0};
#pragma unroll 1
      for (uint32_t s = 0; s < 15; ++s) {
        if (s >= digit) {
          A.w3 = s;
          hash_f<N>(sd, A, x);
        }
      }
      lds_put_node<N>(slice, c, x);
    }
    if (lane == 0) lds_put_adrs(slice, Adrs{(uint32_t)layer, tree, WOTS_PK, leaf, 0, 0});
    wave_sync();
    t_lds<N>(sd, slice, 22 + LEN * N, node);
    wave_sync();
#pragma unroll 1
    for (int j = 0; j < P.hp; ++j) {
      uint32_t au[NW];
      load_node<N>(xs + (size_t)(LEN + j) * N, au);
      hash_h<N>(sd, Adrs{(uint32_t)layer, tree, TREE, 0, (uint32_t)j + 1, leaf >> (j + 1)}, node, au, (leaf >> j) & 1);
    }
    if (TRACE && lane == 0) store_node<N>(tr.roots + (row * P.d + layer) * N, node);
    leaf = (uint32_t)tree & ((1u << P.hp) - 1);
    tree >>= P.hp;
  }

  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < NW; ++j) diff |= node[j] ^ be32(pkr + N + 4 * j);
  const uint32_t fl = diff ? FLAG_ROOT : 0;
  if (lane == 0) status[row] = fl ? -1 : 0;
  if (TRACE) {
    for (int b = lane; b < P.m; b += 64) tr.digest[row * P.m + b] = dg[b];
    if (lane == 0) tr.flags[row] = fl;
  }
}

// scratch of a chunk of C rows: flags | digest
struct Layout {
  uint32_t* flags;
  uint8_t* digest;
  size_t bytes;
};
static Layout layout(const Params& P, size_t C, void* scratch) {
  uint8_t* p = (uint8_t*)scratch;
  Layout l;
  l.flags = (uint32_t*)p;
  l.digest = p + C * sizeof(uint32_t);
  l.bytes = C * (sizeof(uint32_t) + P.m);
  return l;
}

template <int PS>
static hipError_t run(size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* off, const uint8_t* sig,
                      const uint8_t* ctx, size_t ctx_len, int32_t* status, const SlhdsaTrace& tr, void* scratch,
                      hipStream_t st) {
  const Layout l = layout(make(PS), n, scratch);
  const dim3 lanes((unsigned)((n + 63) / 64)), waves((unsigned)((n + 3) / 4));
  QRK_LAUNCH("k_slhdsa_front", st, k_slhdsa_front<PS>, lanes, dim3(64), 0, st, n, pk, msg, off, sig, ctx,
             (uint32_t)ctx_len, l.digest, l.flags);
  if (tr.flags)
    QRK_LAUNCH("k_slhdsa_core", st, (k_slhdsa_core<PS, true>), waves, dim3(256), 0, st, n, pk, sig, l.digest, l.flags,
               status, tr);
  else
    QRK_LAUNCH("k_slhdsa_core", st, (k_slhdsa_core<PS, false>), waves, dim3(256), 0, st, n, pk, sig, l.digest, l.flags,
               status, tr);
  return launch_status();
}

}  // namespace slhdsa

int slhdsa_find(const char* name) {
  static const char* const NAMES[6] = {"SPHINCS+-SHA2-128f-simple", "SLH-DSA-SHA2-128f", "SPHINCS+-SHA2-192f-simple",
                                       "SLH-DSA-SHA2-192f",         "SPHINCS+-SHA2-256f-simple", "SLH-DSA-SHA2-256f"};
  for (int i = 0; name && i < 6; ++i)
    if (!strcmp(name, NAMES[i])) return i;
  return -1;
}

bool slhdsa_is_fips(int which) { return which & 1; }

void slhdsa_sizes(int which, size_t out[6]) {
  const slhdsa::Params P = slhdsa::make(which);
  out[0] = P.pk(), out[1] = P.sk(), out[2] = P.sig(), out[3] = P.m, out[4] = P.n, out[5] = P.d;
}

size_t slhdsa_scratch_bytes(int which, size_t chunk) {
  return slhdsa::layout(slhdsa::make(which), chunk, nullptr).bytes;
}

hipError_t slhdsa_verify(int which, size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* msg_off,
                         const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len, int32_t* status,
                         const SlhdsaTrace& trace, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || (ctx_len && !slhdsa_is_fips(which)) || n > (1u << 24)) return hipErrorInvalidValue;
  switch (which) {
    case 0: return slhdsa::run<0>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
    case 1: return slhdsa::run<1>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
    case 2: return slhdsa::run<2>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
    case 3: return slhdsa::run<3>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
    case 4: return slhdsa::run<4>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
    case 5: return slhdsa::run<5>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace qrk
