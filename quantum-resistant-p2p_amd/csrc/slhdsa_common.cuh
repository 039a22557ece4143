// Device helpers shared by SLH-DSA-SHA2 / SPHINCS+-SHA2-simple verification (slhdsa.hip) and key generation
// and signing (slhdsa_sign.hip): the parameter sets, the compressed address, the PK.seed states and the tweakable
// hashes F / H / T_l seeded with them, H_msg, the LDS node stream, a digest's FORS, tree and leaf indices and the
// WOTS+ digits.  Everything here works on public data or is constant-time in its inputs (the SHA-2 rounds);
// PRF(PK.seed, SK.seed, ADRS) has F's shape and is hash_f on SK.seed with a PRF-type address.
#pragma once
#include "qrkem_internal.h"
#include "sha2.cuh"

namespace qrk {
namespace slhdsa {

enum : uint32_t { FLAG_ROOT = 1, FLAG_LONG = 2 };
enum : uint32_t { WOTS_HASH = 0, WOTS_PK = 1, TREE = 2, FORS_TREE = 3, FORS_ROOTS = 4, WOTS_PRF = 5, FORS_PRF = 6 };

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

// Start and length of ragged row `row`; false (FLAG_LONG) for decreasing offsets or 2^31 bytes or more.
__device__ __forceinline__ bool row_span(const uint64_t* off, size_t row, uint64_t& o0, uint32_t& mlen) {
  o0 = off[row];
  const uint64_t o1 = off[row + 1];
  if (o1 < o0 || o1 - o0 >= (1ull << 31)) return false;
  mlen = (uint32_t)(o1 - o0);
  return true;
}

// Byte q of M' (FIPS 205 Algorithm 22 / 24: M' = 0 || len(ctx) || ctx || M; round 3.1: M itself).
template <int PS>
__device__ __forceinline__ uint32_t frame_at(uint32_t q, const uint8_t* m, const uint8_t* ctx, uint32_t ctx_len) {
  if (make(PS).fips) {
    if (q < 2) return q ? ctx_len : 0u;
    q -= 2;
    if (q < ctx_len) return ctx[q];
    q -= ctx_len;
  }
  return m[q];
}

// ------------------------------------------------------------------ H_msg
// out[0 .. m) = H_msg(R, PK.seed, PK.root, M') = MGF1-SHA-X(R || PK.seed || SHA-X(R || PK.seed || PK.root ||
// M'), m) in one lane; r: R (n bytes), pkr: PK.seed || PK.root, m / mlen: M (below 2^31 bytes).
template <int PS>
__device__ __forceinline__ void h_msg(const uint8_t* r, const uint8_t* pkr, const uint8_t* m, uint32_t mlen,
                                      const uint8_t* ctx, uint32_t ctx_len, uint8_t* out) {
  using namespace sha;
  constexpr Params P = make(PS);
  constexpr uint32_t N = P.n;
  const uint32_t pre = P.fips ? 2 + ctx_len : 0;
  auto none32 = [](uint32_t, int, uint32_t x) { return x; };
  auto none64 = [](uint32_t, int, uint64_t x) { return x; };
  // R || PK.seed || PK.root || M'
  auto inner_at = [&](uint32_t p) -> uint32_t {
    if (p < N) return r[p];
    if (p < 3 * N) return pkr[p - N];
    return frame_at<PS>(p - 3 * N, m, ctx, ctx_len);
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
// ... computed from w = PK.seed || 0^(64 - n) as big-endian words: SHA-256 after w, and for n > 16 SHA-512 after
// PK.seed || 0^(128 - n).  In parts, so that a caller that only stores them (slhdsa_sign.hip) holds one at a time.
template <int N>
__device__ __forceinline__ void seed_block(const uint8_t* pk_seed, uint32_t w[16]) {
#pragma unroll
  for (int t = 0; t < 16; ++t) w[t] = t < N / 4 ? be32(pk_seed + 4 * t) : 0u;
}
__device__ __forceinline__ sha::H8 seed_state256(const uint32_t w[16]) {
  sha::H8 s = sha::init();
  sha::compress(s, w);
  return s;
}
template <int N>
__device__ __forceinline__ sha::H8x64 seed_state512(const uint32_t w[16]) {
  uint64_t v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) v[t] = t < N / 8 ? ((uint64_t)w[2 * t] << 32) | w[2 * t + 1] : 0ull;
  sha::H8x64 s = sha::init512();
  sha::compress512(s, v);
  return s;
}
template <int N>
__device__ __forceinline__ Seeds<N> seed_states(const uint8_t* pk_seed) {
  Seeds<N> sd;
  uint32_t w[16];
  seed_block<N>(pk_seed, w);
  sd.s256 = seed_state256(w);
  if constexpr (N > 16) sd.s512 = seed_state512<N>(w);
  return sd;
}

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

// md | idx_tree (8 bytes, big-endian, mod 2^(h - h')) | idx_leaf (1 byte, mod 2^h'): the indices of layer 0
template <int PS>
__device__ __forceinline__ void digest_indices(const uint8_t* dg, uint64_t& tree, uint32_t& leaf) {
  constexpr Params P = make(PS);
  tree = ((uint64_t)be32(dg + P.md()) << 32) | be32(dg + P.md() + 4);
  if constexpr (P.h - P.hp < 64) tree &= (1ull << (P.h - P.hp)) - 1;  // 256f: all 64 bits, no shift by 64
  leaf = dg[P.md() + 8] & ((1u << P.hp) - 1);
}
// ... and from those of one hypertree layer the next one's: h' bits at a time, never a shift by 64
template <int PS>
__device__ __forceinline__ void next_layer(uint64_t& tree, uint32_t& leaf) {
  constexpr Params P = make(PS);
  leaf = (uint32_t)tree & ((1u << P.hp) - 1);
  tree >>= P.hp;
}

// WOTS+ (lg_w = 4) over a node: the checksum, sum of 15 - digit over the 2 n message digits (below 2^12), and the
// digit of chain c: for c < 2 n from `word`, the node's word c >> 3, for the other three from the checksum.
template <int N>
__device__ __forceinline__ uint32_t wots_csum(const uint32_t* node) {
  uint32_t csum = 0;
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
#pragma unroll
    for (int q = 0; q < 8; ++q) csum += 15 - ((node[j] >> (4 * q)) & 15);
  }
  return csum;
}
__device__ __forceinline__ uint32_t wots_msg_digit(uint32_t c, uint32_t word) { return (word >> (28 - 4 * (c & 7))) & 15; }
template <int N>
__device__ __forceinline__ uint32_t wots_csum_digit(uint32_t c, uint32_t csum) {
  return (csum >> (4 * (2 * N + 2 - c))) & 15;
}

}  // namespace slhdsa
}  // namespace qrk
