// AEAD for long messages on gfx950: one row sealed or opened across many workgroups, byte for byte what
// aead.hip's one-lane kernels return (qrk_aead_seal_long_batch / qrk_aead_open_long_batch).
//
// The reference sends a file by reading it whole and passing it to one SymmetricAlgorithm.encrypt call
// (app/messaging.py:1707-1713 -> send_message -> :1645) and opens it with one decrypt (:1465).  In aead.hip
// that is one lane walking the whole message; here the row is cut into segments of S = 256 C bytes
// (LONG_C = 256, S = 64 KiB), one 256-lane workgroup per segment, each lane owning C consecutive bytes.
//
// Geometry.  The MAC of both AEADs is a Horner walk y = (y + X_j) K over the 16-byte blocks X_j of the
// ciphertext (K = H in GF(2^128), or r mod 2^130 - 5 with every block carrying the 2^128 bit: RFC 8439's
// pad16 makes every block of aad | ct | lens full).  A block of zeros absorbed into a zero accumulator
// leaves it zero, so padding is free at the front and at the front only.  A row of nb blocks is therefore
// laid out right-aligned: with nseg = ceil(nb / 4096) segments it is preceded by pad = 4096 nseg - nb
// virtual blocks that no lane touches, lane t of segment g owns virtual blocks [(256 g + t) 16, + 16), and
// every lane's walk ends on a 16-block boundary.  All raggedness sits in the first segment (its first lanes
// have nothing to do, one lane has a short walk) and every combine step below multiplies by one uniform
// power of K: no step needs a length-dependent exponent.  The lane that owns block 0 starts from the
// accumulator of the associated data, absorbed serially (it is a message id: short).
//
// Within the workgroup: lane partials y_t combine as sum_t y_t Q^(255 - t), Q = K^16, by a log-step tree:
// six cross-lane steps y_t = y_t Q^(2^k) + y_(t + 2^k) inside each wave (Q squared between steps), then the
// four wave results through LDS.  Across segments: the partial of segment g goes to context scratch and a
// tail workgroup per row (64 lanes) combines them the same way over M = K^4096: every lane walks
// cnt = ceil(nseg / 64) consecutive partials (right-aligned again), then the same six-step tree over
// M^cnt.  A 2^31-byte row has 2^15 segments: 512 multiplies per lane and six tree steps, not 2^15 in a row.
// The tail then absorbs the length block, adds E_K(J0) or s, and on Seal writes nonce and tag; on Open it
// compares without early exit and writes the row's verdict, and a second pass over the segments decrypts
// the rows whose verdict is 0 and writes zeros over the plaintext span of those whose tag did not match.
//
// Keys.  Every workgroup derives what it needs from the caller's key buffer itself (AES-256 key schedule and
// H = E_K(0), or the ChaCha key state and the Poly1305 one-time key from block 0); no round key, H, r or s
// is a kernel argument or goes to global memory.  The segment partials are secret-derived (H or r can be
// solved from one and the public ciphertext): they live only in context scratch, the tail overwrites its
// row's whole partial span with zeros once consumed, and qrk_ctx_cleanse covers the scratch.
//
// Multiplies: the bit-serial masked gf128_mul of aead_dev.cuh, and 26-bit-limb products with 64-bit column
// sums; no branch or address depends on H, r or an accumulator.  Branches on lengths, counters and the
// verdict are public.
#include "aead_dev.cuh"

namespace qrk {
namespace aead {

constexpr uint32_t LONG_C = 256, LONG_S = 256 * LONG_C;      // bytes per lane, per segment
constexpr uint32_t LANE_BLOCKS = LONG_C / 16, SEG_BLOCKS = LONG_S / 16;
constexpr uint32_t TAIL_LANES = 64;                          // fan-in of the tail's lane walk + tree
static_assert(LONG_C % 64 == 0 && (SEG_BLOCKS & (SEG_BLOCKS - 1)) == 0, "segment geometry");

// ------------------------------------------------------------------ the two MACs as one interface
// V: an accumulator or a power of the multiplier.  mul(y, p): y = y p.  add(y, x): y = y + x.
// absorb(y, m): y = (y + block m) K, m the block's 16 bytes as four little-endian words.
struct GhashMac {
  static constexpr int W = 4, STORE = 4;  // words of a value, words of a scratch slot
  uint32_t k[4];                          // H, big-endian words as gf128_mul takes them
  __device__ __forceinline__ static void one(uint32_t v[W]) { v[0] = 0x80000000u, v[1] = v[2] = v[3] = 0; }
  __device__ __forceinline__ static void mul(uint32_t y[W], const uint32_t p[W]) {
    const uint32_t q[4] = {p[0], p[1], p[2], p[3]};  // p may be y
    gf128_mul(y, q);
  }
  __device__ __forceinline__ static void add(uint32_t y[W], const uint32_t x[W]) {
#pragma unroll
    for (int t = 0; t < W; ++t) y[t] ^= x[t];
  }
  __device__ __forceinline__ void absorb(uint32_t y[W], const uint32_t m[4]) const {
#pragma unroll
    for (int t = 0; t < 4; ++t) y[t] ^= bswap(m[t]);
    gf128_mul(y, k);
  }
};

struct PolyMac {
  static constexpr int W = 5, STORE = 8;
  uint32_t k[5];  // r, clamped, 26-bit limbs
  __device__ __forceinline__ static void one(uint32_t v[W]) { v[0] = 1, v[1] = v[2] = v[3] = v[4] = 0; }
  // y = y p mod 2^130 - 5, partially carried.  With the limbs of p below 2^27 (5 p below 2^29.4) any
  // 32-bit limbs of y keep the five column sums below 2^64; the result has limb 1 below 2^26 + 2^13 and
  // the others below 2^26.  Between two multiplies an accumulator takes at most 15 such values in add().
  __device__ __forceinline__ static void mul(uint32_t y[W], const uint32_t p[W]) {
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4];
    const uint32_t s1 = 5 * p1, s2 = 5 * p2, s3 = 5 * p3, s4 = 5 * p4;
    const uint32_t h0 = y[0], h1 = y[1], h2 = y[2], h3 = y[3], h4 = y[4];
    auto m = [](uint32_t a, uint32_t b) { return (uint64_t)a * b; };
    uint64_t d0 = m(h0, p0) + m(h1, s4) + m(h2, s3) + m(h3, s2) + m(h4, s1);
    uint64_t d1 = m(h0, p1) + m(h1, p0) + m(h2, s4) + m(h3, s3) + m(h4, s2);
    uint64_t d2 = m(h0, p2) + m(h1, p1) + m(h2, p0) + m(h3, s4) + m(h4, s3);
    uint64_t d3 = m(h0, p3) + m(h1, p2) + m(h2, p1) + m(h3, p0) + m(h4, s4);
    uint64_t d4 = m(h0, p4) + m(h1, p3) + m(h2, p2) + m(h3, p1) + m(h4, p0);
    uint64_t c = d0 >> 26;
    d1 += c, c = d1 >> 26;
    d2 += c, c = d2 >> 26;
    d3 += c, c = d3 >> 26;
    d4 += c, c = d4 >> 26;
    const uint64_t f = (d0 & 0x3ffffff) + c * 5;
    y[0] = (uint32_t)f & 0x3ffffff;
    y[1] = ((uint32_t)d1 & 0x3ffffff) + (uint32_t)(f >> 26);
    y[2] = (uint32_t)d2 & 0x3ffffff, y[3] = (uint32_t)d3 & 0x3ffffff, y[4] = (uint32_t)d4 & 0x3ffffff;
  }
  __device__ __forceinline__ static void add(uint32_t y[W], const uint32_t x[W]) {
#pragma unroll
    for (int t = 0; t < W; ++t) y[t] += x[t];
  }
  // every block is 16 full bytes and carries the 2^128 bit (1 << 24 in the top limb)
  __device__ __forceinline__ void absorb(uint32_t y[W], const uint32_t m[4]) const {
    y[0] += m[0] & 0x3ffffff, y[1] += ((m[0] >> 26) | (m[1] << 6)) & 0x3ffffff;
    y[2] += ((m[1] >> 20) | (m[2] << 12)) & 0x3ffffff, y[3] += ((m[2] >> 14) | (m[3] << 18)) & 0x3ffffff;
    y[4] += (m[3] >> 8) | (1u << 24);
    mul(y, k);
  }
};

template <class M>
__device__ __forceinline__ void zero(uint32_t v[M::W]) {
#pragma unroll
  for (int t = 0; t < M::W; ++t) v[t] = 0;
}
// p = p^(2^k)
template <class M>
__device__ __forceinline__ void square_times(uint32_t p[M::W], int k) {
#pragma unroll 1
  for (int s = 0; s < k; ++s) M::mul(p, p);
}
// Lane 0 of each wave gets sum_(t < 64) y_t q^(63 - t) over the wave's lanes; q becomes q^64.  Every lane
// runs every step: lane 0's result depends on lane 2^k at step k, whose own inputs lie below lane 64, so
// what a lane near the end of the wave reads past it (its own value) never reaches lane 0.
template <class M>
__device__ __forceinline__ void wave_tree(uint32_t y[M::W], uint32_t q[M::W]) {
#pragma unroll 1
  for (int s = 1; s < 64; s <<= 1) {
    uint32_t o[M::W];
#pragma unroll
    for (int t = 0; t < M::W; ++t) o[t] = __shfl_down(y[t], s, 64);
    M::mul(y, q);
    M::add(y, o);
    M::mul(q, q);
  }
}

// ------------------------------------------------------------------ arguments and rows
// Everything a launch needs, by value.  keys / nonces point into the caller's buffers: no key material here.
struct LongArgs {
  size_t n;
  const uint8_t *keys, *nonces, *in;
  const uint64_t* off;
  const uint8_t* aad;
  const uint64_t* aad_off;
  uint32_t aad_len, max_len, nseg_max;
  uint8_t* out;
  int32_t* status;
  uint32_t* part;    // context scratch: [n][nseg_max][STORE] words
  int32_t* verdict;  // context scratch: [n]
};
enum { SEAL = 0, OPEN_MAC = 1, OPEN_DEC = 2, DBG = 3 };
enum : int32_t { V_OK = 0, V_BAD_TAG = -1, V_REFUSED = -2 };

struct Row {
  bool ok;
  uint32_t len, nb, nseg, pad;  // payload bytes, 16-byte blocks, segments, virtual blocks in front
  const uint8_t *in, *nonce;    // payload in, 12 nonce bytes
  uint8_t* out;                 // Seal: the sealed row; Open: the plaintext; DBG: the 16-byte result
  Span ad;
};
template <int MODE>
__device__ __forceinline__ Row row_of(const LongArgs& a, size_t i) {
  Row r;
  const uint64_t o = a.off[i], l64 = a.off[i + 1] - o;  // decreasing offsets wrap to a length >= 2^63
  r.ad = MODE == DBG ? Span{nullptr, 0, true} : span_of(a.aad, a.aad_off, a.aad_len, i);
  if (MODE == SEAL) {
    r.ok = l64 <= a.max_len && r.ad.ok;
    r.len = (uint32_t)l64, r.in = a.in + o, r.nonce = a.nonces + NONCE * i, r.out = a.out + o + OVERHEAD * i;
  } else if (MODE == DBG) {
    r.ok = l64 <= a.max_len;
    r.len = (uint32_t)l64 & ~15u, r.in = a.in + o, r.nonce = nullptr, r.out = a.out + 16 * i;
  } else {
    // (o < 28 i: rows before this one were shorter than 28 bytes and its plaintext has no place)
    r.ok = l64 >= OVERHEAD && l64 - OVERHEAD <= a.max_len && r.ad.ok && o >= (uint64_t)OVERHEAD * i;
    r.len = (uint32_t)l64 - OVERHEAD, r.nonce = a.in + o, r.in = a.in + o + NONCE;
    r.out = a.out + (o - OVERHEAD * i);
  }
  r.nb = (r.len + 15) / 16;  // max_len < 2^31: no overflow
  r.nseg = (r.nb + SEG_BLOCKS - 1) / SEG_BLOCKS;
  r.pad = r.nseg * SEG_BLOCKS - r.nb;
  return r;
}

// 16 bytes at p + pos as four little-endian words, bytes at or past len read as zero
__device__ __forceinline__ void load_block(const uint8_t* p, uint32_t pos, uint32_t len, uint32_t m[4]) {
  if (pos + 16 <= len) {
    __builtin_memcpy(m, p + pos, 16);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) m[t] = gather32(p, pos + 4 * t, len);
  }
}
__device__ __forceinline__ void store_block(uint8_t* p, uint32_t pos, uint32_t len, const uint32_t m[4]) {
  if (pos + 16 <= len) {
    __builtin_memcpy(p + pos, m, 16);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) scatter32(p, pos + 4 * t, len, m[t]);
  }
}
// all ones over the bytes of word t of the block at pos that lie below len
__device__ __forceinline__ uint32_t valid_mask(uint32_t pos, uint32_t len, int t) {
  const uint32_t at = pos + 4 * t;
  const uint32_t v = at >= len ? 0 : (len - at >= 4 ? 4 : len - at);
  return v >= 4 ? ~0u : (1u << (8 * v)) - 1;
}

// ------------------------------------------------------------------ the algorithms behind the kernels
// init(L, key, nonce); mac: the MAC under this row's key; keystream(L, j, ks): the 16 keystream bytes of
// payload block j; aad(y): y = the MAC accumulator after the associated data; finish(L, y, ad_len, len, t):
// the 16 tag bytes from the accumulator after aad and payload.
struct GcmLong {
  static constexpr bool LDS = true;
  using Mac = GhashMac;
  Gcm G;
  Mac mac;
  __device__ __forceinline__ void init(const aes::Lds2& L, const uint8_t* key, const uint8_t* nonce) {
    G.init(L, key, nonce);
#pragma unroll
    for (int t = 0; t < 4; ++t) mac.k[t] = G.h[t];
  }
  __device__ __forceinline__ void keystream(const aes::Lds2& L, uint32_t j, uint32_t ks[4]) { G.counter_block(L, 2 + j, ks); }
  __device__ __forceinline__ void aad(const Span& ad, uint32_t y[4]) const { ghash_padded(y, G.h, ad.p, ad.len); }
  __device__ __forceinline__ void finish(const aes::Lds2& L, uint32_t y[4], uint32_t ad_len, uint32_t len,
                                         uint32_t tag[4]) const {
    y[0] ^= ad_len >> 29, y[1] ^= ad_len << 3, y[2] ^= len >> 29, y[3] ^= len << 3;
    gf128_mul(y, G.h);
    G.counter_block(L, 1, tag);
#pragma unroll
    for (int t = 0; t < 4; ++t) tag[t] ^= bswap(y[t]);
  }
};

struct ChaLong {
  static constexpr bool LDS = false;
  using Mac = PolyMac;
  ChaKey K;
  Poly P;  // the one-time key: r in mac.k too, s in P.pad
  Mac mac;
  uint32_t ks64[16], have;
  __device__ __forceinline__ void init(const aes::Lds2&, const uint8_t* key, const uint8_t* nonce) {
    K = chacha_key(key, nonce);
    uint32_t b0[16];
    chacha_block(K, 0, b0);
    P.init(b0);
#pragma unroll
    for (int t = 0; t < 5; ++t) mac.k[t] = P.r[t];
    have = ~0u;
  }
  // payload block j lies in ChaCha block 1 + j / 4, computed when the walk enters it (a lane's 16 blocks
  // start on a multiple of 4 only when the row's length does: up to five ChaCha blocks per lane, not four)
  __device__ __forceinline__ void keystream(const aes::Lds2&, uint32_t j, uint32_t ks[4]) {
    if ((j >> 2) != have) {
      have = j >> 2;
      chacha_block(K, 1 + have, ks64);
    }
    const uint32_t q = j & 3;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      ks[t] = q == 0 ? ks64[t] : q == 1 ? ks64[4 + t] : q == 2 ? ks64[8 + t] : ks64[12 + t];
  }
  __device__ __forceinline__ void aad(const Span& ad, uint32_t y[5]) const {
#pragma unroll 1
    for (uint32_t b = 0; b < ad.len; b += 16) {
      uint32_t m[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) m[t] = gather32(ad.p, b + 4 * t, ad.len);
      mac.absorb(y, m);
    }
  }
  __device__ __forceinline__ void finish(const aes::Lds2&, uint32_t y[5], uint32_t ad_len, uint32_t len, uint32_t tag[4]) {
    const uint32_t lens[4] = {ad_len, 0, len, 0};
    mac.absorb(y, lens);
#pragma unroll
    for (int t = 0; t < 5; ++t) P.h[t] = y[t];
    P.finish(tag);
  }
};

// tests: GHASH under a chosen H, Poly1305 under a chosen key32 = r | s, over whole blocks; no cipher
struct GhashDbg {
  static constexpr bool LDS = false;
  using Mac = GhashMac;
  Mac mac;
  __device__ __forceinline__ void init(const aes::Lds2&, const uint8_t* key, const uint8_t*) {
#pragma unroll
    for (int t = 0; t < 4; ++t) mac.k[t] = bswap(load32(key + 4 * t));
  }
  __device__ __forceinline__ void keystream(const aes::Lds2&, uint32_t, uint32_t[4]) {}
  __device__ __forceinline__ void aad(const Span&, uint32_t[4]) const {}
  __device__ __forceinline__ void finish(const aes::Lds2&, uint32_t y[4], uint32_t, uint32_t, uint32_t tag[4]) const {
#pragma unroll
    for (int t = 0; t < 4; ++t) tag[t] = bswap(y[t]);
  }
};
struct PolyDbg {
  static constexpr bool LDS = false;
  using Mac = PolyMac;
  Poly P;
  Mac mac;
  __device__ __forceinline__ void init(const aes::Lds2&, const uint8_t* key, const uint8_t*) {
    uint32_t k[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) k[t] = load32(key + 4 * t);
    P.init(k);
#pragma unroll
    for (int t = 0; t < 5; ++t) mac.k[t] = P.r[t];
  }
  __device__ __forceinline__ void keystream(const aes::Lds2&, uint32_t, uint32_t[4]) {}
  __device__ __forceinline__ void aad(const Span&, uint32_t[5]) const {}
  __device__ __forceinline__ void finish(const aes::Lds2&, uint32_t y[5], uint32_t, uint32_t, uint32_t tag[4]) {
#pragma unroll
    for (int t = 0; t < 5; ++t) P.h[t] = y[t];
    P.finish(tag);
  }
};
template <class A>
constexpr uint32_t key_stride() { return std::is_same<A, GhashDbg>::value ? 16u : 32u; }

// the LDS T-table for the algorithms that use AES, after the workgroup's (uniform) early exits
#define QRK_LONG_LDS_TABLE(A, NTHREADS)                                                                \
  __shared__ __attribute__((aligned(16))) uint32_t tab[A::LDS ? 256 * 64 : 32];                        \
  if (A::LDS) {                                                                                        \
    aes::fill_lds2(tab, threadIdx.x, NTHREADS);                                                        \
    __syncthreads();                                                                                   \
  }                                                                                                    \
  const aes::Lds2 L{(const char*)tab, (uint32_t)(threadIdx.x & 31) * 4u, 128u + (uint32_t)(threadIdx.x & 31) * 4u}

// ------------------------------------------------------------------ one segment of one row
// grid: n nseg_max workgroups of 256, workgroup b = segment b % nseg_max of row b / nseg_max.
// SEAL: encrypt and MAC the ciphertext from registers.  OPEN_MAC, DBG: MAC the input.  OPEN_DEC: the second
// pass of Open, under the row's verdict.  The MAC modes leave the segment's partial in a.part.
template <class A, int MODE>
__global__ __launch_bounds__(256) void k_long_seg(const LongArgs a) {
  using M = typename A::Mac;
  const uint32_t g = blockIdx.x % a.nseg_max;
  const size_t i = blockIdx.x / a.nseg_max;
  const Row r = row_of<(MODE == OPEN_DEC ? (int)OPEN_MAC : MODE)>(a, i);
  if (!r.ok || g >= r.nseg) return;  // the whole workgroup, before it touches the row
  int32_t verdict = V_OK;
  if (MODE == OPEN_DEC) {
    verdict = a.verdict[i];
    if (verdict == V_REFUSED) return;
  }
  QRK_LONG_LDS_TABLE(A, 256);
  A alg;
  if (MODE != OPEN_DEC || verdict == V_OK) alg.init(L, a.keys + key_stride<A>() * i, r.nonce);
  uint8_t* const dst = MODE == SEAL ? r.out + NONCE : r.out;

  uint32_t y[M::W];
  zero<M>(y);
  const uint32_t v0 = (g * 256 + threadIdx.x) * LANE_BLOCKS;  // below 2^27 + 4096
#pragma unroll 1
  for (uint32_t k = 0; k < LANE_BLOCKS; ++k) {
    if (v0 + k < r.pad) continue;
    const uint32_t j = v0 + k - r.pad, pos = 16 * j;
    uint32_t m[4];
    if (MODE == OPEN_DEC && verdict != V_OK) {
      m[0] = m[1] = m[2] = m[3] = 0;  // no plaintext byte of an unauthenticated row is written
      store_block(dst, pos, r.len, m);
      continue;
    }
    if (MODE != OPEN_DEC && j == 0) alg.aad(r.ad, y);
    load_block(r.in, pos, r.len, m);
    if (MODE == SEAL || MODE == OPEN_DEC) {
      uint32_t ks[4];
      alg.keystream(L, j, ks);
#pragma unroll
      for (int t = 0; t < 4; ++t) m[t] ^= ks[t];
      store_block(dst, pos, r.len, m);
      if (MODE == SEAL && pos + 16 > r.len) {
#pragma unroll
        for (int t = 0; t < 4; ++t) m[t] &= valid_mask(pos, r.len, t);  // the MAC pads with zeros
      }
    }
    if (MODE != OPEN_DEC) alg.mac.absorb(y, m);
  }
  if (MODE == OPEN_DEC) return;

  uint32_t q[M::W];
#pragma unroll
  for (int t = 0; t < M::W; ++t) q[t] = alg.mac.k[t];
  square_times<M>(q, 4);  // K^16: LANE_BLOCKS blocks
  static_assert(LANE_BLOCKS == 16, "the lane power");
  wave_tree<M>(y, q);     // q = K^(16 * 64)
  // the four wave results meet in the first words of the table's LDS, once no wave reads the table any more
  static_assert(4 * M::STORE <= 32, "the wave results fit the smallest table");
  uint32_t(*wsum)[M::STORE] = (uint32_t(*)[M::STORE])tab;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int t = 0; t < M::W; ++t) wsum[threadIdx.x >> 6][t] = y[t];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
      uint32_t o[M::W];
#pragma unroll
      for (int t = 0; t < M::W; ++t) o[t] = wsum[w][t];
      M::mul(y, q);
      M::add(y, o);
    }
    uint32_t* slot = a.part + ((size_t)i * a.nseg_max + g) * M::STORE;
#pragma unroll
    for (int t = 0; t < M::STORE; ++t) slot[t] = t < M::W ? y[t] : 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      for (int t = 0; t < M::W; ++t) wsum[w][t] = 0;
  }
}

// ------------------------------------------------------------------ the tail: one 64-lane workgroup per row
// Combines the row's segment partials, zeroes the row's partial span, finishes the tag.  SEAL: writes nonce
// and tag (a refused row is left unwritten).  OPEN_MAC: compares, writes status and the verdict.  DBG:
// writes the 16 result bytes.
template <class A, int MODE>
__global__ __launch_bounds__(TAIL_LANES) void k_long_tail(const LongArgs a) {
  using M = typename A::Mac;
  const size_t i = blockIdx.x;
  const uint32_t u = threadIdx.x;
  const Row r = row_of<MODE>(a, i);
  uint32_t* const part = a.part + (size_t)i * a.nseg_max * M::STORE;
  if (!r.ok) {
    for (size_t w = u; w < (size_t)a.nseg_max * M::STORE; w += TAIL_LANES) part[w] = 0;
    if (MODE == OPEN_MAC && u == 0) a.status[i] = -1, a.verdict[i] = V_REFUSED;
    return;
  }
  QRK_LONG_LDS_TABLE(A, TAIL_LANES);
  A alg;
  alg.init(L, a.keys + key_stride<A>() * i, r.nonce);

  uint32_t y[M::W];
  zero<M>(y);
  if (r.nseg == 0) {
    alg.aad(r.ad, y);  // an empty payload: the accumulator after the associated data (every lane; lane 0's is used)
  } else {
    uint32_t mp[M::W];
#pragma unroll
    for (int t = 0; t < M::W; ++t) mp[t] = alg.mac.k[t];
    square_times<M>(mp, 12);  // M = K^4096: one segment
    static_assert(SEG_BLOCKS == 4096, "the segment power");
    const uint32_t cnt = (r.nseg + TAIL_LANES - 1) / TAIL_LANES, padseg = TAIL_LANES * cnt - r.nseg;
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; ++k) {
      if (u * cnt + k < padseg) continue;
      const uint32_t* slot = part + (size_t)(u * cnt + k - padseg) * M::STORE;
      uint32_t p[M::W];
#pragma unroll
      for (int t = 0; t < M::W; ++t) p[t] = slot[t];
      M::mul(y, mp);
      M::add(y, p);
    }
    // M^cnt by square and multiply over the (public) count
    uint32_t q[M::W];
    M::one(q);
#pragma unroll 1
    for (uint32_t e = cnt; e; e >>= 1) {
      if (e & 1) M::mul(q, mp);
      M::mul(mp, mp);
    }
    wave_tree<M>(y, q);
  }
  // consumed (or never written): the row's whole partial span is zero when the call is over.  All of this
  // workgroup's reads of it are done: the tree above exchanged registers after them.
  __syncthreads();
  for (size_t w = u; w < (size_t)a.nseg_max * M::STORE; w += TAIL_LANES) part[w] = 0;
  if (u != 0) return;

  uint32_t tag[4];
  alg.finish(L, y, r.ad.len, r.len, tag);
  if (MODE == SEAL) {
#pragma unroll
    for (int t = 0; t < 3; ++t) scatter32(r.out, 4 * t, NONCE, load32(r.nonce + 4 * t));
#pragma unroll
    for (int t = 0; t < 4; ++t) scatter32(r.out + NONCE + r.len, 4 * t, TAG, tag[t]);
  } else if (MODE == OPEN_MAC) {
    uint32_t d = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) d |= tag[t] ^ load32(r.in + r.len + 4 * t);
    const bool ok = d == 0;
    a.status[i] = ok ? 0 : -1;
    a.verdict[i] = ok ? V_OK : V_BAD_TAG;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) scatter32(r.out, 4 * t, TAG, tag[t]);
  }
}

}  // namespace aead

// ------------------------------------------------------------------ launchers
void aead_long_layout(AeadAlg alg, size_t out[4]) {
  out[0] = aead::LONG_S, out[1] = aead::LONG_C, out[2] = aead::TAIL_LANES;
  out[3] = 4 * (alg == AeadAlg::AES_256_GCM ? aead::GhashMac::STORE : aead::PolyMac::STORE);
}
static size_t long_segments(size_t max_len) { return (max_len + aead::LONG_S - 1) / aead::LONG_S; }
size_t aead_long_part_bytes(AeadAlg alg, size_t n, size_t max_len) {
  size_t lay[4];
  aead_long_layout(alg, lay);
  return n * long_segments(max_len) * lay[3];
}
size_t aead_long_scratch_bytes(AeadAlg alg, size_t n, size_t max_len) {
  return aead_long_part_bytes(alg, n, max_len) + 4 * n;
}
size_t aead_long_workgroups(size_t n, size_t max_len) { return n * long_segments(max_len); }

static aead::LongArgs long_args(AeadAlg alg, size_t n, size_t max_len, void* scratch) {
  aead::LongArgs a{};
  a.n = n, a.max_len = (uint32_t)max_len, a.nseg_max = (uint32_t)long_segments(max_len);
  a.part = (uint32_t*)scratch;
  a.verdict = (int32_t*)((char*)scratch + aead_long_part_bytes(alg, n, max_len));
  return a;
}
template <class A, int MODE>
static void launch_seg(const char* name, const aead::LongArgs& a, hipStream_t st) {
  QRK_LAUNCH(name, st, (aead::k_long_seg<A, MODE>), dim3((unsigned)(a.n * a.nseg_max)), dim3(256), 0, st, a);
}
template <class A, int MODE>
static void launch_tail(const char* name, const aead::LongArgs& a, hipStream_t st) {
  QRK_LAUNCH(name, st, (aead::k_long_tail<A, MODE>), dim3((unsigned)a.n), dim3(aead::TAIL_LANES), 0, st, a);
}
// A launch of the call failed: whatever segment partials reached the scratch do not outlive it.
static hipError_t long_done(AeadAlg alg, size_t n, size_t max_len, void* scratch, hipStream_t st) {
  if (launch_status() != hipSuccess) (void)hipMemsetAsync(scratch, 0, aead_long_part_bytes(alg, n, max_len), st);
  return launch_status();
}

hipError_t aead_seal_long(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* nonces, const uint8_t* pt,
                          const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                          size_t max_len, uint8_t* sealed, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (aad_len >= aead::ROW_MAX || max_len == 0 || max_len >= aead::ROW_MAX) return hipErrorInvalidValue;
  aead::LongArgs a = long_args(alg, n, max_len, scratch);
  a.keys = keys, a.nonces = nonces, a.in = pt, a.off = pt_off, a.aad = aad, a.aad_off = aad_off;
  a.aad_len = (uint32_t)aad_len, a.out = sealed;
  if (alg == AeadAlg::AES_256_GCM) {
    launch_seg<aead::GcmLong, aead::SEAL>("k_long_seg_gcm_seal", a, st);
    launch_tail<aead::GcmLong, aead::SEAL>("k_long_tail_gcm_seal", a, st);
  } else {
    launch_seg<aead::ChaLong, aead::SEAL>("k_long_seg_chacha_seal", a, st);
    launch_tail<aead::ChaLong, aead::SEAL>("k_long_tail_chacha_seal", a, st);
  }
  return long_done(alg, n, max_len, scratch, st);
}

hipError_t aead_open_long(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* sealed, const uint64_t* sealed_off,
                          const uint8_t* aad, const uint64_t* aad_off, size_t aad_len, size_t max_len, uint8_t* pt,
                          int32_t* status, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (aad_len >= aead::ROW_MAX || max_len == 0 || max_len >= aead::ROW_MAX) return hipErrorInvalidValue;
  aead::LongArgs a = long_args(alg, n, max_len, scratch);
  a.keys = keys, a.in = sealed, a.off = sealed_off, a.aad = aad, a.aad_off = aad_off;
  a.aad_len = (uint32_t)aad_len, a.out = pt, a.status = status;
  if (alg == AeadAlg::AES_256_GCM) {
    launch_seg<aead::GcmLong, aead::OPEN_MAC>("k_long_seg_gcm_mac", a, st);
    launch_tail<aead::GcmLong, aead::OPEN_MAC>("k_long_tail_gcm_open", a, st);
    launch_seg<aead::GcmLong, aead::OPEN_DEC>("k_long_seg_gcm_decrypt", a, st);
  } else {
    launch_seg<aead::ChaLong, aead::OPEN_MAC>("k_long_seg_chacha_mac", a, st);
    launch_tail<aead::ChaLong, aead::OPEN_MAC>("k_long_tail_chacha_open", a, st);
    launch_seg<aead::ChaLong, aead::OPEN_DEC>("k_long_seg_chacha_decrypt", a, st);
  }
  return long_done(alg, n, max_len, scratch, st);
}

// tests: the segment and tail kernels' MAC machinery under a chosen H (h [n][16]) or key32 = r | s ([n][32])
template <class A>
static hipError_t dbg_mac_long(AeadAlg alg, size_t n, const uint8_t* key, const uint8_t* data, const uint64_t* data_off,
                               size_t max_len, uint8_t* out, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (max_len == 0 || max_len >= aead::ROW_MAX) return hipErrorInvalidValue;
  aead::LongArgs a = long_args(alg, n, max_len, scratch);
  a.keys = key, a.in = data, a.off = data_off, a.out = out;
  launch_seg<A, aead::DBG>("k_long_seg_dbg", a, st);
  launch_tail<A, aead::DBG>("k_long_tail_dbg", a, st);
  return long_done(alg, n, max_len, scratch, st);
}
hipError_t dbg_ghash_long(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, size_t max_len,
                          uint8_t* out, void* scratch, hipStream_t st) {
  return dbg_mac_long<aead::GhashDbg>(AeadAlg::AES_256_GCM, n, h, data, data_off, max_len, out, scratch, st);
}
hipError_t dbg_poly1305_long(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, size_t max_len,
                             uint8_t* tag, void* scratch, hipStream_t st) {
  return dbg_mac_long<aead::PolyDbg>(AeadAlg::CHACHA20_POLY1305, n, key32, msg, msg_off, max_len, tag, scratch, st);
}

}  // namespace qrk
