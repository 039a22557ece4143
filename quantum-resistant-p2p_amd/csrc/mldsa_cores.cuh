// The kernel bodies that the per-row ML-DSA calls (mldsa.hip, mldsa_sign.hip) and the key-set calls
// (mldsa_keyed.hip) share, as __forceinline__ device functions: each __global__ kernel stays in its own file
// under its own name and supplies where the key material comes from (the row's pk / sk, or a key set expanded
// once); everything after that is one copy here.
//
// The two halves keep their rules.  The verification bodies (front_mu_c, verify_core_body, verify_final_body)
// work on public data and leave early on it.  The signing bodies (sign_mu_body, sk_decode_ntt, sign_core_body)
// follow the header of mldsa_sign.hip: no branch or address depends on secret data inside an iteration, every
// LDS array is zeroed on exit, and nothing of the verification half is used by them.
#pragma once

#include "mldsa_common.cuh"
#include "qrkem_internal.h"

namespace qrk {
namespace mldsa {

constexpr int T0_BYTES = 32 * D;  // one polynomial of t0, 13 bits per coefficient
__host__ __device__ constexpr int eta_of(const Params& P) { return P.beta / P.tau; }
__host__ __device__ constexpr int eta_bits(const Params& P) { return eta_of(P) == 2 ? 3 : 4; }

__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b);
  return v;
}
__device__ __forceinline__ void st64(uint8_t* p, uint64_t v) {
#pragma unroll
  for (int b = 0; b < 8; ++b) p[b] = (uint8_t)(v >> (8 * b));
}
// Field i of 256 fields of `bits` (<= 20) bits packed little-endian at p.  Reads only the bytes that hold
// the field (up to three), so the last field reads nothing past the polynomial.  The address depends on i alone.
__device__ __forceinline__ uint32_t field(const uint8_t* p, int bits, int i) {
  const int bit = i * bits, o = bit >> 3, sh = bit & 7;
  uint32_t v = p[o];
  if (sh + bits > 8) v |= (uint32_t)p[o + 1] << 8;
  if (sh + bits > 16) v |= (uint32_t)p[o + 2] << 16;
  return (v >> sh) & ((1u << bits) - 1);
}
// Byte b of the packing of 256 fields val(i) < 2^bits.  256 bits is a whole number of bytes, so the last
// byte ends with field 255 and no index beyond it is formed.
template <class Val>
__device__ __forceinline__ uint8_t packed_byte(int bits, int b, Val val) {
  const int bit = 8 * b;
  int i = bit / bits, have = bits - (bit - i * bits);  // what field i still has from position `bit` on
  uint32_t x = val(i) >> (bits - have);
  while (have < 8) {
    ++i;
    x |= val(i) << have;
    have += bits;
  }
  return (uint8_t)x;
}

// ================================================================= Verify
// The rest of a front lane once tr is in: s holds tr in words 0 .. 7 of an otherwise empty SHAKE256 block.
// mu = H(tr || 0 || len(ctx) || ctx || M, 64) to mu[row], then c = SampleInBall(c~) into this lane's LDS row
// `c` (256 int8) through this lane's block buffer `blk` (17 words).  ct: the row's signature (c~ first).
template <int PS>
__device__ __forceinline__ void front_mu_c(KState& s, size_t row, const uint8_t* m, uint32_t mlen,
                                           const uint8_t* ctx, uint32_t ctx_len, const uint8_t* ct,
                                           uint64_t* __restrict__ mu, int8_t* c, uint64_t* blk) {
  constexpr Params P = Set<PS>::P;
  absorb_bytes<RW_SHAKE256, 8>(s, 2 + ctx_len + mlen, [&](uint32_t i) -> uint32_t {
    if (i < 2) return i ? ctx_len : 0u;
    i -= 2;
    return i < ctx_len ? ctx[i] : m[i - ctx_len];
  });
#pragma unroll
  for (int w = 0; w < 8; ++w) mu[row * 8 + w] = kword(s, w);
  bool started = false;
  sample_in_ball(P.tau, c, (uint8_t*)blk, [&](uint8_t*) {
    if (!started) {
      kzero(s);
      absorb_bytes<RW_SHAKE256, 0>(s, P.ctilde, [&](uint32_t i) -> uint32_t { return ct[i]; });
      started = true;
    } else {
      keccak_f(s);
    }
#pragma unroll
    for (int w = 0; w < 17; ++w) blk[w] = kword(s, w);
  });
}

// One workgroup of 256 threads, one row that the front did not skip: HintBitUnpack and its checks, BitUnpack of
// z and the norm check, the forward NTTs, A_hat z_hat - c_hat (t1 2^d)_hat, k inverse NTTs, UseHint, w1Encode.
// a: the k l polynomials of the row's A_hat.  Per row (KEYED = false) t1 is unpacked from t1p (pk + 32) and
// transformed here; with a key set t1h holds (t1 2^d)_hat of the row's key, reduced to [0, q).
template <int PS, bool KEYED>
__device__ __forceinline__ void verify_core_body(size_t row, const uint8_t* sg, const uint8_t* t1p,
                                                 const int32_t* __restrict__ t1h, const int32_t* __restrict__ a,
                                                 const int8_t* __restrict__ cpoly, uint8_t* __restrict__ w1,
                                                 uint32_t* __restrict__ flags) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l;
  __shared__ int zc[(L + 1) * N];  // z_hat[0 .. l), c_hat
  __shared__ int tp[N];            // (t1 2^d)_hat of row i, then w'_approx of row i
  __shared__ uint32_t hb[K * 8];   // the hint, one bit per coefficient
  __shared__ uint8_t wv[N];
  __shared__ uint32_t s_flag;
  const int tid = threadIdx.x;
  if (tid < K * 8) hb[tid] = 0;
  if (tid == 0) s_flag = 0;
  __syncthreads();
  if (tid == 0 && !hint_unpack(sg + P.hint_off(), K, P.omega, hb)) s_flag = FLAG_HINT;
  bool over = false;
  for (int e = tid; e < L * N; e += 256) {
    const int z = z_coeff(sg + P.ctilde + (e >> 8) * 32 * P.zbits, P.zbits, P.gamma1, e & 255);
    over |= (z < 0 ? -z : z) >= P.gamma1 - P.beta;
    zc[e] = z;
  }
  zc[L * N + tid] = cpoly[row * N + tid];
  __syncthreads();
  if (s_flag & FLAG_HINT) {  // early exit (public input): w1 is undefined without the hint
    if (tid == 0) flags[row] = FLAG_HINT;
    return;
  }
  if (over) atomicOr(&s_flag, FLAG_NORM);
  ntt_fwd(zc, L + 1, tid, 256);  // |z| <= gamma1, |c| <= 1: outputs below 2^25.1 (2^19 + 8 HALFQ)
  for (int i = 0; i < K; ++i) {
    int t;
    if constexpr (KEYED) {
      t = t1h[i * N + tid];  // in [0, q): the product with c_hat is below 2^48.1
    } else {
      tp[tid] = t1_coeff_2d(t1p + 320 * i, tid);
      ntt_fwd(tp, 1, tid, 256);  // input in [0, q): output below 5 q < 2^25.4
      t = tp[tid];
    }
    // l + 1 products below 2^50.5 (A_hat in [0, q)); the sum is at most 8 HALFQ < 2^25
    int acc = -modmul(zc[L * N + tid], (double)t);
    const int32_t* ai = a + (size_t)i * L * N + tid;
    for (int j = 0; j < L; ++j) acc += modmul(ai[j * N], (double)zc[j * N + tid]);
    tp[tid] = acc;
    ntt_inv(tp, 1, tid, 256);
    const int h = (hb[i * 8 + (tid >> 5)] >> (tid & 31)) & 1;
    wv[tid] = (uint8_t)use_hint<P.gamma2>(h, canon(tp[tid]));
    __syncthreads();
    constexpr int NB = 32 * P.w1bits;
    if (tid < NB) w1[row * P.w1_bytes() + i * NB + tid] = w1_byte(wv, P.w1bits, tid);
    __syncthreads();
  }
  if (tid == 0) flags[row] = s_flag;
}

// One lane per row: c~' = H(mu || w1, lambda / 4), the comparison, status; the only writer of status.  A row
// whose flag word says that no w1 exists (malformed hint, a row skipped by the front) is not hashed.  The trace
// outputs are all set or all NULL.
template <int PS>
__device__ __forceinline__ void verify_final_body(size_t n, const uint8_t* __restrict__ sig,
                                                  const uint64_t* __restrict__ mu, const uint8_t* __restrict__ w1,
                                                  const uint32_t* __restrict__ flags, int32_t* __restrict__ status,
                                                  const MldsaTrace& tr) {
  constexpr Params P = Set<PS>::P;
  constexpr int CW = P.ctilde / 8;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  uint32_t fl = flags[row];
  const bool hashed = !(fl & (FLAG_HINT | FLAG_LONG | FLAG_KEY));
  KState s;
  kzero(s);
  if (hashed) {
#pragma unroll
    for (int w = 0; w < 8; ++w) kxor(s, w, mu[row * 8 + w]);
    const uint8_t* wr = w1 + row * P.w1_bytes();
    absorb_bytes<RW_SHAKE256, 8>(s, P.w1_bytes(), [&](uint32_t i) -> uint32_t { return wr[i]; });
    const uint8_t* ct = sig + row * P.sig;
    bool same = true;
#pragma unroll
    for (int w = 0; w < CW; ++w) {
      uint64_t v = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) v |= (uint64_t)ct[8 * w + b] << (8 * b);
      same &= v == kword(s, w);
    }
    if (!same) fl |= FLAG_HASH;
  }
  status[row] = fl ? -1 : 0;
  if (tr.flags) {
    tr.flags[row] = fl;
    uint64_t* tm = (uint64_t*)tr.mu + row * 8;
    uint64_t* tc = (uint64_t*)tr.ctilde + row * 8;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      tm[w] = hashed ? mu[row * 8 + w] : 0;
      tc[w] = hashed && w < CW ? kword(s, w) : 0;
    }
    for (int b = 0; b < P.w1_bytes(); ++b) tr.w1[row * P.w1_bytes() + b] = hashed ? w1[row * P.w1_bytes() + b] : 0;
  }
}

// ================================================================= Sign
// One lane, one row: mu = H(tr || 0 || len(ctx) || ctx || M, 64) and the row's flag word.  `refuse` is a flag
// the caller already has for the row (0 for none); a row of 2^31 bytes or more, or one whose offsets decrease,
// gets FLAG_LONG.  A flagged row gets mu = 0, and tr is not read for it.  tr = H(pk, 64) is public.
__device__ __forceinline__ void sign_mu_body(size_t row, const uint8_t* tr, uint32_t refuse,
                                             const uint8_t* __restrict__ msg, const uint64_t* __restrict__ off,
                                             const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                             uint64_t* __restrict__ mu, uint32_t* __restrict__ flags) {
  const uint64_t o0 = off[row], o1 = off[row + 1];
  const bool bad = o1 < o0 || o1 - o0 >= (1ull << 31);
  KState s;
  kzero(s);
  if (!bad && !refuse) {
    const uint32_t mlen = (uint32_t)(o1 - o0);
    const uint8_t* m = msg + o0;
#pragma unroll
    for (int w = 0; w < 8; ++w) kxor(s, w, ld64(tr + 8 * w));
    absorb_bytes<RW_SHAKE256, 8>(s, 2 + ctx_len + mlen, [&](uint32_t i) -> uint32_t {
      if (i < 2) return i ? ctx_len : 0u;
      i -= 2;
      return i < ctx_len ? ctx[i] : m[i - ctx_len];
    });
  }
#pragma unroll
  for (int w = 0; w < 8; ++w) mu[row * 8 + w] = kword(s, w);  // zeros for a flagged row
  flags[row] = refuse | (bad ? FLAG_LONG : 0u);
}

// skDecode of s1, s2, t0 (skr: one secret key) into three LDS arrays and their forward NTTs, by the 256 threads
// of a workgroup.  A field above 2 eta is outside [-eta, eta]: every field is looked at, and what was found is
// ORed into *bad (LDS, zeroed by the caller before a barrier) once.  *bad is complete when this returns.
template <int PS>
__device__ __forceinline__ void sk_decode_ntt(const uint8_t* skr, int* s1h, int* s2h, int* t0h, uint32_t* bad, int tid) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l, ETA = eta_of(P), EB = eta_bits(P), SB = 32 * EB;
  {
    uint32_t over = 0;
    for (int e = tid; e < L * N; e += 256) {
      const uint32_t v = field(skr + 128 + (e >> 8) * SB, EB, e & 255);
      over |= (uint32_t)(2 * ETA - (int)v) >> 31;
      s1h[e] = ETA - (int)v;
    }
    for (int e = tid; e < K * N; e += 256) {
      const uint32_t v = field(skr + 128 + (L + (e >> 8)) * SB, EB, e & 255);
      over |= (uint32_t)(2 * ETA - (int)v) >> 31;
      s2h[e] = ETA - (int)v;
      t0h[e] = (1 << (D - 1)) - (int)field(skr + 128 + (L + K) * SB + (e >> 8) * T0_BYTES, D, e & 255);
    }
    atomicOr(bad, over);
  }
  ntt_fwd(s1h, L, tid, 256);  // inputs within 2^12: outputs below 2^25
  ntt_fwd(s2h, K, tid, 256);
  ntt_fwd(t0h, K, tid, 256);
}

// Where the signing core takes its key from.
//   SIGN_ROW  the row's own secret key: skDecode and the 2 k + l forward NTTs run here, K is sk + 32
//   SIGN_LDS  a key set: NTT(s1), NTT(s2), NTT(t0) are copied into LDS once per workgroup
//   SIGN_L2   a key set: they are read from the set in every iteration; (2 k + l) KiB of LDS less
// In both key-set modes the addresses depend on the key index (public) and the thread alone.
enum { SIGN_ROW = 0, SIGN_LDS = 1, SIGN_L2 = 2 };
struct SignKey {
  const uint8_t* K;                // the 32 bytes of K
  const int32_t *s1h, *s2h, *t0h;  // key-set modes: NTT(s1) [l][256], NTT(s2) [k][256], NTT(t0) [k][256]
  uint32_t bad;                    // key-set modes: the key's refusal flag
};

// One workgroup of 256 threads per row, the whole rejection loop inside (FIPS 204 Algorithm 7 from line 7 on).
// a: the k l polynomials of the row's A_hat; mu_row: the row's 8 words of mu; row_flags: the row's flag word
// from the mu kernel.  sg and status of the row are written exactly once, here.  TRACE also stores mu and the
// iterations run.
template <int PS, bool TRACE, int MODE>
__device__ __forceinline__ void sign_core_body(size_t row, const uint8_t* skr, const SignKey& key,
                                               const uint8_t* __restrict__ rnd, const int32_t* __restrict__ A,
                                               const uint64_t* __restrict__ mu_row, uint32_t row_flags,
                                               uint32_t max_iters, uint8_t* __restrict__ sg,
                                               int32_t* __restrict__ status, uint8_t* __restrict__ tr_mu,
                                               uint32_t* __restrict__ tr_iters) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l;
  constexpr int ZB = 32 * P.zbits;            // bytes of one packed polynomial of y or z
  constexpr int YBLK = (ZB + 135) / 136;      // SHAKE256 blocks of one ExpandMask stream
  constexpr int YW = YBLK * RW_SHAKE256;      // ... in words
  constexpr int CW = P.ctilde / 8;
  constexpr int W1B = 32 * P.w1bits;          // bytes of one polynomial of w1Encode
  constexpr bool HELD = MODE != SIGN_L2;      // the NTT'd secret vectors are in LDS
  static_assert(2 * N * (int)sizeof(int) <= L * YW * 8, "the two-polynomial scratch fits the mask bytes");
  // LDS: (3 k + 2 l + 1) KiB of coefficients ((k + l + 1) KiB in SIGN_L2), the mask bytes, 2 k 128 bytes of high
  // bits, under 1 KiB of small buffers: 26064 / 35488 / 47696 bytes for ML-DSA-44 / 65 / 87 with them held.
  __shared__ int s1h[HELD ? L * N : 1], s2h[HELD ? K * N : 1], t0h[HELD ? K * N : 1];  // NTT(s1), NTT(s2), NTT(t0)
  __shared__ int y[L * N];                            // y_hat, then c s1, then z
  __shared__ int w[K * N];                            // A_hat y_hat, then w
  __shared__ int ch[N];                               // c_hat
  __shared__ uint64_t yb[L * YW];  // the ExpandMask streams; once z is formed, two polynomials of scratch
  __shared__ uint8_t wv[K * N];    // HighBits(w)
  __shared__ int8_t cs[N];         // c
  __shared__ uint64_t sb[RW_SHAKE256], rho2[8], mus[8], ctl[8];  // SampleInBall's block, rho'', mu, c~
  __shared__ uint32_t hb[K * 8];   // the hint, one bit per coefficient
  __shared__ uint8_t hbytes[P.omega + K];
  __shared__ uint32_t s_bad, s_rej, s_hcnt;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = 0;
  if (tid < 8) mus[tid] = mu_row[tid];
  __syncthreads();
  if constexpr (MODE == SIGN_ROW) {
    sk_decode_ntt<PS>(skr, s1h, s2h, t0h, &s_bad, tid);
  } else if constexpr (MODE == SIGN_LDS) {
    for (int e = tid; e < L * N; e += 256) s1h[e] = key.s1h[e];
    for (int e = tid; e < K * N; e += 256) s2h[e] = key.s2h[e], t0h[e] = key.t0h[e];
    __syncthreads();
  }
  auto s1_at = [&](int e) -> int { if constexpr (HELD) return s1h[e]; else return key.s1h[e]; };
  auto s2_at = [&](int e) -> int { if constexpr (HELD) return s2h[e]; else return key.s2h[e]; };
  auto t0_at = [&](int e) -> int { if constexpr (HELD) return t0h[e]; else return key.t0h[e]; };
  // the same for the whole workgroup
  const bool refused = (MODE == SIGN_ROW ? s_bad != 0 : key.bad != 0) || row_flags != 0;
  uint32_t iters = 0;
  bool done = false;
  if (!refused) {
    if (tid == 0) {  // rho'' = H(K || rnd || mu, 64): 128 bytes, one block
      KState s;
      kzero(s);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        kxor(s, x, ld64(key.K + 8 * x));
        kxor(s, 4 + x, rnd ? ld64(rnd + row * 32 + 8 * x) : 0ull);
      }
#pragma unroll
      for (int x = 0; x < 8; ++x) kxor(s, 8 + x, mus[x]);
      s.a[16].lo ^= DS_SHAKE;
      s.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
      keccak_f(s);
#pragma unroll
      for (int x = 0; x < 8; ++x) rho2[x] = kword(s, x);
    }
    for (uint32_t it = 0; it < max_iters; ++it) {
      if (tid == 0) s_rej = 0, s_hcnt = 0;
      __syncthreads();
      // ExpandMask (Algorithm 34): lane r squeezes H(rho'' || kappa + r as two bytes, 32 zbits bytes)
      if (tid < L) {
        KState s;
        kzero(s);
#pragma unroll
        for (int x = 0; x < 8; ++x) kxor(s, x, rho2[x]);
        s.a[8].lo ^= (it * L + (uint32_t)tid) | (DS_SHAKE << 16);  // kappa + r <= 814 * 7 + 6 < 2^16
        s.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
        for (int blk = 0; blk < YBLK; ++blk) {
          keccak_f(s);
#pragma unroll
          for (int x = 0; x < RW_SHAKE256; ++x) yb[tid * YW + blk * RW_SHAKE256 + x] = kword(s, x);
        }
      }
      __syncthreads();
      for (int e = tid; e < L * N; e += 256)
        y[e] = P.gamma1 - (int)field((const uint8_t*)(yb + (e >> 8) * YW), P.zbits, e & 255);
      ntt_fwd(y, L, tid, 256);  // |y| <= gamma1: outputs below 2^25.1
      // w = INTT(A_hat y_hat): l products below 2^48.1 per coefficient, the sum at most 7 HALFQ
      const int32_t* a = A + tid;
      for (int i = 0; i < K; ++i) {
        int acc = 0;
        for (int j = 0; j < L; ++j) acc += modmul(a[(i * L + j) * N], (double)y[j * N + tid]);
        w[i * N + tid] = acc;
      }
      ntt_inv(w, K, tid, 256);
      for (int i = 0; i < K; ++i) {
        int r1, r0;
        decompose<P.gamma2>(canon(w[i * N + tid]), r1, r0);
        wv[i * N + tid] = (uint8_t)r1;
      }
      __syncthreads();
      // c~ = H(mu || w1Encode(w1), lambda / 4) and c = SampleInBall(c~): one sponge after the other on lane 0
      if (tid == 0) {
        KState s;
        kzero(s);
#pragma unroll
        for (int x = 0; x < 8; ++x) kxor(s, x, mus[x]);
        absorb_bytes<RW_SHAKE256, 8>(s, P.w1_bytes(), [&](uint32_t i) -> uint32_t {
          return w1_byte(wv + (i / W1B) * N, P.w1bits, i % W1B);
        });
#pragma unroll
        for (int x = 0; x < 8; ++x) ctl[x] = x < CW ? kword(s, x) : 0ull;
        kzero(s);
#pragma unroll
        for (int x = 0; x < CW; ++x) kxor(s, x, ctl[x]);
        s.a[CW].lo ^= DS_SHAKE;
        s.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
        sample_in_ball(P.tau, cs, (uint8_t*)sb, [&](uint8_t*) {
          keccak_f(s);
#pragma unroll
          for (int x = 0; x < RW_SHAKE256; ++x) sb[x] = kword(s, x);
        });
      }
      __syncthreads();
      ch[tid] = cs[tid];
      ntt_fwd(ch, 1, tid, 256);  // outputs below 2^25
      // z = y + c s1 (products below 2^50.1); c s1 is exact and within beta for a key that was not refused
      for (int e = tid; e < L * N; e += 256) y[e] = modmul(s1_at(e), (double)ch[e & 255]);
      ntt_inv(y, L, tid, 256);
      uint32_t rej = 0;
      for (int e = tid; e < L * N; e += 256) {
        const int z = P.gamma1 - (int)field((const uint8_t*)(yb + (e >> 8) * YW), P.zbits, e & 255) + y[e];
        rej |= (uint32_t)(P.gamma1 - P.beta - 1 - (z < 0 ? -z : z)) >> 31;  // bit 0: ||z|| >= gamma1 - beta
        y[e] = z;
      }
      __syncthreads();  // the mask bytes are dead: yb is scratch from here
      // Row by row of the rest: r = w - c s2 and its low bits, c t0, the hint.  All of it runs in every
      // iteration, whatever the checks before it found.
      int* tmp = (int*)yb;
      uint32_t hcnt = 0;
      for (int i = 0; i < K; ++i) {
        tmp[tid] = modmul(s2_at(i * N + tid), (double)ch[tid]);
        tmp[N + tid] = modmul(t0_at(i * N + tid), (double)ch[tid]);
        ntt_inv(tmp, 2, tid, 256);
        const int r = w[i * N + tid] - tmp[tid], ct0 = tmp[N + tid];  // |r| <= 2 HALFQ; c t0 exact, <= tau 2^12
        int r1, r0, v1, v0;
        decompose<P.gamma2>(canon(r), r1, r0);
        rej |= ((uint32_t)(P.gamma2 - P.beta - 1 - (r0 < 0 ? -r0 : r0)) >> 31) << 1;  // bit 1: LowBits
        rej |= ((uint32_t)(P.gamma2 - 1 - (ct0 < 0 ? -ct0 : ct0)) >> 31) << 2;        // bit 2: ||c t0|| >= gamma2
        decompose<P.gamma2>(canon(r + ct0), v1, v0);                                  // MakeHint(-c t0, r + c t0)
        const unsigned long long bal = __ballot(v1 != r1);
        if ((tid & 63) == 0) {
          hb[i * 8 + (tid >> 6) * 2] = (uint32_t)bal;
          hb[i * 8 + (tid >> 6) * 2 + 1] = (uint32_t)(bal >> 32);
          hcnt += (uint32_t)__popcll(bal);
        }
      }
      atomicOr(&s_rej, rej);
      if ((tid & 63) == 0) atomicAdd(&s_hcnt, hcnt);
      __syncthreads();
      const bool reject = s_rej != 0 || s_hcnt > (uint32_t)P.omega;  // decided once, for the whole workgroup
      iters = it + 1;
      __syncthreads();  // every thread has read the two words before lane 0 clears them again
      if (!reject) {
        done = true;
        break;
      }
    }
  }
  if (done) {  // sigEncode: everything stored from here on is the signature, public
    if (tid < P.omega + K) hbytes[tid] = 0;
    __syncthreads();
    if (tid == 0) {
      int index = 0;
      for (int i = 0; i < K; ++i) {
        for (int x = 0; x < 8; ++x)
          for (uint32_t m = hb[i * 8 + x]; m; m &= m - 1) hbytes[index++] = (uint8_t)(32 * x + __builtin_ctz(m));
        hbytes[P.omega + i] = (uint8_t)index;  // index <= omega: the weight check passed
      }
    }
    __syncthreads();
    for (int b = tid; b < P.ctilde; b += 256) sg[b] = ((const uint8_t*)ctl)[b];
    for (int b = tid; b < L * ZB; b += 256) {
      const int* z = y + (b / ZB) * N;
      sg[P.ctilde + b] = packed_byte(P.zbits, b % ZB, [&](int i) -> uint32_t { return (uint32_t)(P.gamma1 - z[i]); });
    }
    if (tid < P.omega + K) sg[P.hint_off() + tid] = hbytes[tid];
  } else {
    for (int b = tid; b < P.sig; b += 256) sg[b] = 0;
  }
  if (tid == 0) status[row] = done ? 0 : -1;
  if constexpr (TRACE) {
    if (tid == 0) tr_iters[row] = iters;
    if (tid < 64) tr_mu[row * 64 + tid] = ((const uint8_t*)mus)[tid];
  }
  __syncthreads();
  if constexpr (HELD) {
    for (int e = tid; e < L * N; e += 256) s1h[e] = 0;
    for (int e = tid; e < K * N; e += 256) s2h[e] = 0, t0h[e] = 0;
  }
  for (int e = tid; e < L * N; e += 256) y[e] = 0;
  for (int e = tid; e < K * N; e += 256) w[e] = 0, wv[e] = 0;
  for (int e = tid; e < L * YW; e += 256) yb[e] = 0;
  ch[tid] = 0, cs[tid] = 0;
  if (tid < RW_SHAKE256) sb[tid] = 0;
  if (tid < 8) rho2[tid] = 0, ctl[tid] = 0;
  if (tid < K * 8) hb[tid] = 0;
}

}  // namespace mldsa
}  // namespace qrk
