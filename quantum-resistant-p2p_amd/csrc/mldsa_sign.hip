// Batched ML-DSA.KeyGen and ML-DSA.Sign (FIPS 204, "pure" ML-DSA: Algorithm 6, Algorithm 2 over Algorithm 7)
// for gfx950: the other half of the reference's MLDSASignature (crypto/signatures.py generate_keypair / sign,
// called on every key-exchange and chat message, messaging.py:620, 864, 1090).
//
// KeyGen, four stream-ordered launches per chunk:
//   k_mldsa_kg_seed    one lane per row: (rho, rho', K) = H(xi || k || l, 128); rho to pk and sk, K to sk
//   k_mldsa_kg_expand  one lane per polynomial of A_hat = ExpandA(rho) (mldsa_common.cuh), rho read from pk
//   k_mldsa_kg_core    one workgroup of 256 threads per row: ExpandS (lanes 0 .. k + l - 1 recompute rho' from xi
//                      and run one SHAKE256 stream each), t = INTT(A_hat NTT(s1)) + s2, Power2Round, the packing
//                      of t1 into pk and of s1, s2, t0 into sk
//   k_mldsa_kg_tr      one lane per row: tr = H(pk, 64) into sk
// Sign, three:
//   k_mldsa_sign_expand  as above, rho read from sk
//   k_mldsa_sign_mu      one lane per row: mu = H(tr || 0 || len(ctx) || ctx || M, 64); a row of 2^31 bytes or
//                        more, or one whose offsets decrease, is flagged and gets mu = 0
//   k_mldsa_sign_core    one workgroup of 256 threads per row, the whole rejection loop inside: see below
//
// Scratch of a chunk (mldsa_sign_scratch_bytes): A_hat (k l KiB) + mu (64 bytes) + a flag word per row, that is
// 16452 / 30788 / 57412 bytes for ML-DSA-44 / 65 / 87.  All three are public.
//
// Secret handling.  xi, rho', K, rho'', s1, s2, t0, y and everything computed from them live in registers and LDS
// only; the only global stores of secret-derived bytes are the `sk` rows KeyGen writes and the accepted
// signature.  Every LDS array is zeroed before its workgroup exits.  Inside an iteration of the signing loop no
// branch and no address depends on s1, s2, t0, y, K or rho'': the norm and weight checks OR / add over all
// coefficients into one LDS word and the workgroup decides once, after the last of them.  What does depend on
// secret data is what the standard itself has: the accept / reject decision per iteration (so the iteration
// count), the rejection sampling of ExpandS in KeyGen, and SampleInBall, whose stream c~ is public for the
// accepted iteration (it is the first field of the signature) and a hash output for a rejected one.  modmul runs
// in fp64 without branches.  Unlike mldsa.hip nothing here leaves early on data.
//
// The loop is counted: it < max_iters, 814 in production (the floor of FIPS 204 Appendix C).  A row that uses
// them all gets status -1 and an all-zero signature, like a refused row (flagged by k_mldsa_sign_mu, or a
// secret key with an s1 / s2 field outside [-eta, eta], which is accumulated into a flag over all fields).
// sig and status of every row are written exactly once, by the core kernel.
#include <cstring>

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

// ================================================================= KeyGen
// (rho, rho', K) = H(xi || k || l, 128): on return s holds the 136-byte output block, rho in words 0..3,
// rho' in 4..11, K in 12..15.
template <int PS>
__device__ __forceinline__ void kg_seed(KState& s, const uint8_t* xi) {
  constexpr Params P = Set<PS>::P;
  kzero(s);
#pragma unroll
  for (int w = 0; w < 4; ++w) kxor(s, w, ld64(xi + 8 * w));
  s.a[4].lo ^= (uint32_t)P.k | ((uint32_t)P.l << 8) | (DS_SHAKE << 16);
  s.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
  keccak_f(s);
}

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_kg_seed(size_t n, const uint8_t* __restrict__ xi,
                                                      uint8_t* __restrict__ pk, uint8_t* __restrict__ sk) {
  constexpr Params P = Set<PS>::P;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  KState s;
  kg_seed<PS>(s, xi + row * 32);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    st64(pk + row * P.pk + 8 * w, kword(s, w));
    st64(sk + row * P.sk + 8 * w, kword(s, w));
    st64(sk + row * P.sk + 32 + 8 * w, kword(s, 12 + w));
  }
}

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_kg_expand(size_t n, const uint8_t* __restrict__ pk,
                                                        int32_t* __restrict__ A) {
  __shared__ int tile[64 * EXPAND_STRIDE];
  expand_a_block<PS>(n, pk, Set<PS>::P.pk, A, tile);
}

template <int PS>
__global__ __launch_bounds__(256) void k_mldsa_kg_core(const uint8_t* __restrict__ xi, const int32_t* __restrict__ A,
                                                       uint8_t* __restrict__ pk, uint8_t* __restrict__ sk) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l, ETA = eta_of(P), EB = eta_bits(P), SB = 32 * EB;
  __shared__ int8_t se[(L + K) * N];  // s1[0 .. l), s2[0 .. k)
  __shared__ int s1h[L * N];
  __shared__ int tp[N];
  __shared__ uint16_t t1v[N], t0v[N];  // t1 and 2^12 - t0 of the current row of t
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  uint8_t* pkr = pk + row * P.pk;
  uint8_t* skr = sk + row * P.sk;
  // ExpandS (Algorithms 33, 31): polynomial tid from SHAKE256(rho' || tid as two bytes).  The number of blocks
  // and the position a coefficient lands at depend on the rejections: that is the standard's sampler.
  if (tid < L + K) {
    KState s;
    kg_seed<PS>(s, xi + row * 32);
    KState t;
    kzero(t);
#pragma unroll
    for (int w = 0; w < 8; ++w) kxor(t, w, kword(s, 4 + w));
    t.a[8].lo ^= (uint32_t)tid | (DS_SHAKE << 16);
    t.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
    int cnt = 0;
    while (cnt < N) {
      keccak_f(t);
#pragma unroll
      for (int w = 0; w < RW_SHAKE256; ++w) {
        const uint64_t v = kword(t, w);
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          const int nib = (int)(v >> (4 * b)) & 15;
          const bool ok = (ETA == 2 ? nib < 15 : nib < 9) && cnt < N;
          if (ok) se[tid * N + cnt++] = (int8_t)(ETA == 2 ? 2 - nib % 5 : 4 - nib);
        }
      }
    }
  }
  __syncthreads();
  for (int b = tid; b < (L + K) * SB; b += 256) {
    const int8_t* s = se + (b / SB) * N;
    skr[128 + b] = packed_byte(EB, b % SB, [&](int i) -> uint32_t { return (uint32_t)(ETA - s[i]); });
  }
  for (int e = tid; e < L * N; e += 256) s1h[e] = se[e];
  ntt_fwd(s1h, L, tid, 256);  // |s1| <= eta: outputs below 2^25
  const int32_t* a = A + row * K * L * N + tid;
  for (int i = 0; i < K; ++i) {
    int acc = 0;  // l products below 2^48; the sum is at most 7 HALFQ
    for (int j = 0; j < L; ++j) acc += modmul(a[(i * L + j) * N], (double)s1h[j * N + tid]);
    tp[tid] = acc;
    ntt_inv(tp, 1, tid, 256);
    const int t = canon(tp[tid] + se[(L + i) * N + tid]);
    int r0 = t & ((1 << D) - 1);  // Power2Round: r0 in (-2^12, 2^12]
    r0 -= (((1 << (D - 1)) - r0) >> 31) & (1 << D);
    t1v[tid] = (uint16_t)((t - r0) >> D);
    t0v[tid] = (uint16_t)((1 << (D - 1)) - r0);
    __syncthreads();
    for (int b = tid; b < 320; b += 256)
      pkr[32 + 320 * i + b] = packed_byte(10, b, [&](int c) -> uint32_t { return t1v[c]; });
    for (int b = tid; b < T0_BYTES; b += 256)
      skr[128 + (L + K) * SB + T0_BYTES * i + b] = packed_byte(D, b, [&](int c) -> uint32_t { return t0v[c]; });
    __syncthreads();
  }
  for (int e = tid; e < (L + K) * N; e += 256) se[e] = 0;
  for (int e = tid; e < L * N; e += 256) s1h[e] = 0;
  tp[tid] = 0, t1v[tid] = 0, t0v[tid] = 0;
}

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_kg_tr(size_t n, const uint8_t* __restrict__ pk,
                                                    uint8_t* __restrict__ sk) {
  constexpr Params P = Set<PS>::P;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  const uint8_t* pkr = pk + row * P.pk;
  KState s;
  kzero(s);
  absorb_bytes<RW_SHAKE256, 0>(s, P.pk, [&](uint32_t i) -> uint32_t { return pkr[i]; });
#pragma unroll
  for (int w = 0; w < 8; ++w) st64(sk + row * P.sk + 64 + 8 * w, kword(s, w));
}

// ================================================================= Sign
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_sign_expand(size_t n, const uint8_t* __restrict__ sk,
                                                          int32_t* __restrict__ A) {
  __shared__ int tile[64 * EXPAND_STRIDE];
  expand_a_block<PS>(n, sk, Set<PS>::P.sk, A, tile);  // rho: the first 32 bytes of a secret key, public
}

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_sign_mu(size_t n, const uint8_t* __restrict__ sk,
                                                      const uint8_t* __restrict__ msg,
                                                      const uint64_t* __restrict__ off,
                                                      const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                                      uint64_t* __restrict__ mu, uint32_t* __restrict__ flags) {
  constexpr Params P = Set<PS>::P;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  const uint64_t o0 = off[row], o1 = off[row + 1];
  const bool bad = o1 < o0 || o1 - o0 >= (1ull << 31);
  KState s;
  kzero(s);
  if (!bad) {
    const uint32_t mlen = (uint32_t)(o1 - o0);
    const uint8_t* tr = sk + row * P.sk + 64;  // tr = H(pk, 64): public
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
  flags[row] = bad ? FLAG_LONG : 0u;
}

// TRACE (tests: qrk_dbg_mldsa_sign_trace) also stores mu and the iterations run; no other call launches that
// instantiation.
template <int PS, bool TRACE>
__global__ __launch_bounds__(256) void k_mldsa_sign_core(const uint8_t* __restrict__ sk,
                                                         const uint8_t* __restrict__ rnd,
                                                         const int32_t* __restrict__ A,
                                                         const uint64_t* __restrict__ mu,
                                                         const uint32_t* __restrict__ flags, uint32_t max_iters,
                                                         uint8_t* __restrict__ sig, int32_t* __restrict__ status,
                                                         uint8_t* __restrict__ tr_mu, uint32_t* __restrict__ tr_iters) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l, ETA = eta_of(P), EB = eta_bits(P), SB = 32 * EB;
  constexpr int ZB = 32 * P.zbits;            // bytes of one packed polynomial of y or z
  constexpr int YBLK = (ZB + 135) / 136;      // SHAKE256 blocks of one ExpandMask stream
  constexpr int YW = YBLK * RW_SHAKE256;      // ... in words
  constexpr int CW = P.ctilde / 8;
  constexpr int W1B = 32 * P.w1bits;          // bytes of one polynomial of w1Encode
  static_assert(2 * N * (int)sizeof(int) <= L * YW * 8, "the two-polynomial scratch fits the mask bytes");
  // LDS: (3 k + 2 l + 1) KiB of coefficients, the mask bytes, 2 k 128 bytes of high bits, under 1 KiB of
  // small buffers: 26064 / 35488 / 47696 bytes for ML-DSA-44 / 65 / 87.
  __shared__ int s1h[L * N], s2h[K * N], t0h[K * N];  // NTT(s1), NTT(s2), NTT(t0)
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
  const size_t row = blockIdx.x;
  const uint8_t* skr = sk + row * P.sk;
  uint8_t* sg = sig + row * P.sig;
  if (tid == 0) s_bad = 0;
  if (tid < 8) mus[tid] = mu[row * 8 + tid];
  __syncthreads();
  // skDecode; a field above 2 eta is outside [-eta, eta]: every field is looked at, the flag is set once
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
    atomicOr(&s_bad, over);
  }
  ntt_fwd(s1h, L, tid, 256);  // inputs within 2^12: outputs below 2^25
  ntt_fwd(s2h, K, tid, 256);
  ntt_fwd(t0h, K, tid, 256);
  const bool refused = s_bad != 0 || flags[row] != 0;  // the same for the whole workgroup
  uint32_t iters = 0;
  bool done = false;
  if (!refused) {
    if (tid == 0) {  // rho'' = H(K || rnd || mu, 64): 128 bytes, one block
      KState s;
      kzero(s);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        kxor(s, x, ld64(skr + 32 + 8 * x));
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
      const int32_t* a = A + row * K * L * N + tid;
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
      for (int e = tid; e < L * N; e += 256) y[e] = modmul(s1h[e], (double)ch[e & 255]);
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
        tmp[tid] = modmul(s2h[i * N + tid], (double)ch[tid]);
        tmp[N + tid] = modmul(t0h[i * N + tid], (double)ch[tid]);
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
  for (int e = tid; e < L * N; e += 256) s1h[e] = 0, y[e] = 0;
  for (int e = tid; e < K * N; e += 256) s2h[e] = 0, t0h[e] = 0, w[e] = 0, wv[e] = 0;
  for (int e = tid; e < L * YW; e += 256) yb[e] = 0;
  ch[tid] = 0, cs[tid] = 0;
  if (tid < RW_SHAKE256) sb[tid] = 0;
  if (tid < 8) rho2[tid] = 0, ctl[tid] = 0;
  if (tid < K * 8) hb[tid] = 0;
}

// scratch of a chunk of C rows: A_hat | mu | flags
struct SignLayout {
  int32_t* A;
  uint64_t* mu;
  uint32_t* flags;
  size_t bytes;
};
static SignLayout sign_layout(const Params& P, size_t C, void* scratch) {
  uint8_t* p = (uint8_t*)scratch;
  SignLayout l;
  size_t o = 0;
  l.A = (int32_t*)(p + o), o += C * P.k * P.l * N * sizeof(int32_t);
  l.mu = (uint64_t*)(p + o), o += C * 64;
  l.flags = (uint32_t*)(p + o), o += C * sizeof(uint32_t);
  l.bytes = o;
  return l;
}

template <int PS>
static hipError_t run_keypair(size_t n, const uint8_t* xi, uint8_t* pk, uint8_t* sk, void* scratch, hipStream_t st) {
  constexpr Params P = Set<PS>::P;
  const SignLayout l = sign_layout(P, n, scratch);
  const dim3 lanes((unsigned)((n + 63) / 64)), polys((unsigned)((n * P.k * P.l + 63) / 64));
  QRK_LAUNCH("k_mldsa_kg_seed", st, k_mldsa_kg_seed<PS>, lanes, dim3(64), 0, st, n, xi, pk, sk);
  QRK_LAUNCH("k_mldsa_kg_expand", st, k_mldsa_kg_expand<PS>, polys, dim3(64), 0, st, n, (const uint8_t*)pk, l.A);
  QRK_LAUNCH("k_mldsa_kg_core", st, k_mldsa_kg_core<PS>, dim3((unsigned)n), dim3(256), 0, st, xi, (const int32_t*)l.A,
             pk, sk);
  QRK_LAUNCH("k_mldsa_kg_tr", st, k_mldsa_kg_tr<PS>, lanes, dim3(64), 0, st, n, (const uint8_t*)pk, sk);
  return launch_status();
}

template <int PS>
static hipError_t run_sign(size_t n, const uint8_t* sk, const uint8_t* msg, const uint64_t* off, const uint8_t* rnd,
                           const uint8_t* ctx, size_t ctx_len, uint8_t* sig, int32_t* status, uint32_t max_iters,
                           uint8_t* tr_mu, uint32_t* tr_iters, void* scratch, hipStream_t st) {
  constexpr Params P = Set<PS>::P;
  const SignLayout l = sign_layout(P, n, scratch);
  const dim3 lanes((unsigned)((n + 63) / 64)), polys((unsigned)((n * P.k * P.l + 63) / 64));
  QRK_LAUNCH("k_mldsa_sign_expand", st, k_mldsa_sign_expand<PS>, polys, dim3(64), 0, st, n, sk, l.A);
  QRK_LAUNCH("k_mldsa_sign_mu", st, k_mldsa_sign_mu<PS>, lanes, dim3(64), 0, st, n, sk, msg, off, ctx,
             (uint32_t)ctx_len, l.mu, l.flags);
  if (tr_iters)
    QRK_LAUNCH("k_mldsa_sign_core", st, (k_mldsa_sign_core<PS, true>), dim3((unsigned)n), dim3(256), 0, st, sk, rnd,
               (const int32_t*)l.A, (const uint64_t*)l.mu, (const uint32_t*)l.flags, max_iters, sig, status, tr_mu,
               tr_iters);
  else
    QRK_LAUNCH("k_mldsa_sign_core", st, (k_mldsa_sign_core<PS, false>), dim3((unsigned)n), dim3(256), 0, st, sk, rnd,
               (const int32_t*)l.A, (const uint64_t*)l.mu, (const uint32_t*)l.flags, max_iters, sig, status, tr_mu,
               tr_iters);
  return launch_status();
}

static const Params& sign_params_of(int which) { return which == 0 ? P44 : which == 1 ? P65 : P87; }

}  // namespace mldsa

size_t mldsa_sign_scratch_bytes(int which, size_t chunk) {
  return mldsa::sign_layout(mldsa::sign_params_of(which), chunk, nullptr).bytes;
}

hipError_t mldsa_keypair(int which, size_t n, const uint8_t* xi, uint8_t* pk, uint8_t* sk, void* scratch,
                         hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > (1u << 24)) return hipErrorInvalidValue;  // grids of n and n k l / 64 workgroups
  return with_which<3>(which, [&](auto ps) {
    return mldsa::run_keypair<decltype(ps)::value>(n, xi, pk, sk, scratch, st);
  });
}

hipError_t mldsa_sign(int which, size_t n, const uint8_t* sk, const uint8_t* msg, const uint64_t* msg_off,
                      const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len, uint8_t* sig, int32_t* status,
                      uint32_t max_iters, uint8_t* trace_mu, uint32_t* trace_iters, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || n > (1u << 24)) return hipErrorInvalidValue;
  return with_which<3>(which, [&](auto ps) {
    return mldsa::run_sign<decltype(ps)::value>(n, sk, msg, msg_off, rnd, ctx_str, ctx_len, sig, status, max_iters,
                                                trace_mu, trace_iters, scratch, st);
  });
}

}  // namespace qrk
