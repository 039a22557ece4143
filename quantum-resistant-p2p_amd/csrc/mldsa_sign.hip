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
// signature.  (A secret key set, mldsa_keyed.hip, is the third place: K, NTT(s1), NTT(s2) and NTT(t0) of its
// keys stay in its own device allocation until qrk_mldsa_keyset_free zeroes it.)  Every LDS array is zeroed before its workgroup exits.  Inside an iteration of the signing loop no
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

#include "mldsa_cores.cuh"

namespace qrk {
namespace mldsa {

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
  sign_mu_body(row, sk + row * P.sk + 64, 0u, msg, off, ctx, ctx_len, mu, flags);  // tr = H(pk, 64): public
}

// The loop itself is sign_core_body (mldsa_cores.cuh), which the key-set call shares; here the key is the row's own.
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
  const size_t row = blockIdx.x;
  const uint8_t* skr = sk + row * P.sk;
  sign_core_body<PS, TRACE, SIGN_ROW>(row, skr, SignKey{skr + 32, nullptr, nullptr, nullptr, 0u}, rnd,
                                      A + row * P.k * P.l * N, mu + row * 8, flags[row], max_iters,
                                      sig + row * P.sig, status, tr_mu, tr_iters);
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
