// Batched ML-DSA.Verify (FIPS 204, "pure" ML-DSA: Algorithm 3 over Algorithm 8) for gfx950.
//
// The receiving side of the reference verifies every handshake message
// (quantum_resistant_p2p/app/messaging.py:721, 933, 1174, 1480 through crypto/signatures.py:167); this
// is that step over n rows at once.  Four stream-ordered launches per chunk, no cross-workgroup waits:
//
//   k_mldsa_front   one lane per row: tr = H(pk, 64), mu = H(tr || 0 || len(ctx) || ctx || M, 64),
//                   c = SampleInBall(c~); a row of 2^31 bytes or more is flagged and skipped
//   k_mldsa_expand  one lane per polynomial of A_hat = ExpandA(rho): five SHAKE128 blocks (a general
//                   loop), coefficients staged per block in LDS so that the global stores are
//                   contiguous runs; k l KiB per row in the context's scratch
//   k_mldsa_core    one workgroup of 256 threads per row: HintBitUnpack and its checks, BitUnpack of z
//                   and the norm check, the l + 1 + k forward NTTs, A_hat z_hat - c_hat (t1 2^d)_hat,
//                   k inverse NTTs, UseHint, w1Encode
//   k_mldsa_final   one lane per row: c~' = H(mu || w1, lambda / 4), the comparison, status
//
// A row's flag word collects what failed (mldsa_arith.cuh FLAG_*); k_mldsa_final is the only writer
// of status and writes every row exactly once: 0 when the flag word is 0, else -1.  Every input of
// verification is public, so the kernels branch on data and leave early (a malformed hint ends the
// core kernel's workgroup at once).  Nothing here may be copied into a signing path.
#include <cstring>

#include "mldsa_common.cuh"
#include "qrkem_internal.h"

namespace qrk {
namespace mldsa {

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_front(size_t n, const uint8_t* __restrict__ pk,
                                                    const uint8_t* __restrict__ msg,
                                                    const uint64_t* __restrict__ off,
                                                    const uint8_t* __restrict__ sig,
                                                    const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                                    uint64_t* __restrict__ mu, uint32_t* __restrict__ cpoly,
                                                    uint32_t* __restrict__ flags) {
  constexpr Params P = Set<PS>::P;
  __shared__ uint32_t cs[64][64];  // c of each lane's row, 256 int8
  __shared__ uint64_t sb[64][17];  // each lane's current SHAKE256 output block
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * 64, row = base + lane;
  if (row < n) {
    const uint64_t o0 = off[row], o1 = off[row + 1];
    uint32_t fl = 0;
    if (o1 < o0 || o1 - o0 >= (1ull << 31)) {
      fl = FLAG_LONG;
    } else {
      const uint32_t mlen = (uint32_t)(o1 - o0);
      const uint8_t* pkr = pk + row * P.pk;
      const uint8_t* m = msg + o0;
      KState s;
      kzero(s);
      absorb_bytes<RW_SHAKE256, 0>(s, P.pk, [&](uint32_t i) -> uint32_t { return pkr[i]; });
      // mu: the 64 bytes of tr are the first 8 words of the next sponge's first block
#pragma unroll
      for (int w = 8; w < 25; ++w) s.a[w] = {0u, 0u};
      absorb_bytes<RW_SHAKE256, 8>(s, 2 + ctx_len + mlen, [&](uint32_t i) -> uint32_t {
        if (i < 2) return i ? ctx_len : 0u;
        i -= 2;
        return i < ctx_len ? ctx[i] : m[i - ctx_len];
      });
#pragma unroll
      for (int w = 0; w < 8; ++w) mu[row * 8 + w] = kword(s, w);
      // c = SampleInBall(c~)
      const uint8_t* ct = sig + row * P.sig;
      bool started = false;
      sample_in_ball(P.tau, (int8_t*)cs[lane], (uint8_t*)sb[lane], [&](uint8_t*) {
        if (!started) {
          kzero(s);
          absorb_bytes<RW_SHAKE256, 0>(s, P.ctilde, [&](uint32_t i) -> uint32_t { return ct[i]; });
          started = true;
        } else {
          keccak_f(s);
        }
#pragma unroll
        for (int w = 0; w < 17; ++w) sb[lane][w] = kword(s, w);
      });
    }
    flags[row] = fl;
  }
  __syncthreads();
  for (int r = 0; r < 64 && base + r < n; ++r) cpoly[(base + r) * 64 + lane] = cs[r][lane];
}

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_expand(size_t n, const uint8_t* __restrict__ pk,
                                                     int32_t* __restrict__ A) {
  __shared__ int tile[64 * EXPAND_STRIDE];
  expand_a_block<PS>(n, pk, Set<PS>::P.pk, A, tile);  // rho: the first 32 bytes of a public key
}

template <int PS>
__global__ __launch_bounds__(256) void k_mldsa_core(const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
                                                    const int32_t* __restrict__ A,
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
  const size_t row = blockIdx.x;
  if (flags[row] & FLAG_LONG) return;  // the whole workgroup: k_mldsa_front wrote nothing else for it
  const uint8_t* sg = sig + row * P.sig;
  const uint8_t* pkr = pk + row * P.pk;
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
    tp[tid] = t1_coeff_2d(pkr + 32 + 320 * i, tid);
    ntt_fwd(tp, 1, tid, 256);  // input in [0, q): output below 5 q < 2^25.4
    // l + 1 products below 2^50.5 (A_hat in [0, q)); the sum is at most 8 HALFQ < 2^25
    int acc = -modmul(zc[L * N + tid], (double)tp[tid]);
    const int32_t* a = A + (row * K * L + (size_t)i * L) * N + tid;
    for (int j = 0; j < L; ++j) acc += modmul(a[j * N], (double)zc[j * N + tid]);
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

// The trace outputs (tests: qrk_dbg_mldsa_verify_trace) are all set or all NULL.
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_final(size_t n, const uint8_t* __restrict__ sig,
                                                    const uint64_t* __restrict__ mu, const uint8_t* __restrict__ w1,
                                                    const uint32_t* __restrict__ flags, int32_t* __restrict__ status,
                                                    MldsaTrace tr) {
  constexpr Params P = Set<PS>::P;
  constexpr int CW = P.ctilde / 8;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  uint32_t fl = flags[row];
  const bool hashed = !(fl & (FLAG_HINT | FLAG_LONG));
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

// scratch of a chunk of C rows: A_hat | mu | w1 | c | flags (every part a multiple of 8 bytes per row
// but the last)
struct Layout {
  int32_t* A;
  uint64_t* mu;
  uint8_t* w1;
  uint32_t* c;
  uint32_t* flags;
  size_t bytes;
};
static Layout layout(const Params& P, size_t C, void* scratch) {
  uint8_t* p = (uint8_t*)scratch;
  Layout l;
  size_t o = 0;
  l.A = (int32_t*)(p + o), o += C * P.k * P.l * N * sizeof(int32_t);
  l.mu = (uint64_t*)(p + o), o += C * 64;
  l.w1 = p + o, o += C * P.w1_bytes();
  l.c = (uint32_t*)(p + o), o += C * N;
  l.flags = (uint32_t*)(p + o), o += C * sizeof(uint32_t);
  l.bytes = o;
  return l;
}

template <int PS>
static hipError_t run(size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* off, const uint8_t* sig,
                      const uint8_t* ctx, size_t ctx_len, int32_t* status, const MldsaTrace& tr, void* scratch,
                      hipStream_t st) {
  constexpr Params P = Set<PS>::P;
  const Layout l = layout(P, n, scratch);
  const dim3 lanes((unsigned)((n + 63) / 64)), polys((unsigned)((n * P.k * P.l + 63) / 64));
  QRK_LAUNCH("k_mldsa_front", st, k_mldsa_front<PS>, lanes, dim3(64), 0, st, n, pk, msg, off, sig, ctx,
             (uint32_t)ctx_len, l.mu, l.c, l.flags);
  QRK_LAUNCH("k_mldsa_expand", st, k_mldsa_expand<PS>, polys, dim3(64), 0, st, n, pk, l.A);
  QRK_LAUNCH("k_mldsa_core", st, k_mldsa_core<PS>, dim3((unsigned)n), dim3(256), 0, st, pk, sig, l.A,
             (const int8_t*)l.c, l.w1, l.flags);
  QRK_LAUNCH("k_mldsa_final", st, k_mldsa_final<PS>, lanes, dim3(64), 0, st, n, sig, l.mu, l.w1, l.flags, status, tr);
  return launch_status();
}

static const Params& params_of(int which) { return which == 0 ? P44 : which == 1 ? P65 : P87; }

}  // namespace mldsa

int mldsa_find(const char* name) {
  static const char* const NAMES[3] = {"ML-DSA-44", "ML-DSA-65", "ML-DSA-87"};
  for (int i = 0; name && i < 3; ++i)
    if (!strcmp(name, NAMES[i])) return i;
  return -1;
}

SigSizes mldsa_sizes(int which) {
  const mldsa::Params& P = mldsa::params_of(which);
  return {(size_t)P.pk, (size_t)P.sk, (size_t)P.sig, 0};
}

MldsaTrace mldsa_trace_at(int which, const MldsaTrace& t, size_t row) {
  if (!t.flags) return t;
  return {t.mu + row * 64, t.ctilde + row * 64, t.w1 + row * mldsa::params_of(which).w1_bytes(), t.flags + row};
}

size_t mldsa_scratch_bytes(int which, size_t chunk) {
  return mldsa::layout(mldsa::params_of(which), chunk, nullptr).bytes;
}

hipError_t mldsa_verify(int which, size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* msg_off,
                        const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len, int32_t* status,
                        const MldsaTrace& trace, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || n > (1u << 24)) return hipErrorInvalidValue;  // grids of n and n k l / 64 workgroups
  return with_which<3>(which, [&](auto ps) {
    return mldsa::run<decltype(ps)::value>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
  });
}

}  // namespace qrk
