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

#include "mldsa_cores.cuh"

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
      front_mu_c<PS>(s, row, m, mlen, ctx, ctx_len, sig + row * P.sig, mu, (int8_t*)cs[lane], sb[lane]);
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
  const size_t row = blockIdx.x;
  if (flags[row] & FLAG_LONG) return;  // the whole workgroup: k_mldsa_front wrote nothing else for it
  verify_core_body<PS, false>(row, sig + row * P.sig, pk + row * P.pk + 32, nullptr, A + row * P.k * P.l * N, cpoly,
                              w1, flags);
}

// The trace outputs (tests: qrk_dbg_mldsa_verify_trace) are all set or all NULL.
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_final(size_t n, const uint8_t* __restrict__ sig,
                                                    const uint64_t* __restrict__ mu, const uint8_t* __restrict__ w1,
                                                    const uint32_t* __restrict__ flags, int32_t* __restrict__ status,
                                                    MldsaTrace tr) {
  verify_final_body<PS>(n, sig, mu, w1, flags, status, tr);
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
