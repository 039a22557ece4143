// ML-DSA key sets for gfx950: verification and signing of n rows under g keys that were expanded once.
//
// A node signs every message with one identity key and verifies what a peer sends against that peer's one key
// (quantum_resistant_p2p/app/messaging.py:600-620, 721, 864, 933, 1090, 1174, 1480, 1622), so a batch is many rows
// under a handful of keys.  The per-row calls (mldsa.hip, mldsa_sign.hip) redo for every row what depends on the
// key alone: ExpandA(rho), tr = H(pk, 64), the forward NTTs of t1 2^d or of s1, s2, t0, and a round trip of A_hat
// through scratch.  Here that work runs once per key, and a row names its key by index.
//
// Expansion of a set, stream-ordered, once (mldsa_keyset_expand):
//   k_mldsa_keyset_expand  one lane per polynomial of A_hat = ExpandA(rho) over all g k l polynomials
//                          (expand_a_block, rho read from the pk or sk rows)
//   k_mldsa_keyset_tr      public set, one lane per key: tr = H(pk, 64)
//   k_mldsa_keyset_t1      public set, one workgroup of 256 threads per key: (t1 2^d)_hat, reduced to [0, q)
//   k_mldsa_keyset_secret  secret set, one workgroup per key: rho | K | tr copied out, skDecode and NTT(s1),
//                          NTT(s2), NTT(t0) exactly as the per-row signing core forms them (sk_decode_ntt), and the
//                          key's refusal word: an s1 / s2 field outside [-eta, eta], ORed over all fields
// Layout of a set (mldsa_keyset_view), every part contiguous over the keys, 32-bit coefficients:
//   public  A_hat k l KiB | t1_hat k KiB | tr 64 bytes                      = 20544 / 36928 / 65600 bytes per key
//   secret  A_hat k l KiB | NTT(s1) l KiB | NTT(s2), NTT(t0) k KiB each | rho, K, tr 128 bytes | flag word
//                                                                           = 28804 / 48260 / 81028 bytes per key
// Verification of a chunk, three launches (the per-row path has four and k l KiB of scratch per row):
//   k_mldsa_keyed_front  one lane per row: the key index is checked against g before anything is addressed with
//                        it (FLAG_KEY: zeros to mu and c, the row is skipped like a FLAG_LONG row); mu from the
//                        set's tr, c = SampleInBall(c~)
//   k_mldsa_keyed_core   verify_core_body with A_hat and t1_hat of the row's key, no forward NTT of t1
//   k_mldsa_keyed_final  verify_final_body: the only writer of status, every row exactly once
// Signing of a chunk, two launches:
//   k_mldsa_keyed_sign_mu    one lane per row: the same index check, mu from the set's tr
//   k_mldsa_keyed_sign_core  sign_core_body with K, A_hat and the NTT'd secret vectors of the row's key; a row
//                            whose key carries the refusal word or whose index is outside the set gets status -1
//                            and an all-zero signature
// Scratch per row, public values only: mu, w1, c and a flag word (1092 / 1092 / 1348 bytes) for verification; mu
// and a flag word (68 bytes) for signing.
//
// Secret handling.  A secret set is the third place where secret-derived bytes live in global memory, next to
// the caller's `sk` rows and the accepted signature: K and NTT(s1), NTT(s2), NTT(t0) of every key stay in the
// set's allocation until qrk_mldsa_keyset_free, which synchronises the device and zeroes all of it before the
// memory is returned.  The rules of mldsa_sign.hip hold unchanged for the loop: inside an iteration no branch and
// no address depends on secret data (the key index is public, and it is the only thing besides the thread index
// that an address into the set is formed from), every LDS array is zeroed on exit, and nothing of the
// verification kernels, which leave early on data, is used on the signing side.
//
// The signing core can hold the three NTT'd vectors in LDS (copied in once per workgroup, SIGN_LDS) or read them
// from the set in every iteration (SIGN_L2: (2 k + l) KiB of LDS less per workgroup; a set of few keys stays in
// L2).  Both are built and g_mldsa_keyed_sign_mode picks one per launch.  Measured (profiles/mldsa/
// keyed_bench.jsonl) they are equal within the run's spread at 2^14 rows: occupancy is not what bounds the core.
// SIGN_LDS is the default, marginally ahead for a single signature.
#include "mldsa_cores.cuh"

namespace qrk {

std::atomic<int> g_mldsa_keyed_sign_mode{MLDSA_KEYED_SIGN_DEFAULT};

namespace mldsa {

static const Params& keyed_params_of(int which) { return which == 0 ? P44 : which == 1 ? P65 : P87; }

// ================================================================= expansion of a set
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_keyset_expand(size_t g, const uint8_t* __restrict__ keys, size_t stride,
                                                            int32_t* __restrict__ A) {
  __shared__ int tile[64 * EXPAND_STRIDE];
  expand_a_block<PS>(g, keys, stride, A, tile);  // rho: the first 32 bytes of a public or a secret key
}

template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_keyset_tr(size_t g, const uint8_t* __restrict__ pk,
                                                        uint64_t* __restrict__ tr) {
  constexpr Params P = Set<PS>::P;
  const size_t key = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (key >= g) return;
  const uint8_t* pkr = pk + key * P.pk;
  KState s;
  kzero(s);
  absorb_bytes<RW_SHAKE256, 0>(s, P.pk, [&](uint32_t i) -> uint32_t { return pkr[i]; });
#pragma unroll
  for (int w = 0; w < 8; ++w) tr[key * 8 + w] = kword(s, w);
}

template <int PS>
__global__ __launch_bounds__(256) void k_mldsa_keyset_t1(const uint8_t* __restrict__ pk, int32_t* __restrict__ t1h) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k;
  __shared__ int tp[K * N];
  const int tid = threadIdx.x;
  const size_t key = blockIdx.x;
  const uint8_t* t1p = pk + key * P.pk + 32;
  for (int i = 0; i < K; ++i) tp[i * N + tid] = t1_coeff_2d(t1p + 320 * i, tid);
  ntt_fwd(tp, K, tid, 256);  // input in [0, q): output below 5 q < 2^25.4
  // Stored in [0, q) (reduce: every int32 to within HALFQ; canon: |x| < 2 q to [0, q)), so the one product the
  // verification core forms with it, c_hat (t1 2^d)_hat, is below 2^25.1 * 2^23 = 2^48.1, against 2^50.5 for
  // the unreduced transform of the per-row core: the accumulate's bounds hold with room to spare.
  for (int i = 0; i < K; ++i) t1h[(key * K + i) * N + tid] = canon(reduce(tp[i * N + tid]));
}

template <int PS>
__global__ __launch_bounds__(256) void k_mldsa_keyset_secret(const uint8_t* __restrict__ sk, int32_t* __restrict__ s1o,
                                                             int32_t* __restrict__ s2o, int32_t* __restrict__ t0o,
                                                             uint8_t* __restrict__ head, uint32_t* __restrict__ bad) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l;
  __shared__ int s1h[L * N], s2h[K * N], t0h[K * N];
  __shared__ uint32_t s_bad;
  const int tid = threadIdx.x;
  const size_t key = blockIdx.x;
  const uint8_t* skr = sk + key * P.sk;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  sk_decode_ntt<PS>(skr, s1h, s2h, t0h, &s_bad, tid);
  if (tid < 128) head[key * 128 + tid] = skr[tid];  // rho | K | tr
  for (int e = tid; e < L * N; e += 256) s1o[key * L * N + e] = s1h[e];
  for (int e = tid; e < K * N; e += 256) s2o[key * K * N + e] = s2h[e], t0o[key * K * N + e] = t0h[e];
  if (tid == 0) bad[key] = s_bad;
  __syncthreads();
  for (int e = tid; e < L * N; e += 256) s1h[e] = 0;
  for (int e = tid; e < K * N; e += 256) s2h[e] = 0, t0h[e] = 0;
}

// ================================================================= Verify
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_keyed_front(size_t n, uint32_t g, const uint32_t* __restrict__ key_index,
                                                          const uint64_t* __restrict__ tr,
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
    const uint32_t key = key_index ? key_index[row] : 0u;
    uint32_t fl = 0;
    if (key >= g) {  // first: nothing is addressed with an index outside the set
      fl = FLAG_KEY;
    } else {
      const uint64_t o0 = off[row], o1 = off[row + 1];
      if (o1 < o0 || o1 - o0 >= (1ull << 31)) {
        fl = FLAG_LONG;
      } else {
        KState s;
        kzero(s);
#pragma unroll
        for (int w = 0; w < 8; ++w) kxor(s, w, tr[(size_t)key * 8 + w]);
        front_mu_c<PS>(s, row, msg + o0, (uint32_t)(o1 - o0), ctx, ctx_len, sig + row * P.sig, mu,
                       (int8_t*)cs[lane], sb[lane]);
      }
    }
    if (fl) {  // a skipped row: zeros to mu and c
#pragma unroll
      for (int w = 0; w < 8; ++w) mu[row * 8 + w] = 0;
      for (int w = 0; w < 64; ++w) cs[lane][w] = 0;
    }
    flags[row] = fl;
  }
  __syncthreads();
  for (int r = 0; r < 64 && base + r < n; ++r) cpoly[(base + r) * 64 + lane] = cs[r][lane];
}

template <int PS>
__global__ __launch_bounds__(256) void k_mldsa_keyed_core(uint32_t g, const uint32_t* __restrict__ key_index,
                                                          const int32_t* __restrict__ A,
                                                          const int32_t* __restrict__ t1h,
                                                          const uint8_t* __restrict__ sig,
                                                          const int8_t* __restrict__ cpoly, uint8_t* __restrict__ w1,
                                                          uint32_t* __restrict__ flags) {
  constexpr Params P = Set<PS>::P;
  const size_t row = blockIdx.x;
  if (flags[row] & (FLAG_LONG | FLAG_KEY)) return;  // the whole workgroup: the front flagged the row
  const size_t key = key_index ? key_index[row] : 0u;
  if (key >= g) return;  // the front's own check, again before the index is used: never taken after it
  verify_core_body<PS, true>(row, sig + row * P.sig, nullptr, t1h + key * P.k * N, A + key * P.k * P.l * N, cpoly, w1,
                             flags);
}

// The trace outputs (tests: qrk_dbg_mldsa_verify_keyed_trace) are all set or all NULL.
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_keyed_final(size_t n, const uint8_t* __restrict__ sig,
                                                          const uint64_t* __restrict__ mu,
                                                          const uint8_t* __restrict__ w1,
                                                          const uint32_t* __restrict__ flags,
                                                          int32_t* __restrict__ status, MldsaTrace tr) {
  verify_final_body<PS>(n, sig, mu, w1, flags, status, tr);
}

// ================================================================= Sign
template <int PS>
__global__ __launch_bounds__(64) void k_mldsa_keyed_sign_mu(size_t n, uint32_t g,
                                                            const uint32_t* __restrict__ key_index,
                                                            const uint8_t* __restrict__ head,
                                                            const uint8_t* __restrict__ msg,
                                                            const uint64_t* __restrict__ off,
                                                            const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                                            uint64_t* __restrict__ mu, uint32_t* __restrict__ flags) {
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  const uint32_t idx = key_index ? key_index[row] : 0u;
  const bool inside = idx < g;  // first: a row outside the set is flagged and reads no tr
  sign_mu_body(row, head + (size_t)(inside ? idx : 0u) * 128 + 64, inside ? 0u : FLAG_KEY, msg, off, ctx, ctx_len, mu,
               flags);
}

// TRACE (tests: qrk_dbg_mldsa_sign_keyed_trace) also stores mu and the iterations run.
template <int PS, bool TRACE, int MODE>
__global__ __launch_bounds__(256) void k_mldsa_keyed_sign_core(MldsaKeys ks, const uint32_t* __restrict__ key_index,
                                                               const uint8_t* __restrict__ rnd,
                                                               const uint64_t* __restrict__ mu,
                                                               const uint32_t* __restrict__ flags, uint32_t max_iters,
                                                               uint8_t* __restrict__ sig, int32_t* __restrict__ status,
                                                               uint8_t* __restrict__ tr_mu,
                                                               uint32_t* __restrict__ tr_iters) {
  constexpr Params P = Set<PS>::P;
  constexpr int K = P.k, L = P.l;
  const size_t row = blockIdx.x;
  const uint32_t idx = key_index ? key_index[row] : 0u;
  // A row outside the set carries FLAG_KEY from the mu kernel and is refused below; it is pointed at key 0, which
  // every set has, so that no address is formed from its index.  The index is public.
  const size_t key = idx < ks.g ? idx : 0u;
  const SignKey sk{ks.head + key * 128 + 32, ks.s1h + key * L * N, ks.s2h + key * K * N, ks.t0h + key * K * N,
                   ks.bad[key]};
  sign_core_body<PS, TRACE, MODE>(row, nullptr, sk, rnd, ks.A + key * K * L * N, mu + row * 8, flags[row], max_iters,
                                  sig + row * P.sig, status, tr_mu, tr_iters);
}

// ================================================================= host
static MldsaKeys view(const Params& P, bool secret, size_t g, void* mem, size_t* bytes) {
  uint8_t* p = (uint8_t*)mem;
  MldsaKeys v;
  size_t o = 0;
  const size_t poly = N * sizeof(int32_t);
  v.g = (uint32_t)g;
  v.A = (const int32_t*)(p + o), o += g * P.k * P.l * poly;
  if (secret) {
    v.s1h = (const int32_t*)(p + o), o += g * P.l * poly;
    v.s2h = (const int32_t*)(p + o), o += g * P.k * poly;
    v.t0h = (const int32_t*)(p + o), o += g * P.k * poly;
    v.head = p + o, o += g * 128;
    v.bad = (const uint32_t*)(p + o), o += g * sizeof(uint32_t);
  } else {
    v.t1h = (const int32_t*)(p + o), o += g * P.k * poly;
    v.head = p + o, o += g * 64;
  }
  if (bytes) *bytes = o;
  return v;
}

template <int PS>
static hipError_t run_expand(bool secret, size_t g, const uint8_t* keys, void* mem, hipStream_t st) {
  constexpr Params P = Set<PS>::P;
  const MldsaKeys v = view(P, secret, g, mem, nullptr);
  const dim3 lanes((unsigned)((g + 63) / 64)), polys((unsigned)((g * P.k * P.l + 63) / 64));
  QRK_LAUNCH("k_mldsa_keyset_expand", st, k_mldsa_keyset_expand<PS>, polys, dim3(64), 0, st, g, keys,
             (size_t)(secret ? P.sk : P.pk), (int32_t*)v.A);
  if (secret) {
    QRK_LAUNCH("k_mldsa_keyset_secret", st, k_mldsa_keyset_secret<PS>, dim3((unsigned)g), dim3(256), 0, st, keys,
               (int32_t*)v.s1h, (int32_t*)v.s2h, (int32_t*)v.t0h, (uint8_t*)v.head, (uint32_t*)v.bad);
  } else {
    QRK_LAUNCH("k_mldsa_keyset_tr", st, k_mldsa_keyset_tr<PS>, lanes, dim3(64), 0, st, g, keys, (uint64_t*)v.head);
    QRK_LAUNCH("k_mldsa_keyset_t1", st, k_mldsa_keyset_t1<PS>, dim3((unsigned)g), dim3(256), 0, st, keys,
               (int32_t*)v.t1h);
  }
  return launch_status();
}

// scratch of a chunk of C verified rows: mu | w1 | c | flags (every part a multiple of 8 bytes per row but the last)
struct KeyedLayout {
  uint64_t* mu;
  uint8_t* w1;
  uint32_t* c;
  uint32_t* flags;
  size_t bytes;
};
static KeyedLayout keyed_layout(const Params& P, size_t C, void* scratch) {
  uint8_t* p = (uint8_t*)scratch;
  KeyedLayout l;
  size_t o = 0;
  l.mu = (uint64_t*)(p + o), o += C * 64;
  l.w1 = p + o, o += C * P.w1_bytes();
  l.c = (uint32_t*)(p + o), o += C * N;
  l.flags = (uint32_t*)(p + o), o += C * sizeof(uint32_t);
  l.bytes = o;
  return l;
}

template <int PS>
static hipError_t run_verify(const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* msg,
                             const uint64_t* off, const uint8_t* sig, const uint8_t* ctx, size_t ctx_len,
                             int32_t* status, const MldsaTrace& tr, void* scratch, hipStream_t st) {
  constexpr Params P = Set<PS>::P;
  const KeyedLayout l = keyed_layout(P, n, scratch);
  const dim3 lanes((unsigned)((n + 63) / 64));
  QRK_LAUNCH("k_mldsa_keyed_front", st, k_mldsa_keyed_front<PS>, lanes, dim3(64), 0, st, n, ks.g, key_index,
             (const uint64_t*)ks.head, msg, off, sig, ctx, (uint32_t)ctx_len, l.mu, l.c, l.flags);
  QRK_LAUNCH("k_mldsa_keyed_core", st, k_mldsa_keyed_core<PS>, dim3((unsigned)n), dim3(256), 0, st, ks.g, key_index,
             ks.A, ks.t1h, sig, (const int8_t*)l.c, l.w1, l.flags);
  QRK_LAUNCH("k_mldsa_keyed_final", st, k_mldsa_keyed_final<PS>, lanes, dim3(64), 0, st, n, sig, l.mu, l.w1, l.flags,
             status, tr);
  return launch_status();
}

template <int PS, bool TRACE, int MODE>
static void launch_sign_core(const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* rnd,
                             const uint64_t* mu, const uint32_t* flags, uint32_t max_iters, uint8_t* sig,
                             int32_t* status, uint8_t* tr_mu, uint32_t* tr_iters, hipStream_t st) {
  QRK_LAUNCH("k_mldsa_keyed_sign_core", st, (k_mldsa_keyed_sign_core<PS, TRACE, MODE>), dim3((unsigned)n), dim3(256), 0,
             st, ks, key_index, rnd, mu, flags, max_iters, sig, status, tr_mu, tr_iters);
}

template <int PS>
static hipError_t run_sign(const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* msg,
                           const uint64_t* off, const uint8_t* rnd, const uint8_t* ctx, size_t ctx_len, uint8_t* sig,
                           int32_t* status, uint32_t max_iters, uint8_t* tr_mu, uint32_t* tr_iters, void* scratch,
                           hipStream_t st) {
  uint64_t* mu = (uint64_t*)scratch;                        // scratch of a chunk of n rows: mu | flags
  uint32_t* flags = (uint32_t*)((uint8_t*)scratch + n * 64);
  const dim3 lanes((unsigned)((n + 63) / 64));
  QRK_LAUNCH("k_mldsa_keyed_sign_mu", st, k_mldsa_keyed_sign_mu<PS>, lanes, dim3(64), 0, st, n, ks.g, key_index,
             ks.head, msg, off, ctx, (uint32_t)ctx_len, mu, flags);
  const bool lds = g_mldsa_keyed_sign_mode.load(std::memory_order_relaxed) == SIGN_LDS;
  auto core = tr_iters ? (lds ? launch_sign_core<PS, true, SIGN_LDS> : launch_sign_core<PS, true, SIGN_L2>)
                       : (lds ? launch_sign_core<PS, false, SIGN_LDS> : launch_sign_core<PS, false, SIGN_L2>);
  core(ks, n, key_index, rnd, mu, flags, max_iters, sig, status, tr_mu, tr_iters, st);
  return launch_status();
}

}  // namespace mldsa

size_t mldsa_keyset_bytes(int which, bool secret, size_t g) {
  size_t bytes = 0;
  mldsa::view(mldsa::keyed_params_of(which), secret, g, nullptr, &bytes);
  return bytes;
}

MldsaKeys mldsa_keyset_view(int which, bool secret, size_t g, void* mem) {
  return mldsa::view(mldsa::keyed_params_of(which), secret, g, mem, nullptr);
}

hipError_t mldsa_keyset_expand(int which, bool secret, size_t g, const uint8_t* keys, void* mem, hipStream_t st) {
  if (g == 0 || g > (1u << 24)) return hipErrorInvalidValue;  // grids of g and g k l / 64 workgroups
  return with_which<3>(which, [&](auto ps) {
    return mldsa::run_expand<decltype(ps)::value>(secret, g, keys, mem, st);
  });
}

size_t mldsa_keyed_scratch_bytes(int which, size_t chunk) {
  return mldsa::keyed_layout(mldsa::keyed_params_of(which), chunk, nullptr).bytes;
}

size_t mldsa_keyed_sign_scratch_bytes(int, size_t chunk) { return chunk * (64 + sizeof(uint32_t)); }

hipError_t mldsa_verify_keyed(int which, const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* msg,
                              const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                              int32_t* status, const MldsaTrace& trace, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || n > (1u << 24) || ks.g == 0) return hipErrorInvalidValue;  // a grid of n workgroups
  return with_which<3>(which, [&](auto ps) {
    return mldsa::run_verify<decltype(ps)::value>(ks, n, key_index, msg, msg_off, sig, ctx_str, ctx_len, status, trace,
                                                  scratch, st);
  });
}

hipError_t mldsa_sign_keyed(int which, const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* msg,
                            const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len,
                            uint8_t* sig, int32_t* status, uint32_t max_iters, uint8_t* trace_mu,
                            uint32_t* trace_iters, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || n > (1u << 24) || ks.g == 0) return hipErrorInvalidValue;
  return with_which<3>(which, [&](auto ps) {
    return mldsa::run_sign<decltype(ps)::value>(ks, n, key_index, msg, msg_off, rnd, ctx_str, ctx_len, sig, status,
                                                max_iters, trace_mu, trace_iters, scratch, st);
  });
}

}  // namespace qrk
