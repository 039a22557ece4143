// ML-KEM key sets (FIPS 203): g keys expanded once, and Encaps / Decaps of n rows that name their key by index.
//
// What depends on the key alone is computed when the set is loaded and never again per row: the matrix A_hat
// (SampleNTT with as many blocks as an entry takes, so the fix-up is part of the load), H(ek) and Encaps'
// modulus check on ek.  A row then costs its own sponges (G, the PRFs; Decaps: J) and the polynomial cores:
//   Encaps  G(m || H(ek)) -> PRFs -> K-PKE.Encrypt                        (8 of the per-row call's 44 permutations
//                                                                          at ML-KEM-768, no SampleNTT launch)
//   Decaps  {J(z || c), K-PKE.Decrypt} -> G(m' || h) -> PRFs -> re-encryption, compare and select
// In the set an entry of A_hat is one contiguous 384-byte run of 12-bit coefficients per (key, x, y) -- the
// batched layout's tile width 1 (mlkem_layout.cuh) -- because a 16-lane group reads one key's entry while its
// neighbours in the wave read other keys': nothing here assumes that neighbouring rows name neighbouring keys.
// A row's index is checked against g before any address is formed from it; a refused row runs on key 0 (so no
// step's work depends on it), and its outputs are zeroed and its status set to -1 at the end.
//
// A translation unit of its own on purpose: it instantiates none of mlkem.hip's kernels and so leaves their
// code as it is (profiles/mlkem_keyed/resources_*.txt).  The device functions come from the headers the
// batched path is built from; keyed_core_hs is encrypt_core_hs (mlkem_batch.cuh) with the matrix, ek and the
// modulus verdict read through the key index.
#include "keccak.cuh"
#include "mlkem_layout.cuh"
#include "mlkem_paths.h"
#include "mlkem_poly.cuh"
#include "mlkem_sample.cuh"

namespace qrk {
namespace mlkem {

// ------------------------------------------------------------ the set
// A_hat [g][K K] entries of XUNITS units | the key bytes [g][stride] (public: ek; secret: dk) | public only:
// H(ek) [g][32] | the modulus verdict [g] (nonzero: a coefficient of t_hat is >= q).  Every part starts 256-aligned.
struct SetLayout {
  size_t a_bytes, key_bytes, h_off, bad_off, total;
};
static SetLayout set_layout(int K, bool secret, size_t g) {
  SetLayout l;
  l.a_bytes = al256((size_t)K * K * g * XUNITS * sizeof(XUnit));
  const size_t stride = secret ? 768 * (size_t)K + 96 : 384 * (size_t)K + 32;
  l.key_bytes = al256(stride * g);
  l.h_off = l.a_bytes + l.key_bytes;
  l.bad_off = l.h_off + (secret ? 0 : al256(32 * g));
  l.total = l.bad_off + (secret ? 0 : al256(4 * g));
  return l;
}

struct KeyRef {
  uint32_t key;  // < g: what addresses are formed from
  bool ok;       // the row's index was in range
};
__device__ __forceinline__ KeyRef key_of(const uint32_t* __restrict__ key_index, size_t hs, uint32_t g) {
  const uint32_t k = key_index ? key_index[hs] : 0u;
  const bool ok = k < g;
  return {ok ? k : 0u, ok};
}

// ------------------------------------------------------------ load
// SampleNTT, one lane per (key, x, y), into the key's contiguous entries; an entry that needs a 4th block (or
// more) takes it in place: the load runs once, so the rare long entry may idle its wave.
template <int K>
__global__ __launch_bounds__(256) void k_keyed_expand(size_t g, const uint8_t* __restrict__ keys, size_t stride,
                                                      size_t rho_off, XUnit* __restrict__ A) {
  __shared__ __attribute__((aligned(16))) uint32_t ring_all[XOF_LDS / 4];
  const uint32_t rb = ((threadIdx.x >> 6) * 16 * 64 + (threadIdx.x & 63)) * 4;  // ring_all: [wave][16][64]
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * K * g) return;
  const size_t key = e / (K * K);
  const int xy = (int)(e % (K * K));
  xof_entry<K, true, 1>((const uint64_t*)(keys + key * stride + rho_off), xy, e, A, (char*)ring_all, rb);
}

// H(ek) and the FIPS 203 7.2 modulus check, one lane per public key
template <int K>
__global__ __launch_bounds__(256) void k_keyed_pub(size_t g, const uint8_t* __restrict__ keys,
                                                   uint64_t* __restrict__ h, uint32_t* __restrict__ bad) {
  const size_t key = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (key >= g) return;
  const uint64_t* ek = (const uint64_t*)(keys + key * P<K>::PK);
  KState s;
  kzero(s);
  absorb_words<RW_SHA3_256, P<K>::PK / 8, DS_SHA3, false>(s, [&](int w) { return ek[w]; });
#pragma unroll
  for (int w = 0; w < 4; ++w) h[key * 4 + w] = kword(s, w);
  bool b = false;
#pragma unroll 1
  for (int w = 0; w < 48 * K; w += 3) (void)decode12_w(ek[w], ek[w + 1], ek[w + 2], b);
  bad[key] = b ? 1u : 0u;
}

// ------------------------------------------------------------ rows
struct KeyedArgs {
  uint32_t g;
  const XUnit* A;
  const uint8_t* keys;  // public: ek rows; secret: dk rows
  size_t stride;
  const uint64_t* h;    // public sets
  const uint32_t* bad;  // public sets
  const uint32_t* key_index;
};

// Encaps front: (K, r) = G(m || H(ek)) with the stored H(ek); K -> ss (zeros for a refused row), r -> seeds
template <int K>
struct RKFrontEnc {
  static constexpr int LDS = 0, WPE = 1;
  KeyedArgs a;
  const uint8_t* coins;
  size_t n;
  uint8_t* ss;
  uint64_t* seeds;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t hs = (size_t)vb * 256 + threadIdx.x;
    if (hs >= n) return;
    const KeyRef kr = key_of(a.key_index, hs, a.g);
    const uint64_t* h = a.h + (size_t)kr.key * 4;
    const uint64_t* m = (const uint64_t*)(coins + hs * 32);
    KState s;
    kzero(s);
    absorb_words<RW_SHA3_512, 8, DS_SHA3>(s, [&](int w) { return w < 4 ? m[w] : h[w - 4]; });
    uint64_t* K_out = (uint64_t*)(ss + hs * 32);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      K_out[w] = kr.ok ? kword(s, w) : 0ull;
      seeds[hs * 4 + w] = kword(s, 4 + w);
    }
  }
};
// Decaps: Kbar = J(z || c), z from the row's key
template <int K>
struct RKJDec {
  static constexpr int LDS = 0, WPE = 1;
  KeyedArgs a;
  const uint8_t* ct;
  size_t n;
  uint64_t* kbar;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t hs = (size_t)vb * 256 + threadIdx.x;
    if (hs >= n) return;
    const KeyRef kr = key_of(a.key_index, hs, a.g);
    const uint64_t* z = (const uint64_t*)(a.keys + (size_t)kr.key * a.stride + 768 * K + 64);
    const uint64_t* c = (const uint64_t*)(ct + hs * P<K>::CT);
    KState s;
    kzero(s);
    absorb_words<RW_SHAKE256, 4 + P<K>::CT / 8, DS_SHAKE, false>(s, [&](int w) { return w < 4 ? z[w] : c[w - 4]; });
#pragma unroll
    for (int w = 0; w < 4; ++w) kbar[hs * 4 + w] = kword(s, w);
  }
};
// Decaps: (K', r') = G(m' || h), h from the row's key
template <int K>
struct RKGDec {
  static constexpr int LDS = 0, WPE = 1;
  KeyedArgs a;
  const uint64_t* mprime;
  size_t n;
  uint64_t *seeds, *kprime;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t hs = (size_t)vb * 256 + threadIdx.x;
    if (hs >= n) return;
    const KeyRef kr = key_of(a.key_index, hs, a.g);
    const uint64_t* h = (const uint64_t*)(a.keys + (size_t)kr.key * a.stride + 768 * K + 32);
    const uint64_t* m = mprime + hs * 4;
    KState s;
    kzero(s);
    absorb_words<RW_SHA3_512, 8, DS_SHA3>(s, [&](int w) { return w < 4 ? m[w] : h[w - 4]; });
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      kprime[hs * 4 + w] = kword(s, w);
      seeds[hs * 4 + w] = kword(s, 4 + w);
    }
  }
};
template <int ETA1, int ETA2>
struct RKPrf {  // PRF_eta(seed, N), lane / (N, row): rows only, no key
  static constexpr int LDS = 0, WPE = 1;
  const uint64_t* seeds;
  size_t n, C;
  int nprf, eta1_upto;
  uint64_t* prf;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t inst = (size_t)vb * 256 + threadIdx.x;
    if (inst >= (size_t)nprf * C || inst % C >= n) return;
    prf_inst<ETA1, ETA2>(seeds + (inst % C) * 4, (int)(inst / C), inst, eta1_upto, prf);
  }
};
// Decaps: m' = K-PKE.Decrypt(dk, c), 16 lanes / row, dk_pke from the row's key
template <int K>
struct RKDecrypt {
  static constexpr int LDS = GROUPS * (int)sizeof(GroupLds), WPE = 1;
  KeyedArgs a;
  size_t n;
  const uint8_t* ct;
  uint64_t* mprime;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char* lds) const {
    const int gi = threadIdx.x >> 4;
    const size_t hs_raw = (size_t)vb * GROUPS + gi;
    const size_t hs = hs_raw < n ? hs_raw : n - 1;
    const KeyRef kr = key_of(a.key_index, hs, a.g);
    // the pointer form of the core (TW != 64): this row's c, its key's dk, this row's m'
    decrypt_core_hs<K, 16>(n, ct + hs * P<K>::CT, a.keys + (size_t)kr.key * a.stride, mprime + hs * 4, hs_raw,
                           threadIdx.x & 15, ((GroupLds*)lds)[gi]);
  }
};

// K-PKE.Encrypt under a key of the set.  MODE 0 (Encaps): write c and the key's modulus verdict.  MODE 1
// (Decaps): compare c' with the input c and select K' or Kbar in constant time.  encrypt_core_hs with
// A_hat[key], ek[key] in place of the row's own; a refused row computes on key 0 and stores zeros.
template <int K, int MODE>
__device__ __forceinline__ void keyed_core_hs(size_t n, size_t C, const KeyedArgs& a, size_t ek_off,
                                              const uint64_t* __restrict__ prf, const uint8_t* __restrict__ m_base,
                                              uint8_t* __restrict__ ct, int32_t* __restrict__ status,
                                              const uint64_t* __restrict__ kprime, const uint64_t* __restrict__ kbar,
                                              uint8_t* __restrict__ ss, size_t hs_raw, int L, GroupLds& g) {
  constexpr int DU = P<K>::DU, DV = P<K>::DV;
  const bool active = hs_raw < n;
  const size_t hs = active ? hs_raw : n - 1;  // index in the chunk
  const KeyRef kr = key_of(a.key_index, hs, a.g);
  const bool store = active && kr.ok;
  const XUnit* xof = a.A + (size_t)kr.key * (K * K * XUNITS);
  uint8_t* c = ct + hs * P<K>::CT;
  uint32_t diff = 0;

  BOp yb[K];
  {
    CbdRaw yr[K];
#pragma unroll
    for (int j = 0; j < K; ++j) yr[j] = cbd_load<P<K>::ETA1, 64>(prf, (size_t)j * C + hs, L);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      PF16 f;
      cbd_f<P<K>::ETA1>(f, yr[j]);
      contig_to_stride_f(f, (float*)g.poly, L);
      ntt_fwd_f<false>(f, (float*)g.poly, L);
      yb[j] = make_bop_f(f, L);
    }
  }
  // u_i = NTT^-1(sum_j A[j][i] o y_j) + e1_i; row i + 1's entries are loaded one row ahead
  PK8 an[K];
#pragma unroll
  for (int j = 0; j < K; ++j) an[j] = load_sampled<1, true>(xof, (size_t)j, L);
  CbdRaw er = cbd_load<P<K>::ETA2, 64>(prf, (size_t)K * C + hs, L);
  auto row = [&](int i, auto last_t) {
    constexpr bool LAST = decltype(last_t)::value;
    int acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) basemul_acc(acc, an[j], yb[j]);
    const CbdRaw ecur = er;
    if (!LAST) {
      if (i + 1 < K) {
#pragma unroll
        for (int j = 0; j < K; ++j) an[j] = load_sampled<1, true>(xof, (size_t)((i + 1) * K + j), L);
      }
    } else {
      // last row: t_hat's 24 bytes per lane and row go into the matrix registers
      const uint8_t* ek = a.keys + (size_t)kr.key * a.stride + ek_off;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const uint2* e = (const uint2*)(ek + 384 * j + 24 * L);
        const uint2 p = e[0], q = e[1], r = e[2];
        an[j].w[0] = p.x, an[j].w[1] = p.y, an[j].w[2] = q.x, an[j].w[3] = q.y, an[j].w[4] = r.x, an[j].w[5] = r.y;
      }
    }
    er = cbd_load<P<K>::ETA2, 64>(prf, (size_t)(K + i + 1) * C + hs, L);  // e1_{i+1}, or e2 after the last row
    PF16 uf;
#pragma unroll
    for (int t = 0; t < 16; ++t) uf.v[t] = acc_to_f(acc[t]);
    ntt_inv_f(uf, (float*)g.poly, L);
    CmpWords<DU> cw;
    if (MODE) cw = cmp_load<DU>(c + 32 * DU * i, L);
    stride_to_contig_f(uf, (float*)g.poly, L);
    PF16 ef;
    cbd_f<P<K>::ETA2>(ef, ecur);
    P16 u;
#pragma unroll
    for (int t = 0; t < 16; ++t) u.v[t] = compress_f<DU>(uf.v[t] + ef.v[t]);
    pack_bits<DU>(u, g, L);
    if (MODE)
      flush_cmp<DU>(g, cw, diff, L);
    else
      flush_bits<DU>(g, c + 32 * DU * i, nullptr, diff, store, L);
  };
#pragma unroll 1
  for (int i = 0; i < K - 1; ++i) row(i, std::false_type{});
  row(K - 1, std::true_type{});
  // v = NTT^-1(t_hat^T o y_hat) + e2 + Decompress_1(m)
  {
    int acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0;
    bool bad = false;  // the verdict was taken at load (KeyedArgs::bad)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint32_t w[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) w[t] = an[j].w[t];
      const uint64_t p = ((uint64_t)w[1] << 32) | w[0], q = ((uint64_t)w[3] << 32) | w[2],
                     r = ((uint64_t)w[5] << 32) | w[4];
      basemul_acc(acc, decode12_w(p, q, r, bad), yb[j]);
    }
    PF16 vf;
#pragma unroll
    for (int t = 0; t < 16; ++t) vf.v[t] = acc_to_f(acc[t]);
    ntt_inv_f(vf, (float*)g.poly, L);
    stride_to_contig_f(vf, (float*)g.poly, L);
    PF16 ef;
    cbd_f<P<K>::ETA2>(ef, er);  // e2
    const uint8_t* m = m_base + hs * 32;
    const uint32_t mb = (uint32_t)m[2 * L] | ((uint32_t)m[2 * L + 1] << 8);
    P16 v;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float mu = ((mb >> t) & 1) ? (float)((Q + 1) / 2) : 0.0f;
      v.v[t] = compress_f<DV>(vf.v[t] + ef.v[t] + mu);
    }
    pack_bits<DV>(v, g, L);
    flush_bits<DV>(g, c + 32 * DU * K, MODE ? c + 32 * DU * K : nullptr, diff, store, L);
  }
  if constexpr (MODE == 0) {
    if (active && !kr.ok) {  // a refused row: nothing above stored to it
#pragma unroll 1
      for (int idx = L; idx < P<K>::CT / 4; idx += 16) ((uint32_t*)c)[idx] = 0u;
    }
    if (active && L == 0 && status) status[hs] = (!kr.ok || a.bad[kr.key]) ? -1 : 0;
  } else {
    // constant-time select: ss = (c == c') ? K' : Kbar; a refused row's ss is zero
    const uint32_t d = group_or(diff);
    const uint32_t mask = (uint32_t)(((uint64_t)d - 1u) >> 32);  // all-ones iff d == 0, no branch
    const uint32_t keep = kr.ok ? 0xFFFFFFFFu : 0u;
    if (L < 8) {
      const uint32_t kp = ((const uint32_t*)(kprime + hs * 4))[L];
      const uint32_t kb = ((const uint32_t*)(kbar + hs * 4))[L];
      if (active) ((uint32_t*)(ss + hs * 32))[L] = ((kp & mask) | (kb & ~mask)) & keep;
    }
    if (active && L == 0 && status) status[hs] = kr.ok ? 0 : -1;
  }
}

// the cores' waves per SIMD: as the per-row cores (RCore, mlkem_batch.cuh)
template <int K, int MODE>
struct RKCore {
  static constexpr int LDS = GROUPS * (int)sizeof(GroupLds), WPE = (K == 4 && MODE == 1) ? 1 : 3;
  KeyedArgs a;
  size_t ek_off, n, C;
  const uint64_t* prf;
  const uint8_t* m_base;
  uint8_t* ct;
  int32_t* status;
  const uint64_t *kprime, *kbar;
  uint8_t* ss;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char* lds) const {
    const int gi = threadIdx.x >> 4;
    keyed_core_hs<K, MODE>(n, C, a, ek_off, prf, m_base, ct, status, kprime, kbar, ss, (size_t)vb * GROUPS + gi,
                           threadIdx.x & 15, ((GroupLds*)lds)[gi]);
  }
};

// One role per launch, or two that do not depend on each other in one launch, the first role's workgroups first
// (the schedule of k_multi, mlkem_batch.cuh; a role synchronises at most within a wave)
template <class R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R::WPE))) void k_keyed_role(R r) {
  constexpr int L = R::LDS;
  __shared__ __attribute__((aligned(16))) char lds[L > 16 ? L : 16];
  r.run(blockIdx.x, lds);
}
template <class R0, class R1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R0::WPE > R1::WPE ? R0::WPE : R1::WPE)))
void k_keyed_pair(R0 r0, R1 r1) {
  constexpr int L = R0::LDS > R1::LDS ? R0::LDS : R1::LDS;
  __shared__ __attribute__((aligned(16))) char lds[L > 16 ? L : 16];
  if (blockIdx.x < r0.nb)
    r0.run(blockIdx.x, lds);
  else
    r1.run(blockIdx.x - r0.nb, lds);
}
template <class R>
static void launch_role(const char* name, const R& r, const Streams& s) {
  if (r.nb) QRK_LAUNCH(name, s.main, k_keyed_role<R>, dim3(r.nb), dim3(256), 0, s.main, r);
}
template <class R0, class R1>
static void launch_pair(const char* name, const char* n0, const char* n1, const R0& r0, const R1& r1,
                        const Streams& s) {
  if (s.serial) {
    launch_role(n0, r0, s);
    launch_role(n1, r1, s);
    return;
  }
  if (r0.nb + r1.nb)
    QRK_LAUNCH(name, s.main, (k_keyed_pair<R0, R1>), dim3(r0.nb + r1.nb), dim3(256), 0, s.main, r0, r1);
}

// ------------------------------------------------------------ host
// Per-row scratch of a chunk of C rows: the PRF words, then seeds | m' | K' | Kbar (4 C words each).  No matrix.
struct KeyedScratch {
  uint64_t *prf, *seeds, *mprime, *kprime, *kbar;
};
static size_t keyed_scratch_words(int K, size_t C) { return (size_t)(2 * K + 1) * C * PRF_W + 16 * C; }
static KeyedScratch keyed_carve(void* base, int K, size_t C) {
  KeyedScratch v;
  v.prf = (uint64_t*)base;
  v.seeds = v.prf + (size_t)(2 * K + 1) * C * PRF_W;
  v.mprime = v.seeds + 4 * C;
  v.kprime = v.mprime + 4 * C;
  v.kbar = v.kprime + 4 * C;
  return v;
}

static KeyedArgs args_of(const MlkemKeys& ks, const uint32_t* key_index) {
  return {ks.g, (const XUnit*)ks.A, ks.keys, ks.stride, (const uint64_t*)ks.h, ks.bad, key_index};
}

template <int K>
static hipError_t expand_impl(bool secret, size_t g, const uint8_t* keys, void* mem, hipStream_t st) {
  const SetLayout l = set_layout(K, secret, g);
  const size_t stride = secret ? P<K>::SK : P<K>::PK;
  uint8_t* base = (uint8_t*)mem;
  qrk_chk(hipMemsetAsync(mem, 0, l.total, st));  // the padding between the parts too
  qrk_chk(hipMemcpyAsync(base + l.a_bytes, keys, stride * g, hipMemcpyDeviceToDevice, st));
  if (launch_status() != hipSuccess) return launch_status();
  const uint8_t* kb = base + l.a_bytes;
  QRK_LAUNCH("k_keyed_expand", st, k_keyed_expand<K>, dim3(blocks_for((size_t)K * K * g)), dim3(256), 0, st, g, kb,
             stride, (size_t)(secret ? 768 * K : 384 * K), (XUnit*)base);
  if (!secret)
    QRK_LAUNCH("k_keyed_pub", st, k_keyed_pub<K>, dim3(blocks_for(g)), dim3(256), 0, st, g, kb,
               (uint64_t*)(base + l.h_off), (uint32_t*)(base + l.bad_off));
  return launch_status();
}

// G -> PRFs -> K-PKE.Encrypt
template <int K>
static hipError_t encaps_impl(const MlkemKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ct, uint8_t* ss,
                              const uint8_t* coins, int32_t* status, void* scratch, const Streams& s) {
  const size_t C = round64(n);
  const KeyedScratch v = keyed_carve(scratch, K, C);
  const KeyedArgs a = args_of(ks, key_index);
  launch_role("k_keyed_front_encaps", RKFrontEnc<K>{a, coins, n, ss, v.seeds, blocks_for(n)}, s);
  launch_role("k_keyed_prf",
              RKPrf<P<K>::ETA1, P<K>::ETA2>{v.seeds, n, C, 2 * K + 1, K, v.prf, blocks_for((2 * K + 1) * C)}, s);
  launch_role("k_keyed_encrypt_core",
              RKCore<K, 0>{a, 0, n, C, v.prf, coins, ct, status, nullptr, nullptr, nullptr,
                           (unsigned)((n + GROUPS - 1) / GROUPS)},
              s);
  return launch_status();
}

// {J, K-PKE.Decrypt} -> G -> PRFs -> re-encryption, compare, select
template <int K>
static hipError_t decaps_impl(const MlkemKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ss, const uint8_t* ct,
                              int32_t* status, void* scratch, const Streams& s) {
  const size_t C = round64(n);
  const KeyedScratch v = keyed_carve(scratch, K, C);
  const KeyedArgs a = args_of(ks, key_index);
  const unsigned gblocks = (unsigned)((n + GROUPS - 1) / GROUPS);
  launch_pair("k_keyed_j_decaps+k_keyed_decrypt_core", "k_keyed_j_decaps", "k_keyed_decrypt_core",
              RKJDec<K>{a, ct, n, v.kbar, blocks_for(n)}, RKDecrypt<K>{a, n, ct, v.mprime, gblocks}, s);
  launch_role("k_keyed_g_decaps", RKGDec<K>{a, v.mprime, n, v.seeds, v.kprime, blocks_for(n)}, s);
  launch_role("k_keyed_prf",
              RKPrf<P<K>::ETA1, P<K>::ETA2>{v.seeds, n, C, 2 * K + 1, K, v.prf, blocks_for((2 * K + 1) * C)}, s);
  launch_role("k_keyed_encrypt_core",
              RKCore<K, 1>{a, (size_t)384 * K, n, C, v.prf, (const uint8_t*)v.mprime, const_cast<uint8_t*>(ct), status,
                           v.kprime, v.kbar, ss, gblocks},
              s);
  return launch_status();
}

}  // namespace mlkem

size_t mlkem_keyset_bytes(const AlgInfo& a, bool secret, size_t g) { return mlkem::set_layout(a.k, secret, g).total; }

MlkemKeys mlkem_keyset_view(const AlgInfo& a, bool secret, size_t g, void* mem) {
  const mlkem::SetLayout l = mlkem::set_layout(a.k, secret, g);
  const uint8_t* base = (const uint8_t*)mem;
  MlkemKeys v;
  v.g = (uint32_t)g;
  v.A = base;
  v.keys = base + l.a_bytes;
  v.stride = secret ? a.sk : a.pk;
  if (!secret) {
    v.h = base + l.h_off;
    v.bad = (const uint32_t*)(base + l.bad_off);
  }
  return v;
}

hipError_t mlkem_keyset_expand(const AlgInfo& a, bool secret, size_t g, const uint8_t* keys, void* mem,
                               hipStream_t st) {
  return mlkem::with_rank(
      a.k, [&](auto rank) { return mlkem::expand_impl<decltype(rank)::value>(secret, g, keys, mem, st); });
}

size_t mlkem_keyed_scratch_bytes(const AlgInfo& a, size_t chunk) {
  return mlkem::keyed_scratch_words(a.k, round64(chunk)) * sizeof(uint64_t);
}

hipError_t mlkem_keyed_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const size_t C = round64(n);
  return hipMemsetAsync(mlkem::keyed_carve(scratch, a.k, C).seeds, 0, 16 * C * sizeof(uint64_t), st);
}

hipError_t mlkem_encaps_keyed(const AlgInfo& a, const MlkemKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ct,
                              uint8_t* ss, const uint8_t* coins, int32_t* status, void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  return mlkem::with_rank(a.k, [&](auto rank) {
    return mlkem::encaps_impl<decltype(rank)::value>(ks, n, key_index, ct, ss, coins, status, scratch, s);
  });
}

hipError_t mlkem_decaps_keyed(const AlgInfo& a, const MlkemKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ss,
                              const uint8_t* ct, int32_t* status, void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  return mlkem::with_rank(a.k, [&](auto rank) {
    return mlkem::decaps_impl<decltype(rank)::value>(ks, n, key_index, ss, ct, status, scratch, s);
  });
}

}  // namespace qrk
