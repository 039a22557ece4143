// ML-KEM (FIPS 203), the batched path: the multi-role schedule for n > QRK_SMALL_MAX -- per-handshake
// sponge fronts, SampleNTT and PRF lanes, the three 16-lane polynomial cores, the roles and
// k_multi / k_role -- and mlkem::CtxState, the per-context state its SampleNTT fix-up counters (and
// the single-shot KeyGens' flag words) live in.  Part of the translation unit mlkem.hip; a tool that
// includes this file alone supplies mlkem_small_max() and the three mlkem_kg_*() sizes CtxState uses.
#pragma once
#include <vector>

#include "keccak_pair.cuh"
#include "mlkem_coop.cuh"
#include "mlkem_paths.h"
#include "mlkem_poly.cuh"
#include "mlkem_sample.cuh"

namespace qrk {
namespace mlkem {

// KeyGen front: (rho, sigma) = G(d || k).  rho -> pk[384k..] and dk's ek copy; sigma -> seeds.
template <int K>
__device__ __forceinline__ void front_keygen_hs(const uint8_t* __restrict__ coins, size_t hs, uint8_t* __restrict__ pk,
                                                uint8_t* __restrict__ sk, uint64_t* __restrict__ seeds,
                                                uint64_t* __restrict__ rho) {
  const uint64_t* d = (const uint64_t*)(coins + hs * 64);
  KState s;
  kzero(s);
#pragma unroll
  for (int w = 0; w < 4; ++w) kxor(s, w, d[w]);
  s.a[4].lo ^= (uint32_t)K | (DS_SHA3 << 8);
  s.a[RW_SHA3_512 - 1].hi ^= 0x80000000u;
  keccak_f(s);
  uint64_t* rho_pk = (uint64_t*)(pk + hs * P<K>::PK + 384 * K);
  uint64_t* rho_sk = (uint64_t*)(sk + hs * P<K>::SK + 768 * K);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    rho_pk[w] = kword(s, w);
    rho_sk[w] = kword(s, w);
    seeds[hs * 4 + w] = kword(s, 4 + w);
    if (rho) rho[hs * 4 + w] = kword(s, w);
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_front_keygen(const uint8_t* __restrict__ coins, size_t n,
                                                      uint8_t* __restrict__ pk, uint8_t* __restrict__ sk,
                                                      uint64_t* __restrict__ seeds, uint64_t* __restrict__ rho,
                                                      uint32_t* __restrict__ nfix) {
  const size_t hs = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (hs == 0) *nfix = 0;  // the SampleNTT fix-up counter (no memset launch)
  if (hs < n) front_keygen_hs<K>(coins, hs, pk, sk, seeds, rho);
}

// KeyGen back: dk = dk_pke || ek || H(ek) || z  (ek already copied by the core kernel)
template <int K>
__device__ __forceinline__ void back_keygen_hs(const uint8_t* __restrict__ coins, size_t hs,
                                               const uint8_t* __restrict__ pk, uint8_t* __restrict__ sk) {
  const uint64_t* ek = (const uint64_t*)(pk + hs * P<K>::PK);
  KState s;
  kzero(s);
  absorb_words<RW_SHA3_256, P<K>::PK / 8, DS_SHA3>(s, [&](int w) { return ek[w]; });
  uint64_t* tail = (uint64_t*)(sk + hs * P<K>::SK + 768 * K + 32);
  const uint64_t* z = (const uint64_t*)(coins + hs * 64 + 32);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    tail[w] = kword(s, w);
    tail[4 + w] = z[w];
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_back_keygen(const uint8_t* __restrict__ coins, size_t n,
                                                     const uint8_t* __restrict__ pk, uint8_t* __restrict__ sk) {
  const size_t hs = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (hs < n) back_keygen_hs<K>(coins, hs, pk, sk);
}

// Encaps front: (K, r) = G(m || H(ek)); K -> ss, r -> seeds
template <int K>
__device__ __forceinline__ void front_encaps_hs(const uint8_t* __restrict__ pk, const uint8_t* __restrict__ coins,
                                                size_t hs, uint8_t* __restrict__ ss, uint64_t* __restrict__ seeds) {
  const uint64_t* ek = (const uint64_t*)(pk + hs * P<K>::PK);
  KState s;
  kzero(s);
  absorb_words<RW_SHA3_256, P<K>::PK / 8, DS_SHA3, false>(s, [&](int w) { return ek[w]; });
  uint64_t h[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) h[w] = kword(s, w);
  const uint64_t* m = (const uint64_t*)(coins + hs * 32);
  kzero(s);
  absorb_words<RW_SHA3_512, 8, DS_SHA3>(s, [&](int w) { return w < 4 ? m[w] : h[w - 4]; });
  uint64_t* K_out = (uint64_t*)(ss + hs * 32);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    K_out[w] = kword(s, w);
    seeds[hs * 4 + w] = kword(s, 4 + w);
  }
}

// Decaps front: (K', r') = G(m' || h), Kbar = J(z || c)
template <int K>
__device__ __forceinline__ void g_decaps_hs(const uint8_t* __restrict__ sk, const uint64_t* __restrict__ mprime,
                                            size_t hs, uint64_t* __restrict__ seeds, uint64_t* __restrict__ kprime) {
  const uint64_t* h = (const uint64_t*)(sk + hs * P<K>::SK + 768 * K + 32);
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
template <int K>
__device__ __forceinline__ void j_decaps_hs(const uint8_t* __restrict__ ct, const uint8_t* __restrict__ sk, size_t hs,
                                            uint64_t* __restrict__ kbar) {
  const uint64_t* z = (const uint64_t*)(sk + hs * P<K>::SK + 768 * K + 64);
  const uint64_t* c = (const uint64_t*)(ct + hs * P<K>::CT);
  KState s;
  kzero(s);
  absorb_words<RW_SHAKE256, 4 + P<K>::CT / 8, DS_SHAKE, false>(s, [&](int w) { return w < 4 ? z[w] : c[w - 4]; });
#pragma unroll
  for (int w = 0; w < 4; ++w) kbar[hs * 4 + w] = kword(s, w);
}

// The Encaps front and G(m' || h) on a lane pair (keccak_pair.cuh: the even lane holds the low
// halves of the state words, the odd lane the high halves) for chunks of at most QRK_PAIR_FRONT_MAX
// handshakes: there the front's lane-per-handshake waves (one per SIMD at 2^14 handshakes) are the
// critical path of their launch (2^14: +8.8 %, 2^15: +1.5 %, profiles/r5/pair_fronts/).  (J on pairs
// lost: see decaps_impl.)  `half` = lane & 1, hm = all-ones on the odd lane.
template <int K>
__device__ __forceinline__ void front_encaps_pair(const uint8_t* __restrict__ pk, const uint8_t* __restrict__ coins,
                                                  size_t hs, int half, uint32_t hm, uint8_t* __restrict__ ss,
                                                  uint64_t* __restrict__ seeds) {
  const uint32_t* ek = (const uint32_t*)(pk + hs * P<K>::PK);
  PState s;
  pzero(s);
  pabsorb<RW_SHA3_256, P<K>::PK / 8, DS_SHA3>(s, hm, [&](int w) { return ek[2 * w + half]; });
  uint32_t h[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) h[w] = s.a[w];
  const uint32_t* m = (const uint32_t*)(coins + hs * 32);
  pzero(s);
  pabsorb<RW_SHA3_512, 8, DS_SHA3>(s, hm, [&](int w) { return w < 4 ? m[2 * w + half] : h[w - 4]; });
  uint32_t* k_out = (uint32_t*)(ss + hs * 32);
  uint32_t* r_out = (uint32_t*)(seeds + hs * 4);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    k_out[2 * w + half] = s.a[w];
    r_out[2 * w + half] = s.a[4 + w];
  }
}
template <int K>
__device__ __forceinline__ void g_decaps_pair(const uint8_t* __restrict__ sk, const uint64_t* __restrict__ mprime,
                                              size_t hs, int half, uint32_t hm, uint64_t* __restrict__ seeds,
                                              uint64_t* __restrict__ kprime) {
  const uint32_t* h = (const uint32_t*)(sk + hs * P<K>::SK + 768 * K + 32);
  const uint32_t* m = (const uint32_t*)(mprime + hs * 4);
  PState s;
  pzero(s);
  pabsorb<RW_SHA3_512, 8, DS_SHA3>(s, hm, [&](int w) { return w < 4 ? m[2 * w + half] : h[2 * (w - 4) + half]; });
  uint32_t* kp = (uint32_t*)(kprime + hs * 4);
  uint32_t* sd = (uint32_t*)(seeds + hs * 4);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    kp[2 * w + half] = s.a[w];
    sd[2 * w + half] = s.a[4 + w];
  }
}

// k_xof reads rho from a compact copy (32 B per handshake) instead of the
// keys themselves.  Its K^2 lanes per handshake sit in K^2 different waves, and each wave's 64
// rho reads at the key stride (1184 B for ML-KEM-768) touch 64 cache lines: rocprofv3 counts
// 1.2 GB of reads per 2^20-handshake k_xof launch for 33 MB of rho
// (profiles/r3/rocprof_mlkem768_b20_r3b.json).  The copy is one 32-B read per handshake.
// It also zeroes the SampleNTT fix-up counter the next kernel counts into (no memset launch).
__global__ __launch_bounds__(256) void k_rho_copy(const uint8_t* __restrict__ base, size_t stride, size_t n,
                                                  uint64_t* __restrict__ out, uint32_t* __restrict__ nfix) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;  // one thread per word
  if (t == 0) *nfix = 0;
  if (t >= 4 * n) return;
  out[t] = ((const uint64_t*)(base + (t >> 2) * stride))[t & 3];
}
// The same copy for a Decaps chunk whose KeyGen's matrix the context kept, with the match pass folded in:
// a row matches where the rho in its dk equals tags[row], the rho KeyGen stored beside the row's kept
// entries (rows below kept_rows; any row beyond them, a permuted row or a key from elsewhere misses), and
// hit[row] = 1 where all four rows of its aligned quad match.  The quad is what one wave of the
// re-encryption core holds (16 lanes per handshake), so the core's choice of matrix is wave-uniform and
// its base stays in scalar registers; a row that matched in a quad that missed is sampled like its
// neighbours, which is always right.  rho is public, so the compare may be what it is.  Four lanes per
// row, a quad's sixteen in one wave.
__global__ __launch_bounds__(256) void k_rho_match(const uint8_t* __restrict__ base, size_t stride, size_t n,
                                                   const uint64_t* __restrict__ tags, size_t kept_rows,
                                                   uint64_t* __restrict__ out, uint32_t* __restrict__ hit,
                                                   uint32_t* __restrict__ nfix) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;  // one thread per word
  if (t == 0) *nfix = 0;
  const size_t row = t >> 2;
  bool eq = false;
  if (row < n) {
    const uint64_t w = ((const uint64_t*)(base + row * stride))[t & 3];
    out[t] = w;
    if (row < kept_rows) eq = w == tags[t];
  }
  const uint64_t m = __ballot(eq);
  if (row < n && (t & 3) == 0) hit[row] = ((m >> (threadIdx.x & 48)) & 0xFFFF) == 0xFFFF;
}

// ------------------------------------------------------------ KeyGen core
// s_hat = NTT(CBD(PRF(sigma, j))), e_hat = NTT(CBD(PRF(sigma, k+i))),
// t_hat_i = sum_j A[i][j] o s_hat_j + e_hat_i   (A[i][j] = SampleNTT(rho || j || i))
template <int K>
__device__ __forceinline__ void keygen_core_hs(size_t n, size_t C, const uint64_t* __restrict__ xof,
                                                     const uint64_t* __restrict__ prf, uint8_t* __restrict__ pk,
                                                     uint8_t* __restrict__ sk, size_t hs_raw, int L, GroupLds& g) {
  const bool active = hs_raw < n;
  const size_t hs = active ? hs_raw : n - 1;  // index in the chunk
  uint8_t* ek = pk + hs * P<K>::PK;
  uint8_t* dk = sk + hs * P<K>::SK;
  BOp sb[K];
  {
    CbdRaw sr[K];  // every s_j's CBD words issued before the first NTT
#pragma unroll
    for (int j = 0; j < K; ++j) sr[j] = cbd_load<P<K>::ETA1, 64>(prf, (size_t)j * C + hs, L);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      PF16 f;
      cbd_f<P<K>::ETA1>(f, sr[j]);
      contig_to_stride_f(f, (float*)g.poly, L);
      ntt_fwd_f<false>(f, (float*)g.poly, L);
      sb[j] = make_bop_f(f, L);
      P16 t;
#pragma unroll
      for (int x = 0; x < 16; ++x) t.v[x] = canon_f(f.v[x]);
      if (active) encode12(t, dk + 384 * j, L);
    }
  }
  // row i's matrix entries and e_i's CBD words are loaded one row ahead
  PK8 an[K];
#pragma unroll
  for (int j = 0; j < K; ++j) an[j] = LOAD_XOF(64, (size_t)(j * K) * C + hs);
  CbdRaw er = cbd_load<P<K>::ETA1, 64>(prf, (size_t)K * C + hs, L);
#pragma unroll 1
  for (int i = 0; i < K; ++i) {
    int acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) basemul_acc(acc, an[j], sb[j]);
    const CbdRaw ecur = er;
    if (i + 1 < K) {
#pragma unroll
      for (int j = 0; j < K; ++j) an[j] = LOAD_XOF(64, (size_t)(j * K + i + 1) * C + hs);
      er = cbd_load<P<K>::ETA1, 64>(prf, (size_t)(K + i + 1) * C + hs, L);
    }
    PF16 ef;
    cbd_f<P<K>::ETA1>(ef, ecur);
    contig_to_stride_f(ef, (float*)g.poly, L);
    ntt_fwd_f<false>(ef, (float*)g.poly, L);
    P16 t;
#pragma unroll
    for (int x = 0; x < 16; ++x) t.v[x] = canon_f(acc_to_f(acc[x]) + ef.v[x]);
    if (active) {
      encode12(t, ek + 384 * i, L);
      encode12(t, dk + 384 * K + 384 * i, L);
    }
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_keygen_core(size_t n, size_t C, const uint64_t* __restrict__ xof,
                                                     const uint64_t* __restrict__ prf, uint8_t* __restrict__ pk,
                                                     uint8_t* __restrict__ sk) {
  __shared__ GroupLds lds[GROUPS];
  const int gi = threadIdx.x >> 4;
  keygen_core_hs<K>(n, C, xof, prf, pk, sk, (size_t)blockIdx.x * GROUPS + gi, threadIdx.x & 15, lds[gi]);
}

// ------------------------------------------------------------ K-PKE.Encrypt core
// MODE 0 (encaps): write c.  MODE 1 (decaps): compare c' with the input c and
// select K' or Kbar in constant time (FIPS 203 Alg. 18 lines 9-11).
// MODE 1 with hit != NULL (a chunk whose KeyGen's matrix the context kept): a wave whose handshakes' hit
// word is set reads its matrix entries from xof_kept, the others from xof (k_rho_match; rho is public).
template <int K, int MODE>
__device__ __forceinline__ void encrypt_core_hs(size_t n, size_t C, const uint64_t* __restrict__ xof_own,
                                                      const uint64_t* __restrict__ prf,
                                                      const uint8_t* __restrict__ ek_base, size_t ek_stride,
                                                      const uint8_t* __restrict__ m_base, size_t m_stride,
                                                      uint8_t* __restrict__ ct, int32_t* __restrict__ status,
                                                      const uint64_t* __restrict__ kprime,
                                                      const uint64_t* __restrict__ kbar, uint8_t* __restrict__ ss,
                                                      const uint64_t* __restrict__ xof_kept,
                                                      const uint32_t* __restrict__ hit, size_t hs_raw, int L,
                                                      GroupLds& g) {
  constexpr int DU = P<K>::DU, DV = P<K>::DV;
  const bool active = hs_raw < n;
  const size_t hs = active ? hs_raw : n - 1;  // index in the chunk
  const uint64_t* xof = xof_own;
  if constexpr (MODE == 1) {
    // the four handshakes of a wave are one quad of k_rho_match (a clamped lane's hs is in the quad or
    // the whole wave is clamped to n - 1): one value per wave
    if (hit && __builtin_amdgcn_readfirstlane(hit[hs])) xof = xof_kept;
  }
  const uint8_t* ek = ek_base + hs * ek_stride;
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
  // u_i = NTT^-1(sum_j A[j][i] o y_j) + e1_i ;  A[j][i] = SampleNTT(rho || i || j).
  // Row i+1's matrix entries and the next CBD words are loaded one row ahead (latency hidden
  // inside the wave; loading each entry as the basemul needs it, at 4 waves / SIMD, was slower).
  // Issuing the first row's entries before the K NTT(y_j) instead was 3 % slower
  // (profiles/r3/ab_core_arith_c.jsonl).
  PK8 an[K];
#pragma unroll
  for (int j = 0; j < K; ++j) an[j] = LOAD_XOF(64, (size_t)j * C + hs);
  CbdRaw er = cbd_load<P<K>::ETA2, 64>(prf, (size_t)K * C + hs, L);
  // one u-row; LAST: the final row (peeled, so its prefetch is t_hat's words: the core waited on
  // memory 25-29 % of its wave time before, profiles/r2/sq_mlkem768_b20_r2b.txt)
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
        for (int j = 0; j < K; ++j) an[j] = LOAD_XOF(64, (size_t)((i + 1) * K + j) * C + hs);
      }
    } else {
      // last row: the matrix registers are free, so t_hat's 24 bytes per lane and row (for v
      // below) are loaded into them here, one row's NTT^-1 ahead of their use
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const uint2* e = (const uint2*)(ek + 384 * j + 24 * L);
        const uint2 a = e[0], b = e[1], c = e[2];
        an[j].w[0] = a.x, an[j].w[1] = a.y, an[j].w[2] = b.x, an[j].w[3] = b.y, an[j].w[4] = c.x, an[j].w[5] = c.y;
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
      flush_bits<DU>(g, c + 32 * DU * i, nullptr, diff, active, L);
  };
#pragma unroll 1
  for (int i = 0; i < K - 1; ++i) row(i, std::false_type{});
  row(K - 1, std::true_type{});
  // v = NTT^-1(t_hat^T o y_hat) + e2 + Decompress_1(m)
  {
    int acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint32_t w[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) w[t] = an[j].w[t];
      const uint64_t a = ((uint64_t)w[1] << 32) | w[0], b = ((uint64_t)w[3] << 32) | w[2],
                     c = ((uint64_t)w[5] << 32) | w[4];
      basemul_acc(acc, decode12_w(a, b, c, bad), yb[j]);
    }
    PF16 vf;
#pragma unroll
    for (int t = 0; t < 16; ++t) vf.v[t] = acc_to_f(acc[t]);
    ntt_inv_f(vf, (float*)g.poly, L);
    stride_to_contig_f(vf, (float*)g.poly, L);
    PF16 ef;
    cbd_f<P<K>::ETA2>(ef, er);  // e2
    const uint8_t* m = m_base + hs * m_stride;
    const uint32_t mb = (uint32_t)m[2 * L] | ((uint32_t)m[2 * L + 1] << 8);
    P16 v;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float mu = ((mb >> t) & 1) ? (float)((Q + 1) / 2) : 0.0f;
      v.v[t] = compress_f<DV>(vf.v[t] + ef.v[t] + mu);
    }
    pack_bits<DV>(v, g, L);
    flush_bits<DV>(g, c + 32 * DU * K, MODE ? c + 32 * DU * K : nullptr, diff, active, L);
    if (MODE == 0 && status) {
      const uint32_t anybad = group_or(bad ? 1u : 0u);
      if (active && L == 0) status[hs] = anybad ? -1 : 0;
    }
  }
  if (MODE == 1) {
    // constant-time select: ss = (c == c') ? K' : Kbar
    const uint32_t d = group_or(diff);
    const uint32_t mask = (uint32_t)(((uint64_t)d - 1u) >> 32);  // all-ones iff d == 0, no branch
    if (L < 8) {
      const uint32_t kp = ((const uint32_t*)(kprime + hs * 4))[L];
      const uint32_t kb = ((const uint32_t*)(kbar + hs * 4))[L];
      if (active) ((uint32_t*)(ss + hs * 32))[L] = (kp & mask) | (kb & ~mask);
    }
  }
}

// ============================================================ multi-role launches
// Every kernel of a call runs on the caller's stream.  Kernels of one operation that do not depend
// on each other share one launch instead of running on side streams: a multi-role kernel
// (k_multi<A, B, ...>) whose first nb_A workgroups run role A, the next nb_B role B, and so on.
// The dispatcher hands out workgroups in grid order, so the first role is resident from the start
// and the later roles fill the CUs around it and after it.  The first role is the latency-bound
// one: a lane-per-handshake sponge (one wave per SIMD at 2^16 handshakes) or the SampleNTT fix-up
// (~0.7 % of the entries, 4+ sequential permutations per lane), and the throughput-bound
// SampleNTT / PRF waves behind it keep the chip full while it runs (tools/fuse_probe.hip,
// profiles/r4/schedule_probe/: at 2^16 Encaps 0.518 -> 0.475 ms, Decaps 0.598 -> 0.535 ms per
// call).  A role must not use workgroup barriers (its workgroups may share a CU with another
// role's) -- the roles below synchronise at most within a wave.

// xof_coop_place (mlkem_coop.cuh) into the batched layout (the SampleNTT fix-up for small chunks, one wave per listed entry
// inst = xy C + hs): the 256 values in FIPS order in the wave's LDS buffer cb, then lanes 0-31
// pack one 8-coefficient chunk each into the entry's 12-bit tiles, as k_xof would have
template <int K>
__device__ __forceinline__ void xof_fix_coop(const uint8_t* __restrict__ rho_base, size_t rho_stride, size_t C,
                                             uint32_t inst, XUnit* __restrict__ out, uint16_t* __restrict__ cb,
                                             uint32_t* __restrict__ pbuf, const Coop& c) {
  const size_t hs = inst % C;
  xof_coop_place<K>((const uint64_t*)(rho_base + hs * rho_stride), (int)(inst / C), pbuf, c,
                    [&](int j, uint32_t d) { cb[j] = (uint16_t)d; });
  const int lane = threadIdx.x & 63;
  if (lane < 32) {
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = cb[8 * lane + j];
    chunk_store(xc<XTW>(xent<XTW>(out, inst), lane), r);
  }
  wave_phase();  // cb is read before the next entry's values are placed
}

template <int K, bool FIX>
struct RXof {  // SampleNTT, lane / matrix entry (FIX: the fix-up list, grid-stride over nb blocks)
  static constexpr int LDS = XOF_LDS, WPE = 1;
  XofArgs<K, FIX> a;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char* lds) const { xof_body<K, FIX>(a, vb, nb, (uint32_t*)lds); }
};
// The fix-up list on one wave per entry (small chunks): the wave-cooperative sponge (~2.7 us per
// permutation) instead of one lane's (~9 us on a lone wave), so the 4+ dependent permutations of an
// entry stop being the critical path of the launch
template <int K>
struct RXofFixCoop {
  static constexpr int WAVE_LDS = 512 + 44 * 4;  // 256 placed values (u16) + the parse buffer
  static constexpr int LDS = 4 * WAVE_LDS, WPE = 1;
  XofArgs<K, true> a;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char* lds) const {
    const int wave = threadIdx.x >> 6;
    char* w = lds + wave * WAVE_LDS;
    const Coop c = coop_init();
    const uint32_t limit = *a.nfix;
#pragma unroll 1
    for (uint32_t r = vb * 4 + wave; r < limit; r += nb * 4)  // wave-uniform
      xof_fix_coop<K>(a.rho_base, a.rho_stride, a.C, a.fix[r], a.out, (uint16_t*)w, (uint32_t*)(w + 512), c);
  }
};
template <int K>
struct RFrontEnc {  // (K, r) = G(m || H(ek)), lane / handshake
  static constexpr int LDS = 0, WPE = 1;
  const uint8_t *pk, *coins;
  size_t n;
  uint8_t* ss;
  uint64_t* seeds;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t hs = (size_t)vb * 256 + threadIdx.x;
    if (hs < n) front_encaps_hs<K>(pk, coins, hs, ss, seeds);
  }
};
template <int K>
struct RJDec {  // Kbar = J(z || c), lane / handshake: needs only the inputs
  static constexpr int LDS = 0, WPE = 1;
  const uint8_t *ct, *sk;
  size_t n;
  uint64_t* kbar;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t hs = (size_t)vb * 256 + threadIdx.x;
    if (hs < n) j_decaps_hs<K>(ct, sk, hs, kbar);
  }
};
// lane-pair forms of two sponge roles (keccak_pair.cuh), 128 handshakes per workgroup
#ifndef QRK_PAIR_FRONT_MAX
#define QRK_PAIR_FRONT_MAX (1 << 15)
#endif
struct PairLane {
  size_t hs;
  int half;
  uint32_t hm;
};
__device__ __forceinline__ PairLane pair_lane(unsigned vb) {
  const size_t t = (size_t)vb * 256 + threadIdx.x;
  const int half = (int)(t & 1);
  return {t >> 1, half, half ? 0xFFFFFFFFu : 0u};
}
template <int K>
struct RFrontEncPair {
  static constexpr int LDS = 0, WPE = 1;
  const uint8_t *pk, *coins;
  size_t n;
  uint8_t* ss;
  uint64_t* seeds;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const PairLane p = pair_lane(vb);
    if (p.hs < n) front_encaps_pair<K>(pk, coins, p.hs, p.half, p.hm, ss, seeds);
  }
};
template <int K>
struct RGDecPair {
  static constexpr int LDS = 0, WPE = 1;
  const uint8_t* sk;
  const uint64_t* mprime;
  size_t n;
  uint64_t *seeds, *kprime;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const PairLane p = pair_lane(vb);
    if (p.hs < n) g_decaps_pair<K>(sk, mprime, p.hs, p.half, p.hm, seeds, kprime);
  }
};
template <int K>
struct RGDec {  // (K', r') = G(m' || h), lane / handshake
  static constexpr int LDS = 0, WPE = 1;
  const uint8_t* sk;
  const uint64_t* mprime;
  size_t n;
  uint64_t *seeds, *kprime;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char*) const {
    const size_t hs = (size_t)vb * 256 + threadIdx.x;
    if (hs < n) g_decaps_hs<K>(sk, mprime, hs, seeds, kprime);
  }
};
template <int ETA1, int ETA2>
struct RPrf {  // PRF_eta(seed, N), lane / (N, handshake)
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
template <int K>
struct RDecrypt {  // m' = K-PKE.Decrypt(dk, c), 16 lanes / handshake
  static constexpr int LDS = GROUPS * (int)sizeof(GroupLds), WPE = 1;
  size_t n;
  const uint8_t *ct, *sk;
  uint64_t* mprime;
  unsigned nb;
  __device__ __forceinline__ void run(unsigned vb, char* lds) const {
    const int gi = threadIdx.x >> 4;
    decrypt_core_hs<K>(n, ct, sk, mprime, (size_t)vb * GROUPS + gi, threadIdx.x & 15, ((GroupLds*)lds)[gi]);
  }
};

// Waves per SIMD the core is compiled for: 3 (<= 168 VGPRs).  ML-KEM-1024's Decaps core spills at
// 168 (16 B) and takes a scratch allocation that slowed the launch after it, so it keeps its 176
// VGPRs (2 waves); its Encaps core fits 168 without spilling: 3.05 -> 2.77 ms per 2^20 core launch
// (both cores at 3 waves, profiles/r6/core4/).
template <int K, int MODE>
struct RCore {  // K-PKE.Encrypt (MODE 1: the Decaps re-encryption, compare and select), 16 lanes / hs
  static constexpr int LDS = GROUPS * (int)sizeof(GroupLds), WPE = (K == 4 && MODE == 1) ? 1 : 3;
  size_t n, C;
  const uint64_t *xof, *prf;
  const uint8_t* ek;
  size_t ek_stride;
  const uint8_t* m_base;
  size_t m_stride;
  uint8_t* ct;
  int32_t* status;
  const uint64_t *kprime, *kbar;
  uint8_t* ss;
  unsigned nb;
  const uint64_t* xof_kept = nullptr;  // MODE 1: the kept matrix and the per-handshake hit words
  const uint32_t* hit = nullptr;       // (k_rho_match), NULL: every handshake reads xof
  __device__ __forceinline__ void run(unsigned vb, char* lds) const {
    const int gi = threadIdx.x >> 4;
    encrypt_core_hs<K, MODE>(n, C, xof, prf, ek, ek_stride, m_base, m_stride, ct, status, kprime, kbar, ss,
                             xof_kept, hit, (size_t)vb * GROUPS + gi, threadIdx.x & 15, ((GroupLds*)lds)[gi]);
  }
};

constexpr int max_of(int a, int b) { return a > b ? a : b; }
template <class... R>
struct Roles {
  static constexpr int LDS = 0, WPE = 1;
};
template <class R0, class... R>
struct Roles<R0, R...> {
  static constexpr int LDS = max_of(R0::LDS, Roles<R...>::LDS), WPE = max_of(R0::WPE, Roles<R...>::WPE);
};
// roles in grid order: workgroup w runs role i with w - (nb_0 + ... + nb_{i-1}) as its block index
template <class... R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Roles<R...>::WPE))) void k_multi(R... r) {
  constexpr int L = Roles<R...>::LDS;
  __shared__ __attribute__((aligned(16))) char lds[L > 16 ? L : 16];
  unsigned w = blockIdx.x;
  bool ran = false;
  ((ran = ran || (w < r.nb ? (r.run(w, lds), true) : (w -= r.nb, false))), ...);
}
template <class R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R::WPE))) void k_role(R r) {
  constexpr int L = R::LDS;
  __shared__ __attribute__((aligned(16))) char lds[L > 16 ? L : 16];
  r.run(blockIdx.x, lds);
}

// ============================================================ host launchers

// independent kernels of one operation: one multi-role launch (roles in grid order), or (serial
// schedule) one launch each in that order -- the per-kernel timings in isolation.  `name` joins
// the kernel names with '+'.
template <class R>
void launch_one(const char* name, const R& r, const Streams& s) {
  if (r.nb) QRK_LAUNCH(name, s.main, k_role<R>, dim3(r.nb), dim3(256), 0, s.main, r);
}
template <class... R>
void launch_multi(const char* name, std::initializer_list<const char*> names, const Streams& s, const R&... r) {
  hipStream_t st = s.main;
  if (names.size() != sizeof...(R)) {  // one name per role (a launcher bug, not an input error)
    qrk_chk(hipErrorInvalidValue);
    return;
  }
  if (s.serial) {
    const char* const* nm = names.begin();
    (launch_one(*nm++, r, s), ...);
    return;
  }
  const unsigned nb = (0u + ... + r.nb);
  if (nb) QRK_LAUNCH(name, st, (k_multi<R...>), dim3(nb), dim3(256), 0, st, r...);
}

// SampleNTT roles for a chunk of C handshakes (n used): the main pass and its fix-up.  The fix-up
// covers fix-up rates up to 1/64 (~0.7 % expected) in a single pass, one lane per listed entry:
// it is latency-bound (4+ sequential permutations per lane), a second grid-stride pass would double it.
// Where SampleNTT reads rho and counts its fix-up entries: the compact copy in scratch and the
// scratch counter (k_rho_copy zeroes it), or -- chunks <= DIRECT_RHO_MAX -- rho in the keys
// themselves and one of the context's two fix-up counters (Streams::fixc), the main pass zeroing
// the other one for the next call: no k_rho_copy launch.
struct RhoSrc {
  const uint8_t* base;
  size_t stride;
  uint32_t *nfix, *zero_other;
};
template <int K>
RXof<K, false> xof_role(const RhoSrc& r, size_t n, size_t C, const ScratchView& v) {
  return {{r.base, r.stride, n, C, (XUnit*)v.xof, v.fix, r.nfix, r.zero_other}, blocks_for((size_t)K * K * C)};
}
template <int K>
RXof<K, true> fix_role(const RhoSrc& r, size_t n, size_t C, const ScratchView& v) {
  return {{r.base, r.stride, n, C, (XUnit*)v.xof, v.fix, r.nfix, nullptr},
          (unsigned)std::min<size_t>((size_t)K * K * C / (64 * 256) + 1, 4096)};
}
template <int K>
RXof<K, false> xof_role(const uint8_t* rho, size_t n, size_t C, const ScratchView& v) {
  return xof_role<K>(RhoSrc{rho, 32, v.nfix, nullptr}, n, C, v);
}
template <int K>
RXof<K, true> fix_role(const uint8_t* rho, size_t n, size_t C, const ScratchView& v) {
  return fix_role<K>(RhoSrc{rho, 32, v.nfix, nullptr}, n, C, v);
}
// chunks up to this size run the fix-up one wave per entry (RXofFixCoop): below it the
// lane-per-entry fix-up's latency shows past the PRFs it shares a launch with, above it the
// cooperative form's issue slots (~4x per entry) cost more.  Same-box A/Bs against the lane form
// (profiles/r4/schedule_ab/abx_2p1*_coop_fixup.jsonl): 2^13 +24.8 %, 2^14 +15.8 %, 2^15 +4.5 %,
// 2^16 -3.1 %, 2^17 -4.2 %.
constexpr size_t COOP_FIX_MAX = (size_t)1 << 15;
template <int K>
RXofFixCoop<K> fix_coop_role(const RhoSrc& r, size_t n, size_t C, const ScratchView& v) {
  return {{r.base, r.stride, n, C, (XUnit*)v.xof, v.fix, r.nfix, nullptr},
          (unsigned)std::min<size_t>((size_t)K * K * C / 256 + 1, 4096)};  // waves for 1/64 of the entries
}
// {SampleNTT fix-up, PRFs}: the fix-up's workgroups first (grid order)
template <int K, class Prf>
void launch_fix_prf(const RhoSrc& r, size_t n, size_t C, const ScratchView& v, const Prf& prf, const Streams& s) {
  if (C <= COOP_FIX_MAX)
    launch_multi("k_xof_fix+k_prf", {"k_xof_fix", "k_prf"}, s, fix_coop_role<K>(r, n, C, v), prf);
  else
    launch_multi("k_xof_fix+k_prf", {"k_xof_fix", "k_prf"}, s, fix_role<K>(r, n, C, v), prf);
}
template <int K, class Prf>
void launch_fix_prf(const uint8_t* rho, size_t n, size_t C, const ScratchView& v, const Prf& prf, const Streams& s) {
  launch_fix_prf<K>(RhoSrc{rho, 32, v.nfix, nullptr}, n, C, v, prf, s);
}

// Chunks up to this size read rho straight from the keys: there the k_rho_copy launch (~5 us,
// launch-bound) costs more than the strided rho reads it saves (64 cache lines per wave instead of
// 16; at 2^20 handshakes those reads were 1.2 GB per k_xof launch, see k_rho_copy).
constexpr size_t DIRECT_RHO_MAX = (size_t)1 << 15;

// ------------------------------------------------------------ per-context state (CtxState, qrkem_internal.h)
// What CtxState guarantees, and the only code that touches its fields:
//  - Streams::fixc / fixp are set by prepare() alone, and point at two device words that are both zero
//    when the call's first chunk starts, unless an earlier chunk of this context failed after its
//    parity flip (rho_source, below) -- then chunk_failed() marked the pair and prepare() queues the
//    re-zero of both words on the call's stream, ahead of its first launch.  A chunk that succeeds
//    leaves the word the next chunk counts into zero (its main pass zeroes it).
//  - Streams::kg_cnt is set by prepare() alone, and points at flag / counter words that are zero between
//    calls: the single-shot KeyGen kernels reset what they set, and after a failed k_keygen_pipe call
//    (a straggler may store after the collector's reset and wipe) keygen_failed() re-zeroes them and
//    the head of the scratch at once, or, if that fails, prepare() does before the next KeyGen launch.
// Every allocation is made on the first call that needs it.

// the flag words and the head of the scratch the single-shot KeyGen workgroups store to, on `st`
hipError_t CtxState::kg_rezero(void* scratch, size_t scratch_bytes, hipStream_t st) {
  hipError_t e = hipMemsetAsync(kg_cnt, 0, mlkem_kg_flag_words() * sizeof(uint32_t), st);
  if (e == hipSuccess && scratch)
    e = hipMemsetAsync(scratch, 0, std::min(scratch_bytes, mlkem_kg_scratch_bytes()), st);
  return e;
}

hipError_t CtxState::prepare(Streams& S, Op op, size_t n, size_t chunk, void* scratch, size_t scratch_bytes,
                             const char** what) {
  if (op == Op::KEYPAIR && n <= mlkem_kg_multi_max()) {
    if (!kg_cnt) {
      *what = "hipMalloc(kg_cnt)";
      hipError_t e = hipMalloc((void**)&kg_cnt, mlkem_kg_flag_words() * sizeof(uint32_t));
      if (e == hipSuccess) e = hipMemset(kg_cnt, 0, mlkem_kg_flag_words() * sizeof(uint32_t));
      if (e != hipSuccess) return e;
    }
    if (kg_dirty) {  // stream-ordered behind the failed call's kernel
      *what = "hipMemsetAsync(kg_cnt)";
      const hipError_t e = kg_rezero(scratch, scratch_bytes, S.main);
      if (e != hipSuccess) return e;
      kg_dirty = false;
    }
    S.kg_cnt = kg_cnt;
  } else {
    S.kg_err = nullptr;
  }
  if (op != Op::KEYPAIR) {
    if (!fixc) {
      *what = "hipMalloc(fixc)";
      hipError_t e = hipMalloc((void**)&fixc, 2 * sizeof(uint32_t));
      if (e == hipSuccess) e = hipMemset(fixc, 0, 2 * sizeof(uint32_t));
      if (e != hipSuccess) return e;
    }
    if (fixc_dirty) {
      *what = "hipMemsetAsync(fixc)";
      const hipError_t e = hipMemsetAsync(fixc, 0, 2 * sizeof(uint32_t), S.main);
      if (e != hipSuccess) return e;
      fixc_dirty = false;
    }
    S.fixc = fixc;
    S.fixp = &fixp;
  }
  return hipSuccess;
}

void CtxState::chunk_failed(const Streams& S) {
  fixc_dirty = S.fixc != nullptr;  // the counters' zero-between-calls invariant is unknown now
}

void CtxState::keygen_failed(bool pipe_call, void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (pipe_call) kg_dirty = true;  // re-zeroed (flags, scratch) before the next KeyGen launch
  if (kg_dirty && kg_cnt) {
    // wipe the secret scratch a straggler may have written after the collector's wipe now, not at
    // the next KeyGen (prepare re-zeroes again if this fails)
    hipError_t w = kg_rezero(scratch, scratch_bytes, st);
    if (w == hipSuccess) w = hipStreamSynchronize(st);
    if (w == hipSuccess) kg_dirty = false;
  }
}

void CtxState::free() {
  if (kg_cnt) (void)hipFree(kg_cnt);
  if (fixc) (void)hipFree(fixc);
  if (keep) (void)hipFree(keep);
}

// ---- the kept region (qrkem_internal.h: what it is, and the rule that keeps a stale one from being read)
static KeepPlan keep_plan_of(int k, size_t n, size_t chunk, size_t cap_bytes) {
  return mlkem_keep_plan((size_t)k * k * XOF_W * sizeof(uint64_t), n, chunk, mlkem_small_max(), cap_bytes);
}

void CtxState::keep_begin(const AlgInfo& a, size_t n, size_t chunk, size_t cap_bytes, void (*quiesce)(void*),
                          void* arg) {
  keep_valid = false;
  const KeepPlan p = keep_plan_of(a.k, n, chunk, cap_bytes);
  keep_k = a.k, keep_n = n, keep_chunk_rows = chunk, keep_chunks = p.kept;
  if (p.bytes <= keep_bytes) return;
  if (keep) {  // public data: nothing to wipe, but an earlier call may still read it
    quiesce(arg);
    (void)hipFree(keep);
    keep = nullptr, keep_bytes = 0;
  }
  if (hipMalloc((void**)&keep, p.bytes) == hipSuccess) {
    keep_bytes = p.bytes;
  } else {
    (void)hipGetLastError();  // not this call's error: the KeyGen runs as it would without the region
    keep = nullptr, keep_chunks = 0;
  }
}

void CtxState::keep_chunk(Streams& S, size_t idx) const {
  S.xof_keep = S.rho_keep = nullptr;
  if (idx >= keep_chunks) return;
  const KeepPlan p = keep_plan_of(keep_k, keep_n, keep_chunk_rows, (size_t)-1);
  S.rho_keep = (uint64_t*)(keep + idx * p.chunk_bytes);
  S.xof_keep = (uint64_t*)(keep + idx * p.chunk_bytes + p.tag_bytes);
}

void CtxState::keep_commit() { keep_valid = keep_chunks > 0; }

void CtxState::kept_chunk(Streams& S, const AlgInfo& a, size_t chunk, size_t idx, size_t m) const {
  S.xof_kept = S.rho_kept = nullptr;
  S.kept_rows = 0;
  if (!keep_valid || a.k != keep_k || chunk != keep_chunk_rows || idx >= keep_chunks) return;
  // the rows KeyGen's chunk idx held; the tiled layout is a function of round64(rows)
  const size_t rows = std::min(keep_chunk_rows, keep_n - idx * keep_chunk_rows);
  if (m <= mlkem_small_max() || round64(m) != round64(rows)) return;
  const KeepPlan p = keep_plan_of(keep_k, keep_n, keep_chunk_rows, (size_t)-1);
  S.rho_kept = (const uint64_t*)(keep + idx * p.chunk_bytes);
  S.xof_kept = (const uint64_t*)(keep + idx * p.chunk_bytes + p.tag_bytes);
  S.kept_rows = rows;
}

void CtxState::keep_invalidate(void** p, size_t* bytes) {
  keep_valid = false;
  *p = keep, *bytes = keep_bytes;
}

hipError_t CtxState::fix_words(uint32_t* out, int* parity, const char** what) const {
  *what = "hipMemcpy(fixc)";
  out[0] = out[1] = 0;
  *parity = fixp;
  return fixc ? hipMemcpy(out, fixc, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost) : hipSuccess;
}

hipError_t CtxState::kg_flags_residue(uint64_t* out) const {
  *out = 0;
  if (!kg_cnt) return hipSuccess;
  std::vector<uint32_t> tmp(mlkem_kg_flag_words());
  const hipError_t e = hipMemcpy(tmp.data(), kg_cnt, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
  for (uint32_t x : tmp) *out += x != 0;
  return e;
}

// Encaps / Decaps rho source for a chunk of C handshakes: keys_rho = the first key's rho.
inline RhoSrc rho_source(const uint8_t* keys_rho, size_t key_stride, size_t n, size_t C, const ScratchView& v,
                         const Streams& s) {
  if (C <= DIRECT_RHO_MAX && s.fixc && s.fixp) {
    const int p = *s.fixp;
    *s.fixp = p ^ 1;  // the next call counts into the word this call's main pass zeroes
    // tests only: a failure after the flip
    if (g_dbg_fail_after_flip.load(std::memory_order_relaxed)) qrk_chk(hipErrorLaunchFailure);
    return {keys_rho, key_stride, s.fixc + p, s.fixc + (p ^ 1)};
  }
  // k_xof reads rho from the compact copy in scratch
  QRK_LAUNCH("k_rho_copy", s.main, k_rho_copy, dim3(blocks_for(4 * n)), dim3(256), 0, s.main, keys_rho, key_stride,
             n, v.rho, v.nfix);
  return {(const uint8_t*)v.rho, 32, v.nfix, nullptr};
}

// QRK_DEBUG_POISON (environment, tests / tools only): fill the sampled-matrix region with 0xFF
// before a batched Encaps / Decaps, so a read of an entry the call has not written shows up as a
// wrong result instead of reusing the previous call's identical matrix.
inline bool debug_poison() {
  static const bool on = std::getenv("QRK_DEBUG_POISON") != nullptr;
  return on;
}
template <int K>
void poison_xof(size_t C, const ScratchView& v, hipStream_t st) {
  if (debug_poison()) qrk_chk(hipMemsetAsync(v.xof, 0xFF, (size_t)K * K * C * XOF_W * 8, st));
}

// KeyGen: front (rho, sigma) -> SampleNTT -> {SampleNTT fix-up, PRFs} -> t_hat rows -> H(ek)
template <int K>
hipError_t keygen_impl(size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch, const Streams& s) {
  const size_t C = round64(n);
  ScratchView v = carve(scratch, K, C);
  hipStream_t st = s.main;
  // the context keeps A_hat, and each row's rho as its tag, for the same party's Decaps (the front writes
  // the compact rho copy SampleNTT reads: here it is the tags)
  if (s.xof_keep && s.rho_keep) v.xof = s.xof_keep, v.rho = s.rho_keep;
  QRK_LAUNCH("k_front_keygen", st, k_front_keygen<K>, dim3(blocks_for(n)), dim3(256), 0, st, coins, n, pk, sk,
             v.seeds, v.rho, v.nfix);
  const uint8_t* rho = (const uint8_t*)v.rho;
  launch_one("k_xof", xof_role<K>(rho, n, C, v), s);
  launch_fix_prf<K>(rho, n, C, v, RPrf<P<K>::ETA1, P<K>::ETA1>{v.seeds, n, C, 2 * K, 2 * K, v.prf, blocks_for(2 * K * C)},
                    s);
  QRK_LAUNCH("k_keygen_core", st, k_keygen_core<K>, dim3((unsigned)((n + GROUPS - 1) / GROUPS)), dim3(256), 0, st,
             n, C, v.xof, v.prf, pk, sk);
  QRK_LAUNCH("k_back_keygen", st, k_back_keygen<K>, dim3(blocks_for(n)), dim3(256), 0, st, coins, n, pk, sk);
  return launch_status();
}

// Encaps: rho copy -> {G(m || H(ek)), SampleNTT} -> {SampleNTT fix-up, PRFs} -> K-PKE.Encrypt
template <int K>
hipError_t encaps_impl(size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                       int32_t* status, void* scratch, const Streams& s) {
  const size_t C = round64(n);
  ScratchView v = carve(scratch, K, C);
  hipStream_t st = s.main;
  poison_xof<K>(C, v, st);
  const RhoSrc rho = rho_source(pk + 384 * K, (size_t)P<K>::PK, n, C, v, s);
  if (launch_status() != hipSuccess) return launch_status();  // nothing after a failed step
  const RFrontEnc<K> front{pk, coins, n, ss, v.seeds, blocks_for(n)};
  const RPrf<P<K>::ETA1, P<K>::ETA2> prf{v.seeds, n, C, 2 * K + 1, K, v.prf, blocks_for((2 * K + 1) * C)};
  const RCore<K, 0> core{n, C, v.xof, v.prf, pk, (size_t)P<K>::PK, coins, (size_t)32, ct, status, v.kprime, v.kbar,
                         nullptr, (unsigned)((n + GROUPS - 1) / GROUPS)};
  if (C <= QRK_PAIR_FRONT_MAX)
    launch_multi("k_front_encaps+k_xof", {"k_front_encaps", "k_xof"}, s,
                 RFrontEncPair<K>{pk, coins, n, ss, v.seeds, blocks_for(2 * n)}, xof_role<K>(rho, n, C, v));
  else
    launch_multi("k_front_encaps+k_xof", {"k_front_encaps", "k_xof"}, s, front, xof_role<K>(rho, n, C, v));
  launch_fix_prf<K>(rho, n, C, v, prf, s);
  launch_one("k_encrypt_core", core, s);
  return launch_status();
}

// Decaps: rho copy -> {J(z || c), K-PKE.Decrypt, SampleNTT} -> G(m' || h) -> {SampleNTT fix-up, PRFs}
// -> re-encryption with the constant-time compare and select.  Under a kept matrix (s.xof_kept) the rho
// copy is k_rho_match and SampleNTT runs for the rows that missed alone.
template <int K>
hipError_t decaps_impl(size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, void* scratch,
                       const Streams& s) {
  const size_t C = round64(n);
  ScratchView v = carve(scratch, K, C);
  hipStream_t st = s.main;
  const unsigned gblocks = (unsigned)((n + GROUPS - 1) / GROUPS);
  const RDecrypt<K> dec{n, ct, sk, v.mprime, gblocks};
  const RJDec<K> jd{ct, sk, n, v.kbar, blocks_for(n)};
  const RGDec<K> gd{sk, v.mprime, n, v.seeds, v.kprime, blocks_for(n)};
  const RPrf<P<K>::ETA1, P<K>::ETA2> prf{v.seeds, n, C, 2 * K + 1, K, v.prf, blocks_for((2 * K + 1) * C)};
  poison_xof<K>(C, v, st);
  // A_hat from this party's KeyGen on this context (s.xof_kept): the match pass rides on the rho copy, at
  // every chunk size, and the launches below are the usual ones under other names (k_xof_miss: the
  // SampleNTT role's lanes return where their row hit, so a wave whose rows all hit retires at once; only
  // rows that ran reach the fix-up list; the core takes each handshake's matrix base from its hit word).
  // Nothing is read back: which rows hit is known on the device alone.  The same launches serve the caller
  // whose dk buffer is the very one KeyGen wrote: pointer equality would prove nothing the match pass does
  // not establish, and a role of empty workgroups costs microseconds.
  const bool kept = s.xof_kept && s.rho_kept;
  RhoSrc rho;
  if (kept) {
    QRK_LAUNCH("k_rho_match", st, k_rho_match, dim3(blocks_for(4 * n)), dim3(256), 0, st, sk + 768 * K,
               (size_t)P<K>::SK, n, s.rho_kept, s.kept_rows, v.rho, v.hit, v.nfix);
    rho = {(const uint8_t*)v.rho, 32, v.nfix, nullptr};
  } else {
    rho = rho_source(sk + 768 * K, (size_t)P<K>::SK, n, C, v, s);
  }
  if (launch_status() != hipSuccess) return launch_status();  // nothing after a failed step
  RCore<K, 1> core{n, C, v.xof, v.prf, sk + 384 * K, (size_t)P<K>::SK, (const uint8_t*)v.mprime, (size_t)32,
                   const_cast<uint8_t*>(ct), nullptr, v.kprime, v.kbar, ss, gblocks};
  RXof<K, false> xof = xof_role<K>(rho, n, C, v);
  if (kept) core.xof_kept = s.xof_kept, core.hit = xof.a.hit = v.hit;
  // J stays one lane per handshake: at chunks <= 2^15 its launch, {J, decrypt core, SampleNTT}, is
  // throughput-bound, and J on lane pairs (1.3x the issue slots) ran it 105.3 -> 118.7 us at 2^14
  // (47.2e6 against 45.5e6 handshakes/s, profiles/r5/pair_fronts/abx_2p14_pairJ_noJ_off.jsonl); J split
  // over this launch and the next (its last two permutations beside the fix-up and the PRFs) took
  // 4 us off this launch and added 3-14 us to the next: no gain (profiles/r5/mid/)
  if (kept)
    launch_multi("k_j_decaps+k_decrypt_core+k_xof_miss", {"k_j_decaps", "k_decrypt_core", "k_xof_miss"}, s, jd, dec,
                 xof);
  else
    launch_multi("k_j_decaps+k_decrypt_core+k_xof", {"k_j_decaps", "k_decrypt_core", "k_xof"}, s, jd, dec, xof);
  if (C <= QRK_PAIR_FRONT_MAX)
    launch_one("k_g_decaps", RGDecPair<K>{sk, v.mprime, n, v.seeds, v.kprime, blocks_for(2 * n)}, s);
  else
    launch_one("k_g_decaps", gd, s);
  launch_fix_prf<K>(rho, n, C, v, prf, s);
  launch_one("k_encrypt_core", core, s);
  return launch_status();
}

hipError_t keygen_batched(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                          const Streams& s) {
  return with_rank(k, [&](auto rank) { return keygen_impl<decltype(rank)::value>(n, pk, sk, coins, scratch, s); });
}
hipError_t encaps_batched(int k, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                          int32_t* status, void* scratch, const Streams& s) {
  return with_rank(
      k, [&](auto rank) { return encaps_impl<decltype(rank)::value>(n, ct, ss, pk, coins, status, scratch, s); });
}
hipError_t decaps_batched(int k, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, void* scratch,
                          const Streams& s) {
  return with_rank(k, [&](auto rank) { return decaps_impl<decltype(rank)::value>(n, ss, ct, sk, scratch, s); });
}

}  // namespace mlkem

std::atomic<int> g_dbg_fail_after_flip{0};

}  // namespace qrk
