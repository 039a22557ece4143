// ML-KEM (FIPS 203), the one-launch path: k_encaps_one, k_decaps_one, k_keygen_one -- one workgroup
// per handshake, every sponge wave-cooperative.  Part of the translation unit mlkem.hip, for n <= QRK_SMALL_MAX.
#pragma once
#include "mlkem_coop.cuh"
#include "mlkem_paths.h"
#include "mlkem_poly.cuh"
#include "mlkem_trace.cuh"

namespace qrk {
namespace mlkem {

// ============================================================ small batches: one launch per operation
// The reference calls one KeyGen / Encaps / Decaps at a time (key_exchange.py:133, 156, 179):
// there the batched schedule's per-kernel launches dominate, and one handshake's sponge chain is
// the critical path.  For small n one 512-thread workgroup per handshake runs the whole operation
// in a single launch, every sponge wave-cooperative (keccak_coop.cuh, one state per wave):
//   encaps: wave 0 H(ek) then G(m || h);    waves 1-7 the K^2 SampleNTT entries
//   decaps: wave 0 Decrypt then G(m' || h); wave 1 J(z || c);  waves 2-7 SampleNTT
//   keygen: wave 0 G(d || k), then PRFs and SampleNTT over all waves, the core, H(ek)
// then the 2K+1 (2K) PRFs, one per wave, and the 16-lane polynomial core.  SampleNTT entries, PRF
// outputs and the decaps intermediates stay in LDS (the batched layouts at tile width 16, C = 1).
// One launch per operation wins up to 1024 handshakes (ML-KEM-768 encaps+decaps 249 against 346 us
// at 1024, 466 against 396 at 2048: profiles/r2/small_crossover.json)
#ifndef QRK_SMALL_MAX
#define QRK_SMALL_MAX 1024
#endif
constexpr int ONE_WAVES = 12;  // Encaps / Decaps: 3 waves per SIMD, the 16-lane cores fit in 170 VGPRs
constexpr int KG_WAVES = 16;
constexpr int MAX_ONE_WAVES = KG_WAVES > ONE_WAVES ? KG_WAVES : ONE_WAVES;

struct OneLds {
  uint4 xs[32 * 16];             // SampleNTT entries (K^2 <= 16)
  uint64_t ps[PRF_W * 16];       // PRF outputs (2K + 1 <= 9)
  uint32_t bop[4][16][16];       // NTT(y_j) / NTT(s_j) as basemul operands: word w of lane L at [j][w][L]
  float ef[4][16][16];           // KeyGen: NTT(e_i), coefficient t of lane L at [i][t][L]
  uint32_t pbuf[MAX_ONE_WAVES][44];  // per-wave SampleNTT parse buffers
  uint64_t io[600];              // the handshake's inputs (Encaps ek | m, Decaps c | dk; KeyGen ek)
  uint64_t seed[4], mp[4], kp[4], kb[4];
  uint32_t diff[8];              // Decaps compare: per worker group
  int flag_seed, flag_kb, n_ready, n_xof, n_done;
  GroupLds g[8];                 // 16-lane groups: PRF instance N's NTT uses g[N]; rows g[0..K-1], v g[4], Decrypt g[5]
};

// Zero the workgroup's LDS copy of the key material before it exits (LDS is not cleared between
// workgroups); every thread of the workgroup calls it.  With a completion flag (single-shot host
// calls) the outputs are first made visible at system scope, then the flag is stored.
__device__ __forceinline__ void wipe_one(OneLds& sl, uint32_t* done, uint32_t ticket) {
  const int nthreads = (int)blockDim.x;
  if (done) __threadfence_system();
  __syncthreads();
  if (done && threadIdx.x == 0) __hip_atomic_store(done, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  uint4* w = (uint4*)&sl;
  for (int x = threadIdx.x; x < (int)(sizeof(OneLds) / 16); x += nthreads) w[x] = make_uint4(0, 0, 0, 0);
}

// Cross-wave flags (Decaps, where the J chain must not hold a workgroup barrier): a wave's LDS
// writes are released before it bumps a counter; readers spin with an acquiring load.
__device__ __forceinline__ void one_signal(int* p) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(p, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void one_wait(int* p, int target) {
  while (__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Copy one handshake's inputs (host-mapped or device memory) into LDS in one parallel burst: the
// zero-copy single-shot calls then pay one PCIe round trip instead of one per dependent load.
__device__ __forceinline__ void stage_in(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, int words) {
  for (int w = threadIdx.x; w < words; w += (int)blockDim.x) dst[w] = src[w];
}

__device__ __forceinline__ void bop_store(OneLds& sl, int j, const BOp& b, int L) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    sl.bop[j][u][L] = b.b0[u];
    sl.bop[j][8 + u][L] = b.b1[u];
  }
}
__device__ __forceinline__ BOp bop_load(const OneLds& sl, int j, int L) {
  BOp b;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    b.b0[u] = sl.bop[j][u][L];
    b.b1[u] = sl.bop[j][8 + u][L];
  }
  return b;
}

// PRF instance N (one wave), then for the secret vector (N < nvec) its NTT on lanes 0-15 into
// the shared basemul operands (KeyGen also writes NTT(s_j) to dk; KG: NTT(e_i) kept as fp32).
template <int K, bool KG>
__device__ __forceinline__ void prf_ntt_one(OneLds& sl, int N, uint8_t* __restrict__ dk, const Coop& c) {
  constexpr int ETA_V = P<K>::ETA1, ETA_E = KG ? P<K>::ETA1 : P<K>::ETA2;
  if (N < K)
    prf_coop<ETA_V>(sl.seed, N, sl.ps, c);
  else
    prf_coop<ETA_E>(sl.seed, N, sl.ps, c);
  const int L = threadIdx.x & 63;
  if (L < 16 && (N < K || KG)) {
    wave_phase();
    PF16 f;
    cbd_f<ETA_V>(f, cbd_load<ETA_V, 16>(sl.ps, (size_t)N, L));
    GroupLds& g = sl.g[N];  // N < 2K <= 8 (KeyGen), N < K otherwise
    contig_to_stride_f(f, (float*)g.poly, L);
    ntt_fwd_f<false>(f, (float*)g.poly, L);
    if (N < K) {
      bop_store(sl, N, make_bop_f(f, L), L);
      if (KG) {
        P16 t;
#pragma unroll
        for (int x = 0; x < 16; ++x) t.v[x] = canon_f(f.v[x]);
        encode12(t, dk + 384 * N, L);
      }
    } else {
#pragma unroll
      for (int x = 0; x < 16; ++x) sl.ef[N - K][x][L] = f.v[x];
    }
  }
}

// u_i = Compress_du(NTT^-1(sum_j A[i][j]^T o y_j) + e1_i) on one 16-lane group: written to c (MODE
// 0) or compared with it into diff (MODE 1).
template <int K, int MODE>
__device__ __forceinline__ void enc_row_one(const OneLds& sl, int i, uint8_t* __restrict__ c, uint32_t& diff,
                                            GroupLds& g, int L) {
  constexpr int DU = P<K>::DU;
  int acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) basemul_acc(acc, load_sampled<16>(sl.xs, (size_t)(i * K + j), L), bop_load(sl, j, L));
  const CbdRaw er = cbd_load<P<K>::ETA2, 16>(sl.ps, (size_t)(K + i), L);
  CmpWords<DU> cw;
  if (MODE) cw = cmp_load<DU>(c + 32 * DU * i, L);
  PF16 uf;
#pragma unroll
  for (int t = 0; t < 16; ++t) uf.v[t] = acc_to_f(acc[t]);
  ntt_inv_f(uf, (float*)g.poly, L);
  stride_to_contig_f(uf, (float*)g.poly, L);
  PF16 ef;
  cbd_f<P<K>::ETA2>(ef, er);
  P16 u;
#pragma unroll
  for (int t = 0; t < 16; ++t) u.v[t] = compress_f<DU>(uf.v[t] + ef.v[t]);
  pack_bits<DU>(u, g, L);
  if (MODE)
    flush_cmp<DU>(g, cw, diff, L);
  else
    flush_bits<DU>(g, c + 32 * DU * i, nullptr, diff, true, L);
}

// v = Compress_dv(NTT^-1(t_hat^T o y_hat) + e2 + Decompress_1(m)) on one 16-lane group; returns
// the FIPS 203 modulus-check failure of ek (Encaps status).
template <int K, int MODE>
__device__ __forceinline__ bool enc_v_one(const OneLds& sl, const uint8_t* __restrict__ ek, const uint8_t* __restrict__ m,
                                          uint8_t* __restrict__ c, uint32_t& diff, GroupLds& g, int L) {
  constexpr int DU = P<K>::DU, DV = P<K>::DV;
  int acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < K; ++j) basemul_acc(acc, decode12(ek + 384 * j, bad, L), bop_load(sl, j, L));
  const CbdRaw er = cbd_load<P<K>::ETA2, 16>(sl.ps, (size_t)(2 * K), L);
  const uint32_t mb = (uint32_t)m[2 * L] | ((uint32_t)m[2 * L + 1] << 8);
  PF16 vf;
#pragma unroll
  for (int t = 0; t < 16; ++t) vf.v[t] = acc_to_f(acc[t]);
  ntt_inv_f(vf, (float*)g.poly, L);
  stride_to_contig_f(vf, (float*)g.poly, L);
  PF16 ef;
  cbd_f<P<K>::ETA2>(ef, er);
  P16 v;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float mu = ((mb >> t) & 1) ? (float)((Q + 1) / 2) : 0.0f;
    v.v[t] = compress_f<DV>(vf.v[t] + ef.v[t] + mu);
  }
  pack_bits<DV>(v, g, L);
  flush_bits<DV>(g, c + 32 * DU * K, MODE ? c + 32 * DU * K : nullptr, diff, true, L);
  return group_or(bad ? 1u : 0u) != 0;
}

// The public input of a single-shot host call (n == 1) passed by value, so the kernel does not read
// it over PCIe before H(ek); the secret inputs (the coins m here, dk for Decaps, d || z for KeyGen)
// stay in the pinned mirror, which the host wipes after the call: the HIP runtime's kernel-argument
// pool is never wiped.
template <int K>
struct EncIn {
  uint64_t pk[P<K>::PK / 8];
};
template <int K>
__global__ __launch_bounds__(64 * ONE_WAVES) void k_encaps_one(size_t n, const uint8_t* __restrict__ pk,
                                                                const uint8_t* __restrict__ coins, EncIn<K> in,
                                                                uint8_t* __restrict__ ct,
                                                                uint8_t* __restrict__ ss, int32_t* __restrict__ status,
                                                                uint32_t* done, uint32_t ticket) {
  __shared__ __attribute__((aligned(16))) OneLds sl;
  const size_t hs = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Coop c = coop_init();
  const int i = c.idx;
  constexpr int EKW = P<K>::PK / 8;
  SS_MARK(threadIdx.x == 0, 0);
  SS_CLK(threadIdx.x == 0, 20);
  // ek from memory, or (pk == nullptr: n == 1 host calls) from the kernel argument; m from memory
  stage_in(sl.io, pk ? (const uint64_t*)(pk + hs * P<K>::PK) : in.pk, EKW);
  stage_in(sl.io + EKW, (const uint64_t*)(coins + hs * 32), 4);
  __syncthreads();
  const uint64_t* ek = sl.io;
  if (wave == 0) {  // (K, r) = G(m || H(ek)): the critical chain
    __builtin_amdgcn_s_setprio(3);
    CState s;
    coop_absorb<RW_SHA3_256, P<K>::PK / 8, DS_SHA3>(s, c, [&](int w) { return ek[w]; });
    const uint64_t h = cs_get(s, (i >= 4 && i < 8) ? i - 4 : 0);
    const uint64_t* m = sl.io + EKW;
    CState g;
    if (i >= 0 && i < 4) cs_xor(g, m[i]);
    if (i >= 4 && i < 8) cs_xor(g, h);
    if (i == 8) {
      g.lo ^= DS_SHA3;
      g.hi ^= 0x80000000u;
    }
    g = kf_coop(g, c);
    if (i >= 0 && i < 4) ((uint64_t*)(ss + hs * 32))[i] = cs_word(g);
    if (i >= 4 && i < 8) sl.seed[i - 4] = cs_word(g);
    __builtin_amdgcn_s_setprio(0);
    SS_MARK(threadIdx.x == 0, 1);
    SS_CLK(threadIdx.x == 0, 21);
  } else {
#pragma unroll 1
    for (int e = wave - 1; e < K * K; e += ONE_WAVES - 1)
      xof_coop<K>(ek + 48 * K, e, (uint16_t*)sl.xs, sl.pbuf[wave], c);
    SS_MARK(threadIdx.x == 64, 3);
  }
  __syncthreads();
  if (wave < 2 * K + 1) prf_ntt_one<K, false>(sl, wave, nullptr, c);  // PRF(r, N), NTT(y_N)
  SS_MARK(threadIdx.x == 0, 2);
  __syncthreads();
  SS_MARK(threadIdx.x == 0, 4);
  uint8_t* cc = ct + hs * P<K>::CT;
  uint32_t diff = 0;
  if (wave == 0 && (lane >> 4) < K) {
    enc_row_one<K, 0>(sl, lane >> 4, cc, diff, sl.g[lane >> 4], lane & 15);
  } else if (wave == 1 && lane < 16) {
    const bool bad = enc_v_one<K, 0>(sl, (const uint8_t*)ek, (const uint8_t*)(sl.io + EKW), cc, diff, sl.g[4], lane);
    if (status && lane == 0) status[hs] = bad ? -1 : 0;
  }
  SS_MARK(threadIdx.x == 0, 7);
  wipe_one(sl, done, ticket);
}

// the ciphertext of a single-shot host call passed by value (<= 1568 B); dk stays in the pinned mirror
template <int K>
struct DecIn {
  uint64_t ct[P<K>::CT / 8];
};
template <int K>
__global__ __launch_bounds__(64 * ONE_WAVES) void k_decaps_one(size_t n, const uint8_t* __restrict__ ct,
                                                                const uint8_t* __restrict__ sk, DecIn<K> in,
                                                                uint8_t* __restrict__ ss,
                                                                uint32_t* done, uint32_t ticket) {
  __shared__ __attribute__((aligned(16))) OneLds sl;
  const size_t hs = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Coop c = coop_init();
  const int i = c.idx;
  constexpr int CTW = P<K>::CT / 8, SKW = P<K>::SK / 8;
  // c from memory, or (ct == nullptr: n == 1 host calls) from the kernel argument; dk from memory
  stage_in(sl.io, ct ? (const uint64_t*)(ct + hs * P<K>::CT) : in.ct, CTW);
  stage_in(sl.io + CTW, (const uint64_t*)(sk + hs * P<K>::SK), SKW);
  uint8_t* cc = (uint8_t*)sl.io;                   // the received ciphertext (LDS copy)
  const uint8_t* dk = (const uint8_t*)(sl.io + CTW);  // dk (LDS copy)
  constexpr int XW = ONE_WAVES - 3;  // SampleNTT waves 2 .. ONE_WAVES - 2; the last wave computes v
  if (threadIdx.x == 0) sl.flag_seed = sl.flag_kb = sl.n_ready = sl.n_xof = sl.n_done = 0;
  __syncthreads();
  SS_MARK(threadIdx.x == 0, 0);
  if (wave == 0) {  // m' = Decrypt(c), (K', r') = G(m' || h), PRF(r', 0), then the u rows and the select
    if (lane < 16) decrypt_core_hs<K, 16>(n, cc, dk, sl.mp, hs, lane, sl.g[5]);
    SS_MARK(lane == 0, 8);
    wave_phase();
    const uint64_t* h = (const uint64_t*)(dk + 768 * K + 32);
    CState g;
    if (i >= 0 && i < 4) cs_xor(g, sl.mp[i]);
    if (i >= 4 && i < 8) cs_xor(g, h[i - 4]);
    if (i == 8) {
      g.lo ^= DS_SHA3;
      g.hi ^= 0x80000000u;
    }
    g = kf_coop(g, c);
    if (i >= 0 && i < 4) sl.kp[i] = cs_word(g);
    if (i >= 4 && i < 8) sl.seed[i - 4] = cs_word(g);
    one_signal(&sl.flag_seed);
    SS_MARK(lane == 0, 9);
    prf_ntt_one<K, false>(sl, 0, nullptr, c);
    one_signal(&sl.n_ready);
    one_wait(&sl.n_ready, 2 * K + 1);
    one_wait(&sl.n_xof, K * K);
    SS_MARK(lane == 0, 4);
    uint32_t diff = 0;
    if ((lane >> 4) < K) enc_row_one<K, 1>(sl, lane >> 4, cc, diff, sl.g[lane >> 4], lane & 15);
    diff = group_or(diff);
    if ((lane & 15) == 0 && (lane >> 4) < K) sl.diff[lane >> 4] = diff;
    one_wait(&sl.n_done, 1);   // v
    one_wait(&sl.flag_kb, 1);  // Kbar
    SS_MARK(lane == 0, 6);
    if (lane < 8) {  // constant-time select: ss = (c == c') ? K' : Kbar
      uint32_t d = sl.diff[4];
#pragma unroll
      for (int r = 0; r < K; ++r) d |= sl.diff[r];
      const uint32_t mask = (uint32_t)(((uint64_t)d - 1u) >> 32);  // all-ones iff d == 0, no branch
      const uint32_t kp = ((const uint32_t*)sl.kp)[lane], kb = ((const uint32_t*)sl.kb)[lane];
      ((uint32_t*)(ss + hs * 32))[lane] = (kp & mask) | (kb & ~mask);
    }
    SS_MARK(lane == 0, 7);
  } else if (wave == 1) {  // Kbar = J(z || c) beside everything else
    __builtin_amdgcn_s_setprio(3);
    const uint64_t* z = (const uint64_t*)(dk + 768 * K + 64);
    const uint64_t* cw = (const uint64_t*)cc;
    CState s;
    coop_absorb<RW_SHAKE256, 4 + P<K>::CT / 8, DS_SHAKE>(s, c, [&](int w) { return w < 4 ? z[w] : cw[w - 4]; });
    if (i >= 0 && i < 4) sl.kb[i] = cs_word(s);
    __builtin_amdgcn_s_setprio(0);
    one_signal(&sl.flag_kb);
    SS_MARK(lane == 0, 11);
  } else if (wave < ONE_WAVES - 1) {  // SampleNTT, then PRF(r', N) for N = wave - 1
#pragma unroll 1
    for (int e = wave - 2; e < K * K; e += XW) {
      xof_coop<K>((const uint64_t*)(dk + 768 * K), e, (uint16_t*)sl.xs, sl.pbuf[wave], c);
      one_signal(&sl.n_xof);
    }
    SS_MARK(lane == 0 && wave == 2, 12);
    const int N = wave - 1;
    if (N < 2 * K + 1) {
      one_wait(&sl.flag_seed, 1);
      prf_ntt_one<K, false>(sl, N, nullptr, c);
      one_signal(&sl.n_ready);
    }
    SS_MARK(lane == 0 && wave == 2, 10);
  } else {  // v
    one_wait(&sl.n_ready, 2 * K + 1);
    if (lane < 16) {
      uint32_t diff = 0;
      enc_v_one<K, 1>(sl, dk + 384 * K, (const uint8_t*)sl.mp, cc, diff, sl.g[4], lane);
      diff = group_or(diff);
      if (lane == 0) sl.diff[4] = diff;
    }
    one_signal(&sl.n_done);
  }
  wipe_one(sl, done, ticket);
}

template <int K>
__global__ __launch_bounds__(64 * KG_WAVES) void k_keygen_one(size_t n, const uint8_t* __restrict__ coins,
                                                                uint8_t* __restrict__ pk, uint8_t* __restrict__ sk,
                                                                uint32_t* done, uint32_t ticket) {
  __shared__ __attribute__((aligned(16))) OneLds sl;
  const size_t hs = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Coop c = coop_init();
  const int i = c.idx;
  uint8_t* ek = pk + hs * P<K>::PK;
  uint8_t* dk = sk + hs * P<K>::SK;
  SS_MARK(threadIdx.x == 0, 0);
  // z (dk's last 32 bytes) is loaded with d: the coins row may be host memory (single-shot calls),
  // and a load after H(ek) put one more PCIe round trip on the critical path
  const uint64_t zw = (wave == 0 && i >= 0 && i < 4) ? ((const uint64_t*)(coins + hs * 64 + 32))[i] : 0;
  if (wave == 0) {  // (rho, sigma) = G(d || k)
    const uint64_t* d = (const uint64_t*)(coins + hs * 64);
    CState g;
    if (i >= 0 && i < 4) cs_xor(g, d[i]);
    if (i == 4) g.lo ^= (uint32_t)K | (DS_SHA3 << 8);
    if (i == RW_SHA3_512 - 1) g.hi ^= 0x80000000u;
    g = kf_coop(g, c);
    if (i >= 0 && i < 4) {
      ((uint64_t*)(ek + 384 * K))[i] = cs_word(g);
      ((uint64_t*)(dk + 768 * K))[i] = cs_word(g);
      sl.kp[i] = cs_word(g);  // rho for SampleNTT
      sl.io[48 * K + i] = cs_word(g);  // ek's LDS copy (hashed below)
    }
    if (i >= 4 && i < 8) sl.seed[i - 4] = cs_word(g);
    SS_MARK(threadIdx.x == 0, 13);
  }
  __syncthreads();
#pragma unroll 1
  for (int it = wave; it < 2 * K + K * K; it += KG_WAVES) {  // the 2K PRFs (+ NTTs) first, then SampleNTT
    if (it < 2 * K)
      prf_ntt_one<K, true>(sl, it, dk, c);
    else
      xof_coop<K>(sl.kp, it - 2 * K, (uint16_t*)sl.xs, sl.pbuf[wave], c);
  }
  SS_MARK(threadIdx.x == 0, 14);
  __syncthreads();
  SS_MARK(threadIdx.x == 0, 4);
  if (wave == 0 && (lane >> 4) < K) {  // t_hat_i = sum_j A[i][j] o s_hat_j + e_hat_i, one group per row
    const int r = lane >> 4, L = lane & 15;
    int acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) basemul_acc(acc, load_sampled<16>(sl.xs, (size_t)(j * K + r), L), bop_load(sl, j, L));
    P16 t;
#pragma unroll
    for (int x = 0; x < 16; ++x) t.v[x] = canon_f(acc_to_f(acc[x]) + sl.ef[r][x][L]);
    encode12(t, ek + 384 * r, L);
    encode12(t, dk + 384 * K + 384 * r, L);
    encode12(t, (uint8_t*)sl.io + 384 * r, L);
  }
  SS_MARK(threadIdx.x == 0, 16);
  __syncthreads();
  if (wave == 0) {  // dk tail: H(ek) || z
    const uint64_t* ekw = sl.io;
    CState s;
    coop_absorb<RW_SHA3_256, P<K>::PK / 8, DS_SHA3>(s, c, [&](int w) { return ekw[w]; });
    uint64_t* tail = (uint64_t*)(dk + 768 * K + 32);
    if (i >= 0 && i < 4) {
      tail[i] = cs_word(s);
      tail[4 + i] = zw;
    }
    SS_MARK(threadIdx.x == 0, 17);
  }
  wipe_one(sl, done, ticket);
}

// ============================================================ host launchers

hipError_t keygen_one(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, const Streams& s) {
  return with_rank(k, [&](auto rank) {
    constexpr int K = decltype(rank)::value;
    QRK_LAUNCH("k_keygen_one", s.main, k_keygen_one<K>, dim3((unsigned)n), dim3(64 * KG_WAVES), 0, s.main, n, coins,
               pk, sk, n == 1 ? s.done : nullptr, s.ticket);
    return launch_status();
  });
}

hipError_t encaps_one(int k, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                      int32_t* status, const Streams& s) {
  return with_rank(k, [&](auto rank) {
    constexpr int K = decltype(rank)::value;
    EncIn<K> in{};
    const bool by_value = n == 1 && s.host_in1;
    if (by_value) memcpy(in.pk, s.host_in1, sizeof(in.pk));
    QRK_LAUNCH("k_encaps_one", s.main, k_encaps_one<K>, dim3((unsigned)n), dim3(64 * ONE_WAVES), 0, s.main, n,
               by_value ? nullptr : pk, coins, in, ct, ss, status, n == 1 ? s.done : nullptr, s.ticket);
    return launch_status();
  });
}

hipError_t decaps_one(int k, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, const Streams& s) {
  return with_rank(k, [&](auto rank) {
    constexpr int K = decltype(rank)::value;
    DecIn<K> in{};
    const bool by_value = n == 1 && s.host_in1;
    if (by_value) memcpy(in.ct, s.host_in1, sizeof(in.ct));
    QRK_LAUNCH("k_decaps_one", s.main, k_decaps_one<K>, dim3((unsigned)n), dim3(64 * ONE_WAVES), 0, s.main, n,
               by_value ? nullptr : ct, sk, in, ss, n == 1 ? s.done : nullptr, s.ticket);
    return launch_status();
  });
}

}  // namespace mlkem

size_t mlkem_small_max() { return QRK_SMALL_MAX; }

}  // namespace qrk

#if QRK_SS_TRACE  // declared in qrkem_debug.h, which mlkem.hip includes
int qrk_dbg_ss_trace(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(qrk::mlkem::g_ss_trace), sizeof(qrk::mlkem::g_ss_trace)) == hipSuccess ? 0 : -1;
}
#endif
