// ML-KEM (FIPS 203), the single-shot multi-workgroup KeyGens for n <= QRK_KG_MULTI_MAX:
// k_keygen_multi (no cross-workgroup waits) and k_keygen_pipe (H(ek) pipelined with SampleNTT over
// sc1 hand-offs and bounded waits).  Part of the translation unit mlkem.hip.
#pragma once
#include "mlkem_coop.cuh"
#include "mlkem_paths.h"
#include "mlkem_poly.cuh"
#include "mlkem_trace.cuh"

namespace qrk {
namespace mlkem {

// ------------------------------------------------------------ single-shot KeyGen over K^2 + 2K workgroups
// k_keygen_one runs the 2K PRFs and K^2 SampleNTT entries of one handshake as 15 waves (ML-KEM-768)
// of one workgroup: their cooperative permutations share one CU and take ~2x their isolated time
// (phase trace: 18.8 us for 3 + 1 sequential permutations, profiles/r2/single_shot_trace_final.json).
// For n <= QRK_KG_MULTI_MAX the items get a one-wave workgroup each, on different CUs: every
// workgroup runs G(d || k) itself (one permutation, no cross-workgroup wait), then its item, writes
// the result to the context scratch (MkScr) and counts itself in with a device-scope fence and an
// atomic add; the workgroup that arrives last computes t_hat on four 16-lane groups, hashes ek
// (H(ek), 9 permutations at ML-KEM-768) and wipes the scratch and its counter.  No workgroup waits
// for another (the last one simply finds everything published), so nothing can spin.
#ifndef QRK_KG_MULTI_MAX
#define QRK_KG_MULTI_MAX 16
#endif
// 1 (default): host-pointer KeyGen calls of n <= QRK_KG_MULTI_MAX run k_keygen_pipe (H(ek) pipelined
// with SampleNTT, below; 37.5 against 41.6 us per kernel, profiles/r5/single_shot/), which reports a
// lost hand-off through the call's error word (Streams::kg_err); device-pointer calls, which have no
// host-visible error word, keep k_keygen_multi (no cross-workgroup waits, so nothing to time out).
// 0: k_keygen_multi everywhere (A/B builds: tools/build_variant.sh ... -DQRK_KG_PIPE=0).
#ifndef QRK_KG_PIPE
#define QRK_KG_PIPE 1
#endif
struct MkScr {
  uint4 xs[32 * 16];        // SampleNTT entries, load_sampled<16> layout (K^2 <= 16)
  uint32_t bop[4][16][16];  // NTT(s_j) basemul operands, word w of lane L at [j][w][L]
  float ef[4][16][16];      // NTT(e_i), coefficient t of lane L at [i][t][L]
};
struct MkLds {
  uint64_t ps[PRF_W * 16];
  uint32_t pbuf[44];
  uint64_t rho[4], sigma[4];
  uint64_t io[200];  // ek (KeyGen's LDS copy for H(ek)): 1568 B at K = 4
  GroupLds g[4];
  int last;
};
__device__ __forceinline__ void mk_wipe_lds(MkLds& sl) {
  __syncthreads();
  uint4* w = (uint4*)&sl;
  for (int x = threadIdx.x; x < (int)(sizeof(MkLds) / 16); x += (int)blockDim.x) w[x] = make_uint4(0, 0, 0, 0);
}

template <int K>
__global__ __launch_bounds__(64) void k_keygen_multi(size_t n, const uint8_t* __restrict__ coins,
                                                     uint8_t* __restrict__ pk, uint8_t* __restrict__ sk,
                                                     MkScr* __restrict__ scr_all, uint32_t* __restrict__ cnt,
                                                     uint32_t* done, uint32_t ticket) {
  constexpr int NI = 2 * K + K * K;
  __shared__ __attribute__((aligned(16))) MkLds sl;
  const size_t hs = blockIdx.x / NI;
  const int item = (int)(blockIdx.x % NI);
  const int lane = threadIdx.x;
  const Coop c = coop_init();
  const int i = c.idx;
  MkScr& scr = scr_all[hs];
  uint8_t* ek = pk + hs * P<K>::PK;
  uint8_t* dk = sk + hs * P<K>::SK;
  // the coins row (secret: always memory, never a kernel argument); z for dk's tail is loaded with d
  // rather than after H(ek) in the last workgroup
  const uint64_t* cw = (const uint64_t*)(coins + hs * 64);
  const uint64_t zw = (i >= 0 && i < 4) ? cw[4 + i] : 0;
  SS_MARK(blockIdx.x == 0 && lane == 0, 0);
  SS_MARK(blockIdx.x == NI - 1 && lane == 0, 14);
  {  // (rho, sigma) = G(d || k), in every workgroup
    const uint64_t* d = cw;
    CState g;
    if (i >= 0 && i < 4) cs_xor(g, d[i]);
    if (i == 4) g.lo ^= (uint32_t)K | (DS_SHA3 << 8);
    if (i == RW_SHA3_512 - 1) g.hi ^= 0x80000000u;
    g = kf_coop(g, c);
    if (i >= 0 && i < 4 && coop_canon(c)) sl.rho[i] = cs_word(g);
    if (i >= 4 && i < 8 && coop_canon(c)) sl.sigma[i - 4] = cs_word(g);
    wave_phase();
    SS_MARK(blockIdx.x == 0 && lane == 0, 13);
  }
  if (item < 2 * K) {  // PRF(sigma, item) -> CBD -> NTT: s_item (operand + dk) or e_(item - K)
    prf_coop<P<K>::ETA1>(sl.sigma, item, sl.ps, c);
    wave_phase();
    if (lane < 16) {
      PF16 f;
      cbd_f<P<K>::ETA1>(f, cbd_load<P<K>::ETA1, 16>(sl.ps, (size_t)item, lane));
      contig_to_stride_f(f, (float*)sl.g[0].poly, lane);
      ntt_fwd_f<false>(f, (float*)sl.g[0].poly, lane);
      if (item < K) {
        const BOp b = make_bop_f(f, lane);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          scr.bop[item][u][lane] = b.b0[u];
          scr.bop[item][8 + u][lane] = b.b1[u];
        }
        P16 t;
#pragma unroll
        for (int x = 0; x < 16; ++x) t.v[x] = canon_f(f.v[x]);
        encode12(t, dk + 384 * item, lane);
      } else {
#pragma unroll
        for (int x = 0; x < 16; ++x) scr.ef[item - K][x][lane] = f.v[x];
      }
    }
  } else {  // SampleNTT entry e = x K + y straight into the scratch
    xof_coop<K>(sl.rho, item - 2 * K, (uint16_t*)scr.xs, sl.pbuf, c);
    SS_MARK(item == 2 * K && lane == 0, 15);
  }
  // publish, then count in: the last of the NI workgroups of this handshake finishes it.  With a
  // host-visible completion flag (n == 1, zero-copy pinned outputs) every workgroup's dk stores are
  // released at system scope before it counts in, so the host-side ordering does not rest on
  // agent -> system release transitivity across the XCDs' L2s.
  if (done)
    __threadfence_system();
  else
    __threadfence();
  __syncthreads();
  if (lane == 0) sl.last = (int)(atomicAdd(&cnt[hs], 1u) == (uint32_t)(NI - 1));
  __syncthreads();
  if (!sl.last) {
    mk_wipe_lds(sl);
    return;
  }
  __threadfence();  // acquire: the other workgroups' stores are visible past the counter
  SS_MARK(lane == 0, 4);
  if ((lane >> 4) < K) {  // t_hat_r = sum_j A[r][j] o s_hat_j + e_hat_r, one 16-lane group per row
    const int r = lane >> 4, L = lane & 15;
    int acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      BOp b;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        b.b0[u] = scr.bop[j][u][L];
        b.b1[u] = scr.bop[j][8 + u][L];
      }
      basemul_acc(acc, load_sampled<16>(scr.xs, (size_t)(j * K + r), L), b);
    }
    P16 t;
#pragma unroll
    for (int x = 0; x < 16; ++x) t.v[x] = canon_f(acc_to_f(acc[x]) + scr.ef[r][x][L]);
    encode12(t, ek + 384 * r, L);
    encode12(t, dk + 384 * K + 384 * r, L);
    encode12(t, (uint8_t*)sl.io + 384 * r, L);
  }
  if (lane < 4) {
    ((uint64_t*)(ek + 384 * K))[lane] = sl.rho[lane];
    ((uint64_t*)(dk + 768 * K))[lane] = sl.rho[lane];
    sl.io[48 * K + lane] = sl.rho[lane];
  }
  wave_phase();
  SS_MARK(lane == 0, 16);
  {  // dk tail: H(ek) || z
    CState s;
    coop_absorb<RW_SHA3_256, P<K>::PK / 8, DS_SHA3>(s, c, [&](int w) { return sl.io[w]; });
    uint64_t* tail = (uint64_t*)(dk + 768 * K + 32);
    if (i >= 0 && i < 4 && coop_canon(c)) {
      tail[i] = cs_word(s);
      tail[4 + i] = zw;
    }
    SS_MARK(lane == 0, 17);
  }
  // wipe the handshake's scratch (s_hat, e_hat, A) and reset its counter for the next call (wiping
  // it before H(ek) instead delays H by 0.9 us and saves 0.4 us after it:
  // profiles/r4/single_shot/keygen_trace_*.json)
  {
    uint4* w = (uint4*)&scr;
    for (int x = lane; x < (int)(sizeof(MkScr) / 16); x += 64) w[x] = make_uint4(0, 0, 0, 0);
  }
  if (lane == 0) atomicSub(&cnt[hs], (uint32_t)NI);
  if (done) __threadfence_system();
  mk_wipe_lds(sl);
  SS_MARK(lane == 0, 18);
  if (done && lane == 0) {
    // n == 1: the only handshake; the flag means every output is visible to the host
    __hip_atomic_store(done, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ------------------------------------------------------------ single-shot KeyGen, H(ek) pipelined
// k_keygen_multi's critical path is G, three SampleNTT blocks, the count-in, t_hat, then the nine
// permutations of H(ek) = SHA3-256(t_hat || rho): 13 sequential cooperative permutations.  H(ek)
// absorbs t_hat_0 first, and t_hat_0's coefficient c needs only coefficient c of the row-0 entries
// A[0][j], which SampleNTT emits in FIPS order: so H's first blocks can run while SampleNTT still
// squeezes.  k_keygen_pipe, per handshake, 3K workgroups of K + 2 waves:
//   PRF items (2K, one wave busy): G, PRF(sigma, N), CBD, NTT -> NTT(s_j) basemul operands or
//     NTT(e_i) into the scratch, published to the others (write-through sc1 stores, a drained wave,
//     then an sc1 flag store: MI355X_MICROARCH.md "Valid forms", table row 1); dk's s_hat bytes
//   row r = 1 .. K-1 (K waves): G and SampleNTT A[r][j] (wave j), then t_hat_r, published the same
//     way; ek / dk's t_hat_r bytes
//   row 0 = the collector (K + 2 waves): waves 0 .. K-1 G and SampleNTT A[0][j], bumping an LDS count
//     after every block; wave K computes t_hat_0 in three ranges of coefficient pairs as soon as
//     every A[0][j] has emitted them (H(ek) blocks 0, 1 and 2 need t_hat_0 bytes < 136, < 272, all),
//     then copies t_hat_1 .. t_hat_{K-1} in from the row workgroups; wave K + 1 computes G itself
//     and absorbs ek block by block as its bytes arrive
// The critical path becomes G, SampleNTT's first two blocks (one block yields ~91 coefficients,
// H's block 0 needs 92), then the nine H(ek) permutations: 11 permutations.
// Hand-offs (MI355X_MICROARCH.md "Valid forms", the Consumer bullet with the acquire kept): the
// producer wave stores every payload byte with sc1 stores, waits vmcnt(0), then one lane stores the
// flag (sc1); the consumer wave polls the flag with relaxed sc1 loads, then ONE agent-scope acquire
// (buffer_inv sc1 + vmcnt(0): the CU's L1 may hold a stale line, the producer may sit on another
// XCD), then loads the payload in that same wave.
// Failure semantics: every wait is a bounded spin (KG_SPIN_TICKS).  A wait that expires marks its
// workgroup in error; a workgroup's outputs-done flag carries it (2 instead of 1); the collector,
// which waits for every other workgroup's flag, stores 1 into the call's error word (host-mapped,
// Streams::kg_err) before the completion ticket when any wait of the handshake expired, and the host
// returns OQS_ERROR for the call, re-zeroes the flag words (a straggler may set one after the
// collector's reset) and wipes the scratch.  The collector waits until every other workgroup has
// published its host outputs (system-scope release before the flag when the outputs are host
// memory), wipes the secret scratch (s_hat, e_hat), resets the flags and stores the ticket.
struct PipeScr {
  uint32_t bop[4][16][16];  // NTT(s_j) basemul operands, word w of lane L at [j][w][L] (secret)
  float ef[4][16][16];      // NTT(e_i), coefficient t of lane L at [i][t][L] (secret)
  uint32_t th[4][96];       // t_hat_r as ek bytes, rows 1 .. K-1 (public)
};
// flag words per handshake (ctx->kg_cnt, zeroed at allocation, reset by the collector):
// [N] PRF item N published, [8 + r] t_hat_r published, [16 + w] workgroup w's outputs written
constexpr int KG_FLAGS = 32;
struct PipeLds {
  uint4 xs[32 * 4];        // the workgroup's K <= 4 entries, load_sampled<4> layout
  uint32_t pbuf[4][44];    // SampleNTT parse buffers
  uint32_t bop[4][16][16];  // collector: the NTT(s_j) operands
  float ef[16][16];        // collector: NTT(e_0)
  uint64_t io[200];        // collector: ek (1568 B at K = 4)
  uint64_t rho[4][4];      // per SampleNTT wave
  uint64_t ps[PRF_W * 16];  // PRF items
  uint64_t sigma[4];
  GroupLds g;
  int prog[4], io_ready;
  int err;  // a bounded wait of this workgroup expired
};
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(1))) uint64_t gu64;
__device__ __forceinline__ void st_sc1(uint32_t* p, uint32_t v) {
  __hip_atomic_store((gu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_sc1(const uint32_t* p) {
  return __hip_atomic_load((gu32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// bounded spins (50 ms of the 100 MHz wall clock): a lost hand-off ends the kernel (and reports
// itself through the error word) instead of hanging the GPU
constexpr uint64_t KG_SPIN_TICKS = 5000000;
// one wave polls flag words (relaxed sc1 loads, all of them issued per pass) until every one is
// nonzero or the spin expires (returns false); *orv = OR of the values last read.  ACQ: the payload
// loads that follow in this wave are ordered by one agent-scope acquire (invalidates this CU's L1;
// its vmcnt(0) waits for the invalidate); without ACQ no payload is read after the poll.
template <int NF, bool ACQ>
__device__ __forceinline__ bool kg_wait_flags(const uint32_t* const (&f)[NF], uint32_t* orv = nullptr) {
  const uint64_t t0 = wall_clock64();
  bool all;
  uint32_t o;
  for (;;) {
    uint32_t v[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) v[k] = ld_sc1(f[k]);
    all = true;
    o = 0u;
#pragma unroll
    for (int k = 0; k < NF; ++k) all = all && v[k] != 0u, o |= v[k];
    if (all || wall_clock64() - t0 >= KG_SPIN_TICKS) break;
    __builtin_amdgcn_s_sleep(1);
  }
  if (ACQ) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (orv) *orv = o;
  return all;
}
__device__ __forceinline__ bool kg_wait_flag(const uint32_t* f) {
  const uint32_t* const a[1] = {f};
  return kg_wait_flags<1, true>(a);
}
// the storing wave's sc1 stores drained, then one lane stores the flag
__device__ __forceinline__ void kg_publish(uint32_t* f) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) st_sc1(f, 1u);
}
__device__ __forceinline__ bool lds_wait_ge(const int* p, int v) {
  const uint64_t t0 = wall_clock64();
  bool ok;
  while (!(ok = __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= v) &&
         wall_clock64() - t0 < KG_SPIN_TICKS)
    __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return ok;
}
// a wave whose bounded wait expired marks its workgroup in error (the whole wave stores the same 1)
__device__ __forceinline__ void kg_mark(PipeLds& sl, bool ok) {
  if (!ok) sl.err = 1;
}
__device__ __forceinline__ void lds_release_store(int* p, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (rho, sigma) = G(d || k) on one wave
__device__ __forceinline__ CState g_keygen_coop(const uint64_t* d, int K, const Coop& c) {
  const int i = c.idx;
  CState g;
  if (i >= 0 && i < 4) cs_xor(g, d[i]);
  if (i == 4) g.lo ^= (uint32_t)K | (DS_SHA3 << 8);
  if (i == RW_SHA3_512 - 1) g.hi ^= 0x80000000u;
  return kf_coop(g, c);
}
// SampleNTT A[r][j] = SampleNTT(rho || j || r) on wave j into slot j of the workgroup's entries
template <int K>
__device__ __forceinline__ void kg_pipe_sample(PipeLds& sl, const uint64_t* d, int r, int j, const Coop& c) {
  const CState g = g_keygen_coop(d, K, c);
  if (c.idx >= 0 && c.idx < 4 && coop_canon(c)) sl.rho[j][c.idx] = cs_word(g);
  wave_phase();
  uint16_t* xs16 = (uint16_t*)sl.xs;
  xof_coop_place<K>(
      sl.rho[j], j * K + r, sl.pbuf[j], c, [&](int q, uint32_t v) { xs16[(((q >> 3) * 4 + j) << 3) + (q & 7)] = (uint16_t)v; },
      [&](int cnt) {
        lds_release_store(&sl.prog[j], cnt < 256 ? cnt : 256);
        SS_MARK(r == 0 && j == 0 && (threadIdx.x & 63) == 0, cnt < 120 ? 10 : cnt < 210 ? 11 : 12);
      });
}
// The s_hat operands and e_hat_r from the PRF workgroups into LDS (one wave): it waits for their K + 1
// flags, then issues every 8-byte sc1 load before the first LDS store (one round trip, not one per load)
template <int K>
__device__ __forceinline__ void kg_load_ops(PipeLds& sl, const PipeScr& scr, const uint32_t* fl, int r) {
  const uint32_t* f[K + 1];
#pragma unroll
  for (int j = 0; j < K; ++j) f[j] = &fl[j];
  f[K] = &fl[K + r];
  kg_mark(sl, kg_wait_flags<K + 1, true>(f));
  const int lane = threadIdx.x & 63;
  constexpr int NB = K * 128 / 64, NE = 128 / 64;  // u64 words per lane
  uint64_t vb[NB], ve[NE];
  const uint64_t* sb = (const uint64_t*)&scr.bop[0][0][0];
  const uint64_t* se = (const uint64_t*)&scr.ef[r][0][0];
#pragma unroll
  for (int k = 0; k < NB; ++k) vb[k] = __hip_atomic_load((const gu64*)(sb + lane + 64 * k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < NE; ++k) ve[k] = __hip_atomic_load((const gu64*)(se + lane + 64 * k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < NB; ++k) ((uint64_t*)&sl.bop[0][0][0])[lane + 64 * k] = vb[k];
#pragma unroll
  for (int k = 0; k < NE; ++k) ((uint64_t*)&sl.ef[0][0])[lane + 64 * k] = ve[k];
  wave_phase();
}
// t_hat_r coefficient pair p (K-term basemul from the entries in LDS and the s_hat operands, + e_hat)
// as its three ek bytes
template <int K, typename BopAt, typename EfAt>
__device__ __forceinline__ uint32_t kg_pipe_pair(const PipeLds& sl, int p, BopAt bop_at, EfAt ef_at) {
  const int L = p >> 3, u = p & 7;
  int a0 = 0, a1 = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t a = ((const uint32_t*)sl.xs)[(((2 * p) >> 3) * 4 + j) * 4 + (p & 3)];
    a0 = dot2(a, bop_at(j, u, L), a0);
    a1 = dot2(a, bop_at(j, 8 + u, L), a1);
  }
  const uint32_t t0 = (uint32_t)canon_f(acc_to_f(a0) + ef_at(2 * u, L));
  const uint32_t t1 = (uint32_t)canon_f(acc_to_f(a1) + ef_at(2 * u + 1, L));
  return t0 | (t1 << 12);  // 24 bits, little-endian ek bytes 3p .. 3p + 2
}
// tests only (qrk_dbg_kg_late): the workgroup of role `late` (>= 0: PRF item N = role < 2K, or row
// r = role - 2K + 1) sleeps this long before it stores its payload and flags, past every consumer's
// and the collector's bounded wait
constexpr uint64_t KG_DBG_LATE_TICKS = 15000000;  // 150 ms
__device__ __forceinline__ void kg_dbg_sleep() {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < KG_DBG_LATE_TICKS) __builtin_amdgcn_s_sleep(127);
}
template <int K>
__global__ __launch_bounds__(64 * (K + 2)) void k_keygen_pipe(size_t n, const uint8_t* __restrict__ coins,
                                                              uint8_t* __restrict__ pk, uint8_t* __restrict__ sk,
                                                              PipeScr* __restrict__ scr_all, uint32_t* __restrict__ flags,
                                                              uint32_t* done, uint32_t ticket, uint32_t* err, int late) {
  constexpr int NWG = 3 * K, PKB = P<K>::PK;
  __shared__ __attribute__((aligned(16))) PipeLds sl;
  const size_t hs = blockIdx.x / NWG;
  const int role = (int)(blockIdx.x % NWG);  // [0, 2K) PRF items, [2K, 3K - 1) rows 1 .. K-1, 3K - 1 the collector
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Coop c = coop_init();
  const int i = c.idx;
  PipeScr& scr = scr_all[hs];
  uint32_t* fl = flags + hs * KG_FLAGS;
  uint8_t* ek = pk + hs * PKB;
  uint8_t* dk = sk + hs * P<K>::SK;
  const uint64_t* d = (const uint64_t*)(coins + hs * 64);
  // returns whether any wait of this workgroup expired, then wipes the LDS
  auto wipe_lds = [&] {
    __syncthreads();
    const int e = sl.err;
    __syncthreads();
    uint4* w = (uint4*)&sl;
    for (int x = threadIdx.x; x < (int)(sizeof(PipeLds) / 16); x += (int)blockDim.x) w[x] = make_uint4(0, 0, 0, 0);
    return e != 0;
  };
  // a non-collector workgroup's last act (after its LDS wipe): its host-memory outputs released at
  // system scope, then its flag, 2 when one of its waits expired (the collector's done ticket follows
  // every such flag)
  auto outputs_done = [&](int w, bool e) {
    if (done) __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      st_sc1(&fl[16 + w], e ? 2u : 1u);
    }
  };
  if (threadIdx.x < 4) sl.prog[threadIdx.x] = 0;
  if (threadIdx.x == 0) sl.io_ready = 0, sl.err = 0;
  __syncthreads();
  SS_MARK(role == NWG - 1 && threadIdx.x == 0, 0);
  if (role < 2 * K) {  // ------------------------------------------------ PRF item N = role
    const int N = role;
    if (wave == 0) {
      const CState g = g_keygen_coop(d, K, c);
      if (i >= 4 && i < 8 && coop_canon(c)) sl.sigma[i - 4] = cs_word(g);
      wave_phase();
      prf_coop<P<K>::ETA1>(sl.sigma, N, sl.ps, c);
      wave_phase();
      PF16 f;
      if (lane < 16) {
        cbd_f<P<K>::ETA1>(f, cbd_load<P<K>::ETA1, 16>(sl.ps, (size_t)N, lane));
        contig_to_stride_f(f, (float*)sl.g.poly, lane);
        ntt_fwd_f<false>(f, (float*)sl.g.poly, lane);
        if (role == late) kg_dbg_sleep();
        if (N < K) {
          const BOp b = make_bop_f(f, lane);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            st_sc1(&scr.bop[N][u][lane], b.b0[u]);
            st_sc1(&scr.bop[N][8 + u][lane], b.b1[u]);
          }
        } else {
#pragma unroll
          for (int x = 0; x < 16; ++x) st_sc1((uint32_t*)&scr.ef[N - K][x][lane], __float_as_uint(f.v[x]));
        }
      }
      kg_publish(&fl[N]);
      SS_MARK(N == 0 && lane == 0, 1);
      if (N < K && lane < 16) {
        P16 t;
#pragma unroll
        for (int x = 0; x < 16; ++x) t.v[x] = canon_f(f.v[x]);
        encode12(t, dk + 384 * N, lane);
      }
    }
    // sigma, the PRF output and NTT(s) / NTT(e): wiped before the flag that ends this workgroup
    const bool e = wipe_lds();
    outputs_done(N, e);
    return;
  }
  const int r = role < NWG - 1 ? role - 2 * K + 1 : 0;  // the matrix row of this workgroup
  if (wave < K) {  // ------------------------------------------------------ SampleNTT A[r][wave]
    kg_pipe_sample<K>(sl, d, r, wave, c);
    SS_MARK(r == 0 && wave == 0 && lane == 0, 2);
  }
  if (r > 0) {  // ---------------------------------------------------------- row r's t_hat
    if (wave == 0) {
      kg_load_ops<K>(sl, scr, fl, r);
#pragma unroll
      for (int j = 0; j < K; ++j) kg_mark(sl, lds_wait_ge(&sl.prog[j], 256));
      // lane l: pairs l and l + 64
      uint32_t tb[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        tb[h] = kg_pipe_pair<K>(
            sl, p, [&](int j, int w, int L) { return sl.bop[j][w][L]; }, [&](int t, int L) { return sl.ef[t][L]; });
      }
      uint8_t* io8 = (uint8_t*)sl.io;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        io8[3 * p] = (uint8_t)tb[h];
        io8[3 * p + 1] = (uint8_t)(tb[h] >> 8);
        io8[3 * p + 2] = (uint8_t)(tb[h] >> 16);
      }
      wave_phase();
      if (role == late) kg_dbg_sleep();
      const uint32_t* io32 = (const uint32_t*)sl.io;
      for (int w = lane; w < 96; w += 64) st_sc1(&scr.th[r][w], io32[w]);
      kg_publish(&fl[8 + r]);
      SS_MARK(r == 1 && lane == 0, 19);
      for (int w = lane; w < 96; w += 64) {
        ((uint32_t*)(ek + 384 * r))[w] = io32[w];
        ((uint32_t*)(dk + 384 * K + 384 * r))[w] = io32[w];
      }
    }
    const bool e = wipe_lds();  // the s_hat / e_hat copies: wiped before the flag that ends this workgroup
    outputs_done(2 * K + r - 1, e);
    return;
  }
  // ------------------------------------------------------------------------ the collector (row 0)
  uint8_t* io8 = (uint8_t*)sl.io;
  if (wave == K) {  // t_hat_0 pairs as A[0][j] fills, then the other rows' t_hat
    kg_load_ops<K>(sl, scr, fl, 0);
    SS_MARK(lane == 0, 22);
    // pair ranges whose bytes complete H(ek) blocks 0, 1, 2: pair p is ek bytes 3p .. 3p + 2
    constexpr int LIM[4] = {0, 46, 91, 128};
#pragma unroll 1
    for (int b = 0; b < 3; ++b) {
#pragma unroll
      for (int j = 0; j < K; ++j) kg_mark(sl, lds_wait_ge(&sl.prog[j], 2 * LIM[b + 1]));
      const int p = LIM[b] + lane;
      if (p < LIM[b + 1]) {
        const uint32_t t = kg_pipe_pair<K>(
            sl, p, [&](int j, int w, int L) { return sl.bop[j][w][L]; }, [&](int t, int L) { return sl.ef[t][L]; });
        io8[3 * p] = (uint8_t)t;
        io8[3 * p + 1] = (uint8_t)(t >> 8);
        io8[3 * p + 2] = (uint8_t)(t >> 16);
      }
      lds_release_store(&sl.io_ready, 3 * LIM[b + 1]);
    }
    SS_MARK(lane == 0, 3);
    const uint32_t* io32 = (const uint32_t*)sl.io;
    for (int w = lane; w < 96; w += 64) {
      ((uint32_t*)ek)[w] = io32[w];
      ((uint32_t*)(dk + 384 * K))[w] = io32[w];
    }
    for (int rr = 1; rr < K; ++rr) {
      kg_mark(sl, kg_wait_flag(&fl[8 + rr]));
      const uint64_t* st = (const uint64_t*)&scr.th[rr][0];
      uint64_t v = 0;
      if (lane < 48) v = __hip_atomic_load((const gu64*)(st + lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane < 48) sl.io[48 * rr + lane] = v;
      lds_release_store(&sl.io_ready, 384 * (rr + 1));
    }
    SS_MARK(lane == 0, 5);
  } else if (wave == K + 1) {  // H(ek), block by block as ek's bytes arrive
    __builtin_amdgcn_s_setprio(3);
    const uint64_t zw = (i >= 0 && i < 4) ? d[4 + i] : 0;
    SS_MARK(lane == 0, 7);
    constexpr int RW = RW_SHA3_256, NW = PKB / 8, NFULL = NW / RW, TAIL = NW % RW;
    const bool rl = i >= 0 && i < RW;
    CState s;
#pragma unroll 1
    for (int b = 0; b < NFULL; ++b) {
      const int need = 8 * RW * (b + 1) < 384 * K ? 8 * RW * (b + 1) : 384 * K;
      kg_mark(sl, lds_wait_ge(&sl.io_ready, need));
      SS_MARK(lane == 0 && b < 4, 8 + (b == 0 ? 0 : b == 1 ? 5 : b == 2 ? 1 : 6));
      if (rl) cs_xor(s, sl.io[b * RW + i]);
      s = kf_coop(s, c);
    }
    // rho (ek's last 32 bytes, in the final partial block for every K) from SampleNTT wave 0's copy
    // of G's output: wave 0 wrote it before its first progress release, which the t_hat wave acquired
    // before it released io_ready (this wave computes no G of its own: one cooperative permutation
    // fewer beside the SampleNTT waves)
    kg_mark(sl, lds_wait_ge(&sl.io_ready, 384 * K));
    if (i >= 0 && i < 4 && coop_canon(c)) {
      const uint64_t rw = sl.rho[0][i];
      sl.io[48 * K + i] = rw;
      ((uint64_t*)(ek + 384 * K))[i] = rw;
      ((uint64_t*)(dk + 768 * K))[i] = rw;
    }
    wave_phase();
    if (rl && i < TAIL) cs_xor(s, sl.io[NFULL * RW + i]);
    if (i == TAIL) s.lo ^= DS_SHA3;
    if (i == RW - 1) s.hi ^= 0x80000000u;
    s = kf_coop(s, c);
    if (i >= 0 && i < 4 && coop_canon(c)) {
      uint64_t* tail = (uint64_t*)(dk + 768 * K + 32);
      tail[i] = cs_word(s);
      tail[4 + i] = zw;
    }
    __builtin_amdgcn_s_setprio(0);
    SS_MARK(lane == 0, 4);
  }
  // Completion, in key-hygiene order: this workgroup's outputs released; its LDS (which holds copies
  // of s_hat and e_hat_0) wiped; every other workgroup's outputs (and its last scratch / flag
  // access) done; the secret scratch (s_hat, e_hat) wiped and the flags reset; those stores drained;
  // the error word set if any wait of this handshake expired; and only then the completion ticket
  // stored for the host -- the ticket is the kernel's last act.
  if (done) __threadfence_system();
  const bool own_err = wipe_lds();
  __syncthreads();
  if (wave == 0) {
    const uint32_t* of[NWG - 1];
#pragma unroll
    for (int w = 0; w < NWG - 1; ++w) of[w] = &fl[16 + w];
    uint32_t seen = 0u;
    const bool all = kg_wait_flags<NWG - 1, false>(of, &seen);  // no payload read after it
    uint4* sw = (uint4*)&scr;
    for (int x = lane; x < (int)(offsetof(PipeScr, th) / 16); x += 64) sw[x] = make_uint4(0, 0, 0, 0);
    if (lane < KG_FLAGS) st_sc1(&fl[lane], 0u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SS_MARK(lane == 0, 6);
    if (lane == 0 && (own_err || !all || (seen & 2u)))
      __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (done && lane == 0) __hip_atomic_store(done, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ============================================================ host launchers

bool keygen_pipe_built() { return QRK_KG_PIPE; }
size_t keygen_scratch_bytes(size_t n) {
  return std::min(n, (size_t)QRK_KG_MULTI_MAX) * std::max(sizeof(MkScr), sizeof(PipeScr));
}

hipError_t keygen_pipe(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                       const Streams& s) {
  return with_rank(k, [&](auto rank) {
    constexpr int K = decltype(rank)::value;
    QRK_LAUNCH("k_keygen_pipe", s.main, k_keygen_pipe<K>, dim3((unsigned)(n * 3 * K)), dim3(64 * (K + 2)), 0, s.main, n,
               coins, pk, sk, (PipeScr*)scratch, s.kg_cnt, n == 1 ? s.done : nullptr, s.ticket, s.kg_err,
               g_kg_dbg_late.load(std::memory_order_relaxed));
    return launch_status();
  });
}

hipError_t keygen_multi(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                        const Streams& s) {
  return with_rank(k, [&](auto rank) {
    constexpr int K = decltype(rank)::value;
    QRK_LAUNCH("k_keygen_multi", s.main, k_keygen_multi<K>, dim3((unsigned)(n * (2 * K + K * K))), dim3(64), 0,
               s.main, n, coins, pk, sk, (MkScr*)scratch, s.kg_cnt, n == 1 ? s.done : nullptr, s.ticket);
    return launch_status();
  });
}

}  // namespace mlkem

size_t mlkem_kg_flag_words() { return (size_t)QRK_KG_MULTI_MAX * mlkem::KG_FLAGS; }
size_t mlkem_kg_scratch_bytes() { return mlkem::keygen_scratch_bytes(QRK_KG_MULTI_MAX); }
size_t mlkem_kg_multi_max() { return QRK_KG_MULTI_MAX; }
std::atomic<int> g_kg_dbg_late{-1};

}  // namespace qrk
