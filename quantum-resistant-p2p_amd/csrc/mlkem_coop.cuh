// ML-KEM (FIPS 203) on one wave: the wave-cooperative SampleNTT and PRF (keccak_coop.cuh, one sponge
// state per wave).  Shared by the one-launch path (mlkem_one.cuh), the single-shot KeyGens
// (mlkem_kg.cuh) and the batched path's cooperative SampleNTT fix-up (mlkem_batch.cuh).
#pragma once
#include "keccak_coop.cuh"
#include "mlkem_layout.cuh"

namespace qrk {
namespace mlkem {

// ordering between lanes of one wave across phases: a workgroup-scope release / acquire around
// a wave barrier
__device__ __forceinline__ void wave_phase() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// SampleNTT entry e = x K + y (FIPS 203 Alg. 7) on one wave: SHAKE128(rho || x || y) squeezed
// block by block; each block's 56 byte triples are parsed by lanes 0-55 (two candidates each)
// and the accepted ones placed by ballot prefix counts, so the wave keeps FIPS order:
// place(j, value) for coefficient j.  pbuf: this wave's 44-dword LDS parse buffer.  after_block(cnt):
// called with the running count of accepted values once a block's values are placed.
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};
template <int K, typename Place, typename Hook = NoHook>
__device__ __forceinline__ void xof_coop_place(const uint64_t* __restrict__ rho, int e, uint32_t* __restrict__ pbuf,
                                               const Coop& c, Place place, Hook after_block = Hook()) {
  const int i = c.idx, lane = threadIdx.x & 63;
  CState s;
  if (i >= 0 && i < 4) cs_xor(s, rho[i]);
  if (i == 4) s.lo ^= (uint32_t)(e / K) | ((uint32_t)(e % K) << 8) | (DS_SHAKE << 16);
  if (i == RW_SHAKE128 - 1) s.hi ^= 0x80000000u;
  int cnt = 0;
#pragma unroll 1
  while (cnt < 256) {  // wave-uniform
    s = kf_coop(s, c);
    if (i >= 0 && i < RW_SHAKE128) {
      pbuf[2 * i] = s.lo;
      pbuf[2 * i + 1] = s.hi;
    }
    wave_phase();
    uint32_t d1 = Q, d2 = Q;
    if (lane < 56) {
      const int b = 3 * lane;
      const uint32_t v = __builtin_amdgcn_alignbit(pbuf[(b >> 2) + 1], pbuf[b >> 2], 8 * (b & 3));
      d1 = v & 0xFFF;
      d2 = (v >> 12) & 0xFFF;
    }
    const bool a1 = d1 < (uint32_t)Q, a2 = d2 < (uint32_t)Q;
    const uint64_t m1 = __ballot(a1), m2 = __ballot(a2);
    const int pre = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0)) +
                    (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0));
    const int p1 = cnt + pre, p2 = p1 + (a1 ? 1 : 0);
    if (a1 && p1 < 256) place(p1, d1);
    if (a2 && p2 < 256) place(p2, d2);
    cnt += __popcll(m1) + __popcll(m2);
    wave_phase();  // this block's parse reads are done before the next block's pbuf writes
    after_block(cnt);
  }
}
// ... into the single-shot layout: coefficient j of entry e at int16 index ((j / 8) 16 + e) 8 + j % 8
// of xs16 (the k_xof layout at tile width 16)
template <int K>
__device__ __forceinline__ void xof_coop(const uint64_t* __restrict__ rho, int e, uint16_t* __restrict__ xs16,
                                         uint32_t* __restrict__ pbuf, const Coop& c) {
  xof_coop_place<K>(rho, e, pbuf, c,
                    [&](int j, uint32_t d) { xs16[(((j >> 3) * 16 + e) << 3) + (j & 7)] = (uint16_t)d; });
}

// PRF instance N on one wave: SHAKE256(seed || N) -> 64 eta bytes; word w at ps[w 16 + N].
template <int ETA>
__device__ __forceinline__ void prf_coop(const uint64_t* __restrict__ seed, int N, uint64_t* __restrict__ ps,
                                         const Coop& c) {
  const int i = c.idx;
  CState s;
  if (i >= 0 && i < 4) cs_xor(s, seed[i]);
  if (i == 4) s.lo ^= (uint32_t)N | (DS_SHAKE << 8);
  if (i == RW_SHAKE256 - 1) s.hi ^= 0x80000000u;
  s = kf_coop(s, c);
  if (ETA == 2) {
    if (i >= 0 && i < 16) ps[i * 16 + N] = cs_word(s);
  } else {
    if (i >= 0 && i < 17) ps[i * 16 + N] = cs_word(s);
    s = kf_coop(s, c);
    if (i >= 0 && i < 7) ps[(17 + i) * 16 + N] = cs_word(s);
  }
}

}  // namespace mlkem
}  // namespace qrk
