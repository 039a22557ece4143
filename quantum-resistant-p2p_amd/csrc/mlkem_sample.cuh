// ML-KEM (FIPS 203) sampling, one lane per Keccak instance: SampleNTT with its compaction into the
// 12-bit tile layout, and the PRF producer.  Used by the batched path (mlkem_batch.cuh).
#pragma once
#include "keccak.cuh"
#include "mlkem_layout.cuh"

namespace qrk {
namespace mlkem {

// ============================================================ lane-per-instance Keccak kernels

// SampleNTT (FIPS 203 Alg. 7), one lane per matrix entry: SHAKE128(rho || x || y)
// squeezed block by block until 256 values < q have been accepted (3 blocks
// with probability ~0.993, rarely 4).  Compaction happens in the producer:
// every candidate is written to a 16-entry per-lane LDS ring at the running
// count (a rejected one is simply overwritten by the next), and each completed
// 8-coefficient chunk is flushed as one 16-byte store.  The ring is
// lane-interleaved (entry i of lane l at dword i*64 + l of the wave's ring), so
// every lane always hits its own LDS bank: the random per-lane write offsets
// never conflict.  Output: 256 int16 coefficients per entry in a 64-entry tiled
// layout of 12-bit chunks (see XUnit, mlkem_layout.cuh), so the consumer reads them without any
// parsing.  inst = (x*K + y) * C + hs.
constexpr int MAX_XOF_BLOCKS = 16;

// Rejected SampleNTT acceptance forms (A/B on one box, no faster than v_cmp + v_cndmask): a sign
// mask (three full-rate ops, profiles/r2/ab_xof_signmask_rejected.jsonl) and a shifted difference
// advancing the ring position by (c - q) >> 23 (profiles/r2/ab_xof_acc_rejected.jsonl).

// (a & m) | b as one v_bitop3_b32 (truth table 0xEA): full rate on gfx950, where
// v_and_or_b32 issues at half rate (profiles/r1/valu_peak_r1b.json)
__device__ __forceinline__ uint32_t and_or3(uint32_t a, uint32_t m, uint32_t b) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(r) : "v"(a), "s"(m), "v"(b));
  return r;
}

// r[j]: the chunk's coefficients (< 2^12, from the ring)
__device__ __forceinline__ void chunk_store(XChunk* dst, const uint32_t r[8]) {
  U3 w;
  w.x = r[0] | (r[1] << 12) | (r[2] << 24);
  w.y = (r[2] >> 8) | (r[3] << 4) | (r[4] << 16) | (r[5] << 28);
  w.z = (r[5] >> 4) | (r[6] << 8) | (r[7] << 20);
  *dst = w;
}
struct XofPend {
  uint32_t r[8];  // the chunk's ring entries, in order
  int ch = -1;    // its chunk index, -1: nothing pending
};
template <int TW = 64>
__device__ __forceinline__ void xof_pend_store(XofPend& pd, XUnit* dst) {
  if (pd.ch >= 0) {
    chunk_store(xc<TW>(dst, pd.ch), pd.r);
    pd.ch = -1;
  }
}

// Compact one squeezed SHAKE128 block (112 candidates) into the lane's ring,
// flushing completed 8-coefficient chunks to dst.
// `rb` = byte offset of the lane's ring column inside ring_all (wave * 4096 + lane * 4): bits
// 8-11 are zero, so an entry address is one v_bitop3_b32, (pos & 0xF00) | rb, with the static
// LDS base folded into the ds_write offset.
// A completed chunk's 8 ring entries are read when it completes and packed + stored one triplet
// later (or after the block), so the LDS read latency is not waited for on the spot (-1.5 %,
// profiles/r2/ab_xof_pipe_flush.jsonl).
template <int TW = 64>
__device__ __forceinline__ void compact_block(const KState& s, char* ring_all, uint32_t rb, int& cnt, XUnit* dst,
                                              XofPend& pd) {
  const uint32_t* ring = (const uint32_t*)(ring_all + rb);
#pragma unroll
  for (int t = 0; t < 14; ++t) {  // 42 dwords = 14 triplets of 8 twelve-bit candidates
    uint32_t d[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int di = 3 * t + e;
      d[e] = (di & 1) ? s.a[di >> 1].hi : s.a[di >> 1].lo;
    }
    int c[8];
    split12(d[0], d[1], d[2], c);
    const int before = cnt;
    // cnt kept pre-scaled by 256 (the byte stride of one ring entry): per candidate
    // one and + add for the address and cmp + cndmask + add for the count
    int pos = cnt << 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      *(uint32_t*)(ring_all + and_or3(pos, 0xF00u, rb)) = (uint32_t)c[e];
      pos += c[e] < Q ? 256 : 0;
    }
    cnt = pos >> 8;
    const int ch = before >> 3;
    // the chunk completed one triplet ago: its ring reads were issued then, so they have
    // landed by now (a wave's LDS instructions execute in issue order, so the reads saw the
    // chunk before this triplet's writes could reuse its slots)
    xof_pend_store<TW>(pd, dst);
    if ((cnt >> 3) != ch && ch < 32) {
      const uint32_t* r = ring + (ch & 1) * 8 * 64;
#pragma unroll
      for (int j = 0; j < 8; ++j) pd.r[j] = r[j * 64];
      pd.ch = ch;
    }
  }
}

// Fix-up entries are recomputed from scratch.  (Resume records -- the sponge state, count and
// partial chunk saved after the 3rd block, so the fix-up needs one more permutation -- cut the
// fix-up from 0.35 to 0.25 ms but slowed k_xof 1.8 %: no net gain, profiles/r2/ab_xof_resume.jsonl.)
// Tile width 64 makes k_xof's stores one contiguous KB per wave; width 1 (each entry contiguous)
// sped the encrypt core up 4 % but slowed k_xof's scattered stores 4-8 % (net -2 %,
// profiles/r2/ab_xof_tile_width.jsonl).
constexpr int XTW = 64;

__device__ __forceinline__ void xof_init(KState& s, const uint64_t* __restrict__ rho, int xy, int K) {
  kzero(s);
#pragma unroll
  for (int w = 0; w < 4; ++w) kxor(s, w, rho[w]);
  s.a[4].lo ^= (uint32_t)(xy / K) | ((uint32_t)(xy % K) << 8) | (DS_SHAKE << 16);
  s.a[RW_SHAKE128 - 1].hi ^= 0x80000000u;
}

// squeeze + compact blocks: exactly NB of them (ALL = false), or until 256 values (ALL = true)
template <bool ALL, int NB, int TW = 64>
__device__ __forceinline__ void xof_blocks(KState& s, int& cnt, XUnit* __restrict__ dst, char* ring_all, uint32_t rb) {
  XofPend pd;
#pragma unroll 1
  for (int b = 0; b < NB && (!ALL || cnt < 256); ++b) {
    // the main pass is throughput-bound (a lane per matrix entry), where the carry form of theta's
    // rot-1 is the faster one; the fix-up is a wave or so per SIMD and keeps the funnel shifts
    if constexpr (ALL) keccak_f(s);
    else keccak_f_carry(s);
    compact_block<TW>(s, ring_all, rb, cnt, dst, pd);
  }
  xof_pend_store<TW>(pd, dst);
}

// One SampleNTT entry inst = (x K + y) C + hs from scratch: SHAKE128(rho || x || y), ALL = false:
// exactly 3 blocks (returns the count, < 256 when a 4th block is needed); ALL = true: as many
// blocks as it takes.  rb = this lane's ring column (see compact_block).
template <int K, bool ALL, int TW = 64>
__device__ __forceinline__ int xof_entry(const uint64_t* __restrict__ rho, int xy, size_t inst, XUnit* __restrict__ out,
                                         char* ring_all, uint32_t rb) {
  XUnit* dst = xent<TW>(out, inst);
  KState s;
  xof_init(s, rho, xy, K);
  int cnt = 0;
  xof_blocks<ALL, ALL ? MAX_XOF_BLOCKS : 3, TW>(s, cnt, dst, ring_all, rb);
  return cnt;
}

// FIX == false: every entry squeezes exactly 3 blocks (uniform across the wave); the ~0.7 % that
// still lack 256 values go on the fix-up list.
// FIX == true: one lane per slot completes the entry (rewriting identical chunks on the
// from-scratch path), so the rare 4th block never idles a whole wave.
template <int K, bool FIX>
struct XofArgs {
  const uint8_t* rho_base;
  size_t rho_stride, n, C;
  XUnit* out;
  uint32_t *fix, *nfix;  // the fix-up list and its counter
  uint32_t* zero_other;  // main pass (chunks <= DIRECT_RHO_MAX): the counter the next call counts into
  // main pass of a Decaps chunk under a kept matrix: per-handshake hit words (k_rho_match), a lane whose
  // row hit has nothing to sample; NULL: every entry is sampled
  const uint32_t* hit = nullptr;
};
// block vb of nvb (FIX: the grid-stride walk over the list uses nvb)
template <int K, bool FIX>
__device__ __forceinline__ void xof_body(const XofArgs<K, FIX>& a, unsigned vb, unsigned nvb, uint32_t* ring_all) {
  const uint32_t rb = ((threadIdx.x >> 6) * 16 * 64 + (threadIdx.x & 63)) * 4;  // ring_all: [wave][16][64]
  char* ring = (char*)ring_all;
  if constexpr (!FIX) {
    if (vb == 0 && threadIdx.x == 0 && a.zero_other) *a.zero_other = 0u;
    const size_t e = (size_t)vb * 256 + threadIdx.x, hs = e % a.C;
    if (e >= (size_t)K * K * a.C || hs >= a.n) return;
    if (a.hit && a.hit[hs]) return;  // rho is public
    const int xy = (int)(e / a.C);
    const size_t inst = (size_t)xy * a.C + hs;
    KState s;
    xof_init(s, (const uint64_t*)(a.rho_base + hs * a.rho_stride), xy, K);
    int cnt = 0;
    xof_blocks<false, 3, XTW>(s, cnt, xent<XTW>(a.out, inst), ring, rb);
    if (cnt < 256) a.fix[atomicAdd(a.nfix, 1u)] = (uint32_t)inst;
  } else {
    const size_t stride = (size_t)nvb * 256, limit = (size_t)*a.nfix;
#pragma unroll 1
    for (size_t r = (size_t)vb * 256 + threadIdx.x; r < limit; r += stride) {
      const size_t inst = a.fix[r];
      xof_entry<K, true, XTW>((const uint64_t*)(a.rho_base + (inst % a.C) * a.rho_stride), (int)(inst / a.C), inst,
                              a.out, ring, rb);
    }
  }
}
constexpr int XOF_LDS = 4 * 16 * 64 * 4;  // the 256-thread block's compaction rings

// PRF producer: SHAKE256(seed || N) -> 64*eta bytes; inst = N * C + hs.
// eta = (N < eta1_upto) ? ETA1 : ETA2.
template <int ETA1, int ETA2, int TW = 64>
__device__ __forceinline__ void prf_inst(const uint64_t* __restrict__ seed, int N, size_t inst, int eta1_upto,
                                         uint64_t* __restrict__ prf) {
  const int eta = N < eta1_upto ? ETA1 : ETA2;
  KState s;
  kzero(s);
#pragma unroll
  for (int w = 0; w < 4; ++w) kxor(s, w, seed[w]);
  s.a[4].lo ^= (uint32_t)N | (DS_SHAKE << 8);
  s.a[RW_SHAKE256 - 1].hi ^= 0x80000000u;
  keccak_f(s);
  if (eta == 2) {
#pragma unroll
    for (int w = 0; w < 16; ++w) prf[tidx<TW>(inst, w, PRF_W)] = kword(s, w);
  } else {
#pragma unroll
    for (int w = 0; w < 17; ++w) prf[tidx<TW>(inst, w, PRF_W)] = kword(s, w);
    keccak_f(s);
#pragma unroll
    for (int w = 0; w < 7; ++w) prf[tidx<TW>(inst, 17 + w, PRF_W)] = kword(s, w);
  }
}

}  // namespace mlkem
}  // namespace qrk
