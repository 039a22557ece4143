// ML-KEM (FIPS 203): what every execution path shares -- the scratch layouts, the per-parameter-set
// sizes P<K> and the scratch carve-up.  Included by the host file (mlkem.hip) and by every path file.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "mlkem_arith.cuh"
#include "qrkem_internal.h"

namespace qrk {
namespace mlkem {

// (Q, the tables, the fp32 modular arithmetic, Compress / Decompress, gsync, the 12-bit splitting
// and decoding, CBD expansion, the fp32 NTTs and the basemul live in mlkem_arith.cuh.)
// The batched SampleNTT output holds 12-bit coefficients (384 B per matrix entry, 8 per 12-byte
// chunk) rather than int16 (512 B): the encrypt core waits on memory, not on the VALU (SQ wait_any
// 0.28-0.35 after the round-3 arithmetic cut its VALU instructions 20 % with no change in time), and
// the matrix is 58 % of its HBM reads.
constexpr int XOF_W = 48;    // u64 words per matrix entry in scratch
constexpr int PRF_W = 24;    // up to 192 B of PRF output (eta = 3)

// Tiled scratch layouts: word w of instance i at ((i / TW) W + w) TW + i % TW -- TW = 64 for the
// batched kernels (one coalesced wave store per word), 16 for the small path's LDS copies.
template <int TW = 64>
__device__ __forceinline__ size_t tidx(size_t inst, int w, int W) {
  return ((inst / TW) * (size_t)W + (size_t)w) * TW + (inst % TW);
}

// Tile units of two consecutive chunks (24 B): chunk pair p of entry i at ((i / TW) 16 + p) TW +
// i % TW, so a consumer lane's 16 coefficients are 24 contiguous bytes (one load pair instead of
// two 12-byte loads 768 B apart).  A/B on one box, four interleaved pairs
// (profiles/r3/final/ab_pair24.jsonl): encrypt core 1.97 -> 1.88 ms, fix-up 0.160 -> 0.103 ms per
// 2^20 launch, k_xof unchanged.
struct U6 {
  U3 h[2];
};
typedef U3 XChunk;
typedef U6 XUnit;
constexpr int XUNITS = 16;  // units per entry
// an entry's first unit, and chunk ch of it
template <int TW>
__device__ __forceinline__ XUnit* xent(XUnit* out, size_t inst) {
  return out + (inst / TW) * XUNITS * TW + (inst % TW);
}
template <int TW>
__device__ __forceinline__ XChunk* xc(XUnit* ent, int ch) {
  return &ent[(ch >> 1) * TW].h[ch & 1];
}

template <int K>
struct P {
  static constexpr int ETA1 = (K == 2) ? 3 : 2;
  static constexpr int ETA2 = 2;
  static constexpr int DU = (K == 4) ? 11 : 10;
  static constexpr int DV = (K == 4) ? 5 : 4;
  static constexpr int PK = 384 * K + 32;
  static constexpr int SK = 768 * K + 96;
  static constexpr int CT = 32 * (DU * K + DV);
};

// Scratch carve-up for a chunk of C handshakes
struct ScratchView {
  uint64_t *xof, *prf, *seeds, *mprime, *kprime, *kbar;
  uint32_t *fix, *nfix;  // SampleNTT fix-up list (entries needing > 3 blocks, capacity K^2 C), its counter
  uint64_t* rho;         // every handshake's rho, 32 B apart (k_rho_copy)
  uint32_t* hit;         // Decaps under a kept matrix: a word per handshake, 1 = its rho matched (k_rho_match)
};
__host__ __device__ inline size_t scratch_words(int K, size_t C) {
  return (size_t)K * K * C * XOF_W + (size_t)(2 * K + 1) * C * PRF_W + 16 * C + ((size_t)K * K * C + 16) / 2 + 4 +
         4 * C + C / 2;
}
inline ScratchView carve(void* base, int K, size_t C) {
  ScratchView v;
  uint64_t* p = (uint64_t*)base;
  v.xof = p;
  p += (size_t)K * K * C * XOF_W;
  v.prf = p;
  p += (size_t)(2 * K + 1) * C * PRF_W;
  v.seeds = p;
  p += 4 * C;
  v.mprime = p;
  p += 4 * C;
  v.kprime = p;
  p += 4 * C;
  v.kbar = p;
  p += 4 * C;
  v.nfix = (uint32_t*)p;
  v.fix = v.nfix + 16;
  p += ((size_t)K * K * C + 16) / 2 + 4;
  v.rho = p;
  p += 4 * C;
  v.hit = (uint32_t*)p;
  return v;
}

}  // namespace mlkem
}  // namespace qrk
