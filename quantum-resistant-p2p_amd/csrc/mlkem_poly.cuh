// ML-KEM (FIPS 203) polynomial I/O of a 16-lane group: loading CBD words, bit-packed encodings and
// sampled matrix entries, packing and flushing results, ByteEncode / ByteDecode_12 -- and the
// K-PKE.Decrypt core, which the batched path (mlkem_batch.cuh) and the one-launch Decaps
// (mlkem_one.cuh) both run.
#pragma once
#include "mlkem_layout.cuh"

namespace qrk {
namespace mlkem {

// ============================================================ 16-lane polynomial groups

struct P16 {
  int v[16];
};

// Per-group LDS: a padded 272-dword polynomial image (index j -> j + j/16, so both
// the stride image [L + 16m] and the contiguous image [16L + t] are conflict-free)
// plus 84 words of byte staging (raw XOF blocks, bit-packed encodings).
constexpr int PBUF = 272;
// 44 words of byte staging hold the largest packed polynomial (du = 11: 352 bytes).  The
// group stride is 368 dwords = 16 (mod 32): the two 16-lane groups that share a ds_* bank
// half (lanes 0-31 / 32-63) then use disjoint bank sets for every access pattern above.
constexpr int RAWW = 44;
// (Aliasing the byte staging onto the polynomial image -- 1088 B per group instead of 1472 -- was
// only needed by the rejected LDS-DMA matrix prefetch)
struct GroupLds {
  int poly[PBUF];
  uint64_t raw[RAWW];
  int pad[8];
};
static_assert(sizeof(GroupLds) / 4 % 32 == 16, "group stride must be 16 mod 32 dwords");
constexpr int GROUPS = 16;  // 256 threads

// The PRF words of one CBD polynomial (expanded by cbd_f, mlkem_arith.cuh)
template <int ETA, int TW = 64>
__device__ __forceinline__ CbdRaw cbd_load(const uint64_t* __restrict__ prf, size_t inst, int L) {
  CbdRaw r;
  if constexpr (ETA == 2) {
    const uint64_t w = prf[tidx<TW>(inst, L, PRF_W)];
    r.d[0] = (uint32_t)w, r.d[1] = (uint32_t)(w >> 32), r.d[2] = 0;
  } else {
    const int wi = (3 * L) >> 1;
    const uint64_t a = prf[tidx<TW>(inst, wi, PRF_W)], b = prf[tidx<TW>(inst, wi + 1, PRF_W)];
    const bool odd = L & 1;
    r.d[0] = odd ? (uint32_t)(a >> 32) : (uint32_t)a;
    r.d[1] = odd ? (uint32_t)b : (uint32_t)(a >> 32);
    r.d[2] = odd ? (uint32_t)(b >> 32) : (uint32_t)b;
  }
  return r;
}

// A group's 16*D*2 bytes at src (4-byte aligned) as this lane's share of dwords (L, L + 16, ...),
// loaded ahead of load_bits_r; DL <= D reads a shorter (DL-bit) encoding into the same shape.
template <int D>
struct RawW {
  uint32_t w[(8 * D + 15) / 16];
};
template <int D, int DL = D>
__device__ __forceinline__ RawW<D> raw_load(const uint8_t* __restrict__ src, int L) {
  RawW<D> r;
  const uint32_t* s32 = (const uint32_t*)src;
#pragma unroll
  for (int i = 0; i < (8 * D + 15) / 16; ++i) {
    const int idx = L + 16 * i;
    r.w[i] = idx < 8 * DL ? s32[idx] : 0u;
  }
  return r;
}
// Group-cooperative stage of 16*D*2 bytes (already loaded, raw_load) into the raw stage, then lane
// L unpacks its 16 D-bit fields (bits 16*D*L ...).
template <int D, int DX>
__device__ __forceinline__ void load_bits_r(P16& p, const RawW<DX>& r, GroupLds& g, int L) {
  constexpr int NDW = 8 * D;  // dwords for 256 D-bit values
  uint32_t* st = (uint32_t*)g.raw;
#pragma unroll
  for (int i = 0; i < (NDW + 15) / 16; ++i) {
    const int idx = L + 16 * i;
    if (idx < NDW) st[idx] = r.w[i];
  }
  gsync();
  // this lane's 2D bytes start at byte 2*D*L
  const int b0 = 2 * D * L;
  uint32_t w[8];
  const uint16_t* st16 = (const uint16_t*)g.raw;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    // assemble dwords from halfwords (2D bytes = D halfwords)
    const uint32_t h = st16[(b0 >> 1) + j];
    if (j & 1)
      w[j >> 1] |= h << 16;
    else
      w[j >> 1] = h;
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int bit = D * t;
    const int i = bit >> 5, sh = bit & 31;
    uint32_t v = w[i] >> sh;
    if (sh + D > 32) v |= w[i + 1] << (32 - sh);
    p.v[t] = (int)(v & ((1u << D) - 1));
  }
  gsync();
}
template <int D>
__device__ __forceinline__ void load_bits(P16& p, const uint8_t* __restrict__ src, GroupLds& g, int L) {
  load_bits_r<D>(p, raw_load<D>(src, L), g, L);
}

// Pack lane L's 16 D-bit fields into the raw stage at byte 2*D*L (whole group: 32*D bytes).
template <int D>
__device__ __forceinline__ void pack_bits(const P16& p, GroupLds& g, int L) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int bit = D * t;
    const int i = bit >> 5, sh = bit & 31;
    const uint32_t v = (uint32_t)p.v[t];
    w[i] |= v << sh;
    if (sh + D > 32) w[i + 1] |= v >> (32 - sh);
  }
  uint16_t* st16 = (uint16_t*)g.raw;
  const int h0 = D * L;
#pragma unroll
  for (int j = 0; j < D; ++j) st16[h0 + j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
  gsync();
}

// Store the packed stage (8*D dwords) to dst; or, when cmp != nullptr, OR the
// XOR with cmp into diff instead (Decaps re-encryption compare).
template <int D>
__device__ __forceinline__ void flush_bits(GroupLds& g, uint8_t* dst, const uint8_t* cmp, uint32_t& diff,
                                           bool active, int L) {
  constexpr int NDW = 8 * D;
  const uint32_t* st = (const uint32_t*)g.raw;
#pragma unroll
  for (int i = 0; i < (NDW + 15) / 16; ++i) {
    const int idx = L + 16 * i;
    if (idx < NDW) {
      const uint32_t v = st[idx];
      if (cmp)
        diff |= v ^ ((const uint32_t*)cmp)[idx];
      else if (active)
        ((uint32_t*)dst)[idx] = v;
    }
  }
  gsync();
}

// Decaps compare with the received ciphertext words loaded ahead of time (cmp_load):
// the global-load latency hides behind the row's NTT work instead of stalling the flush.
template <int D>
struct CmpWords {
  uint32_t w[(8 * D + 15) / 16];
};
template <int D>
__device__ __forceinline__ CmpWords<D> cmp_load(const uint8_t* cmp, int L) {
  CmpWords<D> r;
#pragma unroll
  for (int i = 0; i < (8 * D + 15) / 16; ++i) {
    const int idx = L + 16 * i;
    r.w[i] = idx < 8 * D ? ((const uint32_t*)cmp)[idx] : 0u;
  }
  return r;
}
template <int D>
__device__ __forceinline__ void flush_cmp(GroupLds& g, const CmpWords<D>& c, uint32_t& diff, int L) {
  const uint32_t* st = (const uint32_t*)g.raw;
#pragma unroll
  for (int i = 0; i < (8 * D + 15) / 16; ++i) {
    const int idx = L + 16 * i;
    if (idx < 8 * D) diff |= st[idx] ^ c.w[i];
  }
  gsync();
}

// SampleNTT consumer: lane L loads coefficients 16L..16L+15 (chunks 2L, 2L+1)
// of the producer's compacted output -- contiguous layout, no parsing.
template <int TW = 64, bool P12 = false>
__device__ __forceinline__ PK8 load_sampled(const void* __restrict__ xs_, size_t inst, int L) {
  if constexpr (P12) {
    const XUnit* base = xent<TW>((XUnit*)xs_, inst);
    const U6 u = base[L * TW];
    return unpack12(u.h[0], u.h[1]);
  } else {
    const uint4* base = (const uint4*)xs_ + (inst / TW) * 32 * TW + (inst % TW);
    const uint4 u = base[(2 * L) * TW], v = base[(2 * L + 1) * TW];
    return PK8{{u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w}};
  }
}
// the batched cores' view of the SampleNTT output
#define LOAD_XOF(TW_, inst) load_sampled<(TW_) == 64 ? XTW : (TW_), (TW_) == 64>(xof, (inst), L)

// ByteDecode_12 (decode12_w, mlkem_arith.cuh) of lane L's 24 bytes of a 384-byte polynomial
__device__ __forceinline__ PK8 decode12(const uint8_t* __restrict__ src, bool& bad, int L) {
  const uint64_t* s = (const uint64_t*)(src + 24 * L);
  return decode12_w(s[0], s[1], s[2], bad);
}

__device__ __forceinline__ void encode12(const P16& p, uint8_t* dst, int L) {
  uint32_t w[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) w[i] = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int bit = 12 * t, i = bit >> 5, sh = bit & 31;
    const uint32_t v = (uint32_t)p.v[t];
    w[i] |= v << sh;
    if (sh + 12 > 32) w[i + 1] |= v >> (32 - sh);
  }
  uint64_t* d = (uint64_t*)(dst + 24 * L);
  d[0] = ((uint64_t)w[1] << 32) | w[0];
  d[1] = ((uint64_t)w[3] << 32) | w[2];
  d[2] = ((uint64_t)w[5] << 32) | w[4];
}

__device__ __forceinline__ uint32_t group_or(uint32_t x) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) x |= __shfl_xor(x, d, 16);
  return x;
}

// ------------------------------------------------------------ K-PKE.Decrypt core
template <int K, int TW = 64>
__device__ __forceinline__ void decrypt_core_hs(size_t n, const uint8_t* __restrict__ ct,
                                                      const uint8_t* __restrict__ sk, uint64_t* __restrict__ mprime, size_t hs_raw, int L, GroupLds& g) {
  constexpr int DU = P<K>::DU, DV = P<K>::DV;
  const bool active = hs_raw < n;
  const size_t hs = active ? hs_raw : n - 1;
  const uint8_t* c = ct + (TW == 64 ? hs : 0) * P<K>::CT;  // the small path passes LDS copies
  const uint8_t* dk = sk + (TW == 64 ? hs : 0) * P<K>::SK;
  int acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0;
  bool bad = false;
#pragma unroll 1
  for (int j = 0; j < K; ++j) {
    // s_hat_j's 24 bytes per lane, issued before the NTT that precedes their use
    const uint2* e = (const uint2*)(dk + 384 * j + 24 * L);
    const uint2 da = e[0], db = e[1], dc = e[2];
    P16 u;
    load_bits<DU>(u, c + 32 * DU * j, g, L);
    PF16 uf;
#pragma unroll
    for (int t = 0; t < 16; ++t) uf.v[t] = i2f(decompress<DU>(u.v[t]));
    contig_to_stride_f(uf, (float*)g.poly, L);
    ntt_fwd_f<true>(uf, (float*)g.poly, L);
    basemul_acc(acc,
                decode12_w(((uint64_t)da.y << 32) | da.x, ((uint64_t)db.y << 32) | db.x, ((uint64_t)dc.y << 32) | dc.x, bad),
                make_bop_f(uf, L));
  }
  PF16 w;
#pragma unroll
  for (int t = 0; t < 16; ++t) w.v[t] = acc_to_f(acc[t]);
  ntt_inv_f(w, (float*)g.poly, L);
  stride_to_contig_f(w, (float*)g.poly, L);
  P16 v;
  load_bits<DV>(v, c + 32 * DU * K, g, L);
  uint32_t bits = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    bits |= (uint32_t)compress_f<1>(i2f(decompress<DV>(v.v[t])) - w.v[t]) << t;
  }
  if (active) ((uint16_t*)(mprime + (TW == 64 ? hs : 0) * 4))[L] = (uint16_t)bits;
}

}  // namespace mlkem
}  // namespace qrk
