// Device functions of the AEAD kernels, shared by aead.hip (one lane per message) and aead_long.hip (one
// row across many workgroups): byte gathers, ChaCha20, Poly1305 in 26-bit limbs, AES-256 over the
// LDS-replicated T-table of aes.cuh, GHASH and the per-message GCM state.  The comment at the head of
// aead.hip says what each is for and why it is shaped as it is.
#pragma once
#include "aes.cuh"
#include "qrkem_internal.h"

namespace qrk {
namespace aead {

constexpr uint32_t NONCE = 12, TAG = 16, OVERHEAD = NONCE + TAG;
constexpr uint64_t ROW_MAX = (uint64_t)1 << 31;  // row lengths are 32-bit: longer rows are refused

__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, 32 - n); }
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_amdgcn_perm(0, x, 0x00010203u); }

// little-endian word of p[pos .. pos+4), bytes at or past len read as zero
__device__ __forceinline__ uint32_t gather32(const uint8_t* p, uint32_t pos, uint32_t len) {
  uint32_t x = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (pos + k < len) x |= (uint32_t)p[pos + k] << (8 * k);
  return x;
}
__device__ __forceinline__ void scatter32(uint8_t* p, uint32_t pos, uint32_t len, uint32_t x) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (pos + k < len) p[pos + k] = (uint8_t)(x >> (8 * k));
}
__device__ __forceinline__ uint32_t load32(const uint8_t* p) { return gather32(p, 0, 4); }

// One message's associated data: shared by all rows (off == NULL) or its own span.
struct Span {
  const uint8_t* p;
  uint32_t len;
  bool ok;
};
__device__ __forceinline__ Span span_of(const uint8_t* base, const uint64_t* off, uint32_t shared_len, size_t i) {
  if (!off) return Span{base, shared_len, true};
  const uint64_t a = off[i], l = off[i + 1] - a;
  return Span{base + a, (uint32_t)l, l < ROW_MAX};
}

// ------------------------------------------------------------------ ChaCha20 (RFC 8439 section 2.3)
struct ChaKey {
  uint32_t k[8], n[3];
};
__device__ __forceinline__ void quarter(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b, d = rotl(d ^ a, 16);
  c += d, b = rotl(b ^ c, 12);
  a += b, d = rotl(d ^ a, 8);
  c += d, b = rotl(b ^ c, 7);
}
__device__ __forceinline__ void chacha_block(const ChaKey& K, uint32_t ctr, uint32_t out[16]) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, K.k[0], K.k[1], K.k[2], K.k[3],
                     K.k[4],      K.k[5],      K.k[6],      K.k[7],      ctr,    K.n[0], K.n[1], K.n[2]};
  uint32_t x[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) x[t] = in[t];
#pragma unroll 1
  for (int r = 0; r < 10; ++r) {
    quarter(x[0], x[4], x[8], x[12]), quarter(x[1], x[5], x[9], x[13]);
    quarter(x[2], x[6], x[10], x[14]), quarter(x[3], x[7], x[11], x[15]);
    quarter(x[0], x[5], x[10], x[15]), quarter(x[1], x[6], x[11], x[12]);
    quarter(x[2], x[7], x[8], x[13]), quarter(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) out[t] = x[t] + in[t];
}
__device__ __forceinline__ ChaKey chacha_key(const uint8_t* key, const uint8_t* nonce) {
  ChaKey K;
#pragma unroll
  for (int t = 0; t < 8; ++t) K.k[t] = load32(key + 4 * t);
#pragma unroll
  for (int t = 0; t < 3; ++t) K.n[t] = load32(nonce + 4 * t);
  return K;
}

// ------------------------------------------------------------------ Poly1305 (RFC 8439 section 2.5)
// h, r in five 26-bit limbs; a block is h = (h + m) r mod 2^130 - 5 with partial carries, so the
// limbs stay below 2^27 and the five 64-bit column sums below 2^63.
struct Poly {
  uint32_t r[5], s5[4], h[5], pad[4];
  // key32 words: r (clamped here, section 2.5) then s
  __device__ __forceinline__ void init(const uint32_t k[8]) {
    r[0] = k[0] & 0x3ffffff;
    r[1] = ((k[0] >> 26) | (k[1] << 6)) & 0x3ffff03;
    r[2] = ((k[1] >> 20) | (k[2] << 12)) & 0x3ffc0ff;
    r[3] = ((k[2] >> 14) | (k[3] << 18)) & 0x3f03fff;
    r[4] = (k[3] >> 8) & 0x00fffff;
#pragma unroll
    for (int t = 0; t < 4; ++t) s5[t] = 5 * r[t + 1], pad[t] = k[4 + t];
#pragma unroll
    for (int t = 0; t < 5; ++t) h[t] = 0;
  }
  // m: 16 little-endian bytes (a short last block already carries its 0x01 byte); hibit = 2^128
  // for a full block (1 << 24 in the top limb), 0 for a short one
  __device__ __forceinline__ void block(const uint32_t m[4], uint32_t hibit) {
    const uint32_t h0 = h[0] + (m[0] & 0x3ffffff), h1 = h[1] + (((m[0] >> 26) | (m[1] << 6)) & 0x3ffffff),
                   h2 = h[2] + (((m[1] >> 20) | (m[2] << 12)) & 0x3ffffff),
                   h3 = h[3] + (((m[2] >> 14) | (m[3] << 18)) & 0x3ffffff), h4 = h[4] + ((m[3] >> 8) | hibit);
    auto mul = [](uint32_t a, uint32_t b) { return (uint64_t)a * b; };
    uint64_t d0 = mul(h0, r[0]) + mul(h1, s5[3]) + mul(h2, s5[2]) + mul(h3, s5[1]) + mul(h4, s5[0]);
    uint64_t d1 = mul(h0, r[1]) + mul(h1, r[0]) + mul(h2, s5[3]) + mul(h3, s5[2]) + mul(h4, s5[1]);
    uint64_t d2 = mul(h0, r[2]) + mul(h1, r[1]) + mul(h2, r[0]) + mul(h3, s5[3]) + mul(h4, s5[2]);
    uint64_t d3 = mul(h0, r[3]) + mul(h1, r[2]) + mul(h2, r[1]) + mul(h3, r[0]) + mul(h4, s5[3]);
    uint64_t d4 = mul(h0, r[4]) + mul(h1, r[3]) + mul(h2, r[2]) + mul(h3, r[1]) + mul(h4, r[0]);
    uint32_t c = (uint32_t)(d0 >> 26);
    h[0] = (uint32_t)d0 & 0x3ffffff;
    d1 += c, c = (uint32_t)(d1 >> 26), h[1] = (uint32_t)d1 & 0x3ffffff;
    d2 += c, c = (uint32_t)(d2 >> 26), h[2] = (uint32_t)d2 & 0x3ffffff;
    d3 += c, c = (uint32_t)(d3 >> 26), h[3] = (uint32_t)d3 & 0x3ffffff;
    d4 += c, c = (uint32_t)(d4 >> 26), h[4] = (uint32_t)d4 & 0x3ffffff;
    h[0] += c * 5, c = h[0] >> 26, h[0] &= 0x3ffffff;
    h[1] += c;
  }
  // Full carry, the final reduction (h >= p => h - p, selected with a mask) and tag = (h + s) mod 2^128.
  __device__ __forceinline__ void finish(uint32_t tag[4]) {
    uint32_t c = h[1] >> 26;
    h[1] &= 0x3ffffff;
    h[2] += c, c = h[2] >> 26, h[2] &= 0x3ffffff;
    h[3] += c, c = h[3] >> 26, h[3] &= 0x3ffffff;
    h[4] += c, c = h[4] >> 26, h[4] &= 0x3ffffff;
    h[0] += c * 5, c = h[0] >> 26, h[0] &= 0x3ffffff;
    h[1] += c;
    uint32_t g[5];
    g[0] = h[0] + 5, c = g[0] >> 26, g[0] &= 0x3ffffff;
    g[1] = h[1] + c, c = g[1] >> 26, g[1] &= 0x3ffffff;
    g[2] = h[2] + c, c = g[2] >> 26, g[2] &= 0x3ffffff;
    g[3] = h[3] + c, c = g[3] >> 26, g[3] &= 0x3ffffff;
    g[4] = h[4] + c - (1u << 26);
    const uint32_t ge = (g[4] >> 31) - 1;  // all ones iff h + 5 >= 2^130, i.e. h >= p
#pragma unroll
    for (int t = 0; t < 5; ++t) h[t] = (h[t] & ~ge) | (g[t] & ge);
    const uint32_t w0 = h[0] | (h[1] << 26), w1 = (h[1] >> 6) | (h[2] << 20), w2 = (h[2] >> 12) | (h[3] << 14),
                   w3 = (h[3] >> 18) | (h[4] << 8);
    uint64_t f = (uint64_t)w0 + pad[0];
    tag[0] = (uint32_t)f;
    f = (uint64_t)w1 + pad[1] + (f >> 32), tag[1] = (uint32_t)f;
    f = (uint64_t)w2 + pad[2] + (f >> 32), tag[2] = (uint32_t)f;
    f = (uint64_t)w3 + pad[3] + (f >> 32), tag[3] = (uint32_t)f;
  }
  // len bytes at p, zero-padded to a multiple of 16 (the AEAD's pad16: every block is full)
  __device__ __forceinline__ void absorb_padded(const uint8_t* p, uint32_t len) {
#pragma unroll 1
    for (uint32_t b = 0; b < len; b += 16) {
      uint32_t m[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) m[t] = gather32(p, b + 4 * t, len);
      block(m, 1u << 24);
    }
  }
};

// RFC 8439 section 2.8: tag = Poly1305(otk, aad | pad16 | ct | pad16 | le64(aad_len) | le64(ct_len)),
// otk = the first 32 bytes of ChaCha20 block 0 (section 2.6).
__device__ __forceinline__ void chacha_tag(const ChaKey& K, const Span& ad, const uint8_t* ct, uint32_t clen,
                                           uint32_t tag[4]) {
  uint32_t b0[16];
  chacha_block(K, 0, b0);
  Poly P;
  P.init(b0);
  P.absorb_padded(ad.p, ad.len);
  P.absorb_padded(ct, clen);
  const uint32_t lens[4] = {ad.len, 0, clen, 0};
  P.block(lens, 1u << 24);
  P.finish(tag);
}

// out[0 .. len) = in[0 .. len) ^ ChaCha20 keystream from block counter 1, ANDed with `keep`
// (all ones, or zero to write zeros instead of unauthenticated plaintext)
__device__ __forceinline__ void chacha_xor(const ChaKey& K, const uint8_t* in, uint8_t* out, uint32_t len,
                                           uint32_t keep) {
#pragma unroll 1
  for (uint32_t b = 0; b < len; b += 64) {
    uint32_t ks[16];
    chacha_block(K, 1 + b / 64, ks);
#pragma unroll
    for (int t = 0; t < 16; ++t) scatter32(out, b + 4 * t, len, (gather32(in, b + 4 * t, len) ^ ks[t]) & keep);
  }
}

// ------------------------------------------------------------------ AES-256 (FIPS 197) over Lds2
// SubWord through the replicated table: the S-box byte is byte 1 of T0 (round_last2's gather)
__device__ __forceinline__ uint32_t sub_word(const aes::Lds2& L, uint32_t w) {
  const uint32_t a = L.t0(w, 0), b = L.t0(w, 1), c = L.t0(w, 2), d = L.t0(w, 3);
  return __builtin_amdgcn_perm(b, a, 0x0C0C0501u) | __builtin_amdgcn_perm(d, c, 0x05010C0Cu);
}
// FIPS 197 section 5.2 with Nk = 8, Nr = 14: 60 round-key words (little-endian columns, as aes.cuh:
// RotWord = rotate right by 8, Rcon in byte 0)
__device__ __forceinline__ void expand_key256(const aes::Lds2& L, const uint32_t key[8], uint32_t rk[60]) {
  uint32_t rc = 1;
#pragma unroll
  for (int i = 0; i < 8; ++i) rk[i] = key[i];
#pragma unroll
  for (int i = 8; i < 60; ++i) {
    uint32_t t = rk[i - 1];
    if (i % 8 == 0) {
      t = sub_word(L, __builtin_amdgcn_alignbit(t, t, 8)) ^ rc;
      rc <<= 1;  // 7 doublings from 1: never reaches the reduction
    } else if (i % 8 == 4) {
      t = sub_word(L, t);
    }
    rk[i] = rk[i - 8] ^ t;
  }
}
__device__ __forceinline__ void encrypt256(const aes::Lds2& L, const uint32_t rk[60], uint32_t s[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) s[c] ^= rk[c];
#pragma unroll
  for (int r = 1; r < 14; ++r) aes::round_full2(L, s, rk + 4 * r);
  aes::round_last2(L, s, rk + 56);
}

// ------------------------------------------------------------------ GHASH (SP 800-38D section 6.4)
// Blocks as four big-endian words: bit 0 of the block (the coefficient of x^0) is the top bit of
// w[0].  y = y * h (section 6.3, Algorithm 1): 128 steps of z ^= v & -(bit i of y), v = v x, where
// v x is a right shift with R = 11100001 || 0^120 folded in under a mask.
__device__ __forceinline__ void gf128_mul(uint32_t y[4], const uint32_t h[4]) {
  uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0, v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t yw = y[w];
#pragma unroll 8
    for (int b = 31; b >= 0; --b) {
      const uint32_t m = 0u - ((yw >> b) & 1u);
      z0 ^= v0 & m, z1 ^= v1 & m, z2 ^= v2 & m, z3 ^= v3 & m;
      const uint32_t lsb = 0u - (v3 & 1u);
      v3 = __builtin_amdgcn_alignbit(v2, v3, 1);
      v2 = __builtin_amdgcn_alignbit(v1, v2, 1);
      v1 = __builtin_amdgcn_alignbit(v0, v1, 1);
      v0 = (v0 >> 1) ^ (lsb & 0xE1000000u);
    }
  }
  y[0] = z0, y[1] = z1, y[2] = z2, y[3] = z3;
}
// y = GHASH_h continued over len bytes at p, zero-padded to a multiple of 16
__device__ __forceinline__ void ghash_padded(uint32_t y[4], const uint32_t h[4], const uint8_t* p, uint32_t len) {
#pragma unroll 1
  for (uint32_t b = 0; b < len; b += 16) {
#pragma unroll
    for (int t = 0; t < 4; ++t) y[t] ^= bswap(gather32(p, b + 4 * t, len));
    gf128_mul(y, h);
  }
}

// Per-message GCM state: round keys, H = E_K(0^128), the IV words.
struct Gcm {
  uint32_t rk[60], h[4], iv[3];
  __device__ __forceinline__ void init(const aes::Lds2& L, const uint8_t* key, const uint8_t* nonce) {
    uint32_t k[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) k[t] = load32(key + 4 * t);
    expand_key256(L, k, rk);
    uint32_t z[4] = {0, 0, 0, 0};
    encrypt256(L, rk, z);
#pragma unroll
    for (int t = 0; t < 4; ++t) h[t] = bswap(z[t]);
#pragma unroll
    for (int t = 0; t < 3; ++t) iv[t] = load32(nonce + 4 * t);
  }
  // E_K(IV || be32(ctr)): ctr = 1 is J0 (section 7.1 step 2), the payload starts at inc32(J0) = 2
  __device__ __forceinline__ void counter_block(const aes::Lds2& L, uint32_t ctr, uint32_t out[4]) const {
    out[0] = iv[0], out[1] = iv[1], out[2] = iv[2], out[3] = bswap(ctr);
    encrypt256(L, rk, out);
  }
  // GCTR (section 6.5) from inc32(J0); `keep` as chacha_xor
  __device__ __forceinline__ void ctr_xor(const aes::Lds2& L, const uint8_t* in, uint8_t* out, uint32_t len,
                                          uint32_t keep) const {
#pragma unroll 1
    for (uint32_t b = 0; b < len; b += 16) {
      uint32_t ks[4];
      counter_block(L, 2 + b / 16, ks);
#pragma unroll
      for (int t = 0; t < 4; ++t) scatter32(out, b + 4 * t, len, (gather32(in, b + 4 * t, len) ^ ks[t]) & keep);
    }
  }
  // T = E_K(J0) ^ GHASH_H(aad | pad | ct | pad | be64(8 aad_len) | be64(8 ct_len)) (section 7.1 steps 5-6),
  // as four little-endian words of the tag bytes
  __device__ __forceinline__ void tag(const aes::Lds2& L, const Span& ad, const uint8_t* ct, uint32_t clen,
                                      uint32_t out[4]) const {
    uint32_t y[4] = {0, 0, 0, 0};
    ghash_padded(y, h, ad.p, ad.len);
    ghash_padded(y, h, ct, clen);
    y[0] ^= ad.len >> 29, y[1] ^= ad.len << 3, y[2] ^= clen >> 29, y[3] ^= clen << 3;
    gf128_mul(y, h);
    counter_block(L, 1, out);
#pragma unroll
    for (int t = 0; t < 4; ++t) out[t] ^= bswap(y[t]);
  }
};

#define QRK_AEAD_LDS_TABLE()                                                   \
  __shared__ __attribute__((aligned(16))) uint32_t tab[256 * 64];              \
  aes::fill_lds2(tab, threadIdx.x, 256);                                       \
  __syncthreads();                                                             \
  const aes::Lds2 L{(const char*)tab, (uint32_t)(threadIdx.x & 31) * 4u, 128u + (uint32_t)(threadIdx.x & 31) * 4u}

}  // namespace aead
}  // namespace qrk
