// SHA-256 and SHA-512 (FIPS 180-4) in registers, one message per lane, for gfx950.
//
// SHA-256: 8 state words + a 16-word rolling message schedule per lane; every rotate is one
// v_alignbit_b32, Ch/Maj are single v_bitop3.  SHA-512 is the same shape over 64-bit words: 80 rounds,
// 128-byte blocks, a 128-bit length field.  tail / tail512 compress the padded end of a byte stream.
// Users: hkdf.hip (HKDF-SHA256) and slhdsa.hip (SLH-DSA-SHA2 verification).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace qrk {
namespace sha {

struct K256T {
  uint32_t k[64];
};
constexpr K256T K256 = {{
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u}};

struct H8 {
  uint32_t h[8];
};
__device__ __forceinline__ H8 init() {
  return H8{{0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu,
             0x5be0cd19u}};
}

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }

// One SHA-256 compression of the 16 big-endian words w into s.
__device__ __forceinline__ void compress(H8& s, const uint32_t win[16]) {
  uint32_t w[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) w[t] = win[t];
  uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) {
      const uint32_t x = w[(t + 1) & 15], y = w[(t + 14) & 15];
      const uint32_t s0 = rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3);
      const uint32_t s1 = rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10);
      w[t & 15] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = h + S1 + ch + K256.k[t] + w[t & 15];
    const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
    const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + S0 + maj;
  }
  s.h[0] += a, s.h[1] += b, s.h[2] += c, s.h[3] += d;
  s.h[4] += e, s.h[5] += f, s.h[6] += g, s.h[7] += h;
}

// Compress the padded tail of a message whose first `prefix` bytes (a multiple of 64)
// are already in s and whose remaining `len` bytes are byte_at(0 .. len-1).
// word_over(b, t, w) may replace word t of tail block b (used for register-held data).
template <class ByteAt, class WordOver>
__device__ __forceinline__ void tail(H8& s, uint32_t prefix, uint32_t len, ByteAt byte_at, WordOver word_over) {
  const uint32_t nblk = (len + 9 + 63) / 64;
  const uint64_t bits = (uint64_t)(prefix + len) * 8;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      uint32_t x = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t pos = 64 * b + 4 * t + k;
        const uint32_t v = pos < len ? byte_at(pos) : (pos == len ? 0x80u : 0u);
        x = (x << 8) | v;
      }
      w[t] = word_over(b, t, x);
    }
    if (b == nblk - 1) {
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    compress(s, w);
  }
}

struct K512T {
  uint64_t k[80];
};
constexpr K512T K512 = {{
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
    0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
    0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
    0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
    0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
    0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
    0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
    0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
    0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
    0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
    0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
    0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull}};

struct H8x64 {
  uint64_t h[8];
};
__device__ __forceinline__ H8x64 init512() {
  return H8x64{{0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull}};
}

__device__ __forceinline__ uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// One SHA-512 compression of the 16 big-endian 64-bit words w into s.
__device__ __forceinline__ void compress512(H8x64& s, const uint64_t win[16]) {
  uint64_t w[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) w[t] = win[t];
  uint64_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
  for (int t = 0; t < 80; ++t) {
    if (t >= 16) {
      const uint64_t x = w[(t + 1) & 15], y = w[(t + 14) & 15];
      const uint64_t s0 = rotr64(x, 1) ^ rotr64(x, 8) ^ (x >> 7);
      const uint64_t s1 = rotr64(y, 19) ^ rotr64(y, 61) ^ (y >> 6);
      w[t & 15] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint64_t S1 = rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41);
    const uint64_t ch = (e & f) ^ (~e & g);
    const uint64_t t1 = h + S1 + ch + K512.k[t] + w[t & 15];
    const uint64_t S0 = rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39);
    const uint64_t maj = (a & b) ^ (a & c) ^ (b & c);
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + S0 + maj;
  }
  s.h[0] += a, s.h[1] += b, s.h[2] += c, s.h[3] += d;
  s.h[4] += e, s.h[5] += f, s.h[6] += g, s.h[7] += h;
}

// tail for SHA-512: `prefix` is a multiple of 128, word_over(b, t, w) may replace 64-bit word t of tail
// block b.  Streams stay below 2^32 bytes, so the upper 64 bits of the length field are zero.
template <class ByteAt, class WordOver>
__device__ __forceinline__ void tail512(H8x64& s, uint32_t prefix, uint32_t len, ByteAt byte_at, WordOver word_over) {
  const uint32_t nblk = (len + 17 + 127) / 128;
  const uint64_t bits = (uint64_t)(prefix + len) * 8;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; ++b) {
    uint64_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      uint64_t x = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t pos = 128 * b + 8 * t + k;
        const uint32_t v = pos < len ? byte_at(pos) : (pos == len ? 0x80u : 0u);
        x = (x << 8) | v;
      }
      w[t] = word_over(b, t, x);
    }
    if (b == nblk - 1) {
      w[14] = 0;
      w[15] = bits;
    }
    compress512(s, w);
  }
}

}  // namespace sha
}  // namespace qrk
