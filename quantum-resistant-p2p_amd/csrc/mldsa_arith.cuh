// ML-DSA (FIPS 204) device primitives for verification: arithmetic modulo q = 8380417, the NTTs over
// 256 coefficients in LDS, Decompose / UseHint, the bit unpackers, the two samplers, HintBitUnpack and
// w1Encode.  Everything here is a __forceinline__ device function or a constant: mldsa.hip includes
// this header for its kernels, and tests/mldsa_arith_probe.hip includes it to run each primitive alone
// over its documented domain.  All inputs of verification are public, so nothing here is constant-time
// (data-dependent branches, early exits): do not reuse these paths for signing.
//
// Representation.  q has 23 bits, so the exact-fp32 products of mlkem_arith.cuh (24-bit mantissa) do
// not carry over, and 32 x 32-bit integer products are not full rate on gfx950.  Coefficients are kept
// as signed 32-bit integers and the one modular product, modmul, runs in fp64: a product of two
// integers below 2^53 in magnitude is exact in a double, and so is the fused multiply-add that takes
// the multiple of q off.  Every bound below is on the magnitude of such integers.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace qrk {
namespace mldsa {

constexpr int Q = 8380417;
constexpr int D = 13;
constexpr int N = 256;
constexpr int ZETA = 1753;
constexpr int HALFQ = (Q + 1) / 2;  // 4190209: the bound of every modmul result
// flag word of a row (qrk_dbg_mldsa_verify_trace); FLAG_LONG is internal: the row has 2^31 bytes or more;
// FLAG_KEY (key-set calls, mldsa_keyed.hip): the row's key index is not below the number of keys in the set
constexpr uint32_t FLAG_HINT = 1, FLAG_NORM = 2, FLAG_HASH = 4, FLAG_LONG = 8, FLAG_KEY = 16;

struct Params {
  int k, l, tau, ctilde, zbits, gamma1, gamma2, omega, beta, w1bits;
  int pk, sk, sig;
  __host__ __device__ constexpr int hint_off() const { return sig - omega - k; }
  __host__ __device__ constexpr int w1_bytes() const { return k * 32 * w1bits; }
};
constexpr Params P44{4, 4, 39, 32, 18, 1 << 17, (Q - 1) / 88, 80, 78, 6, 1312, 2560, 2420};
constexpr Params P65{6, 5, 49, 48, 20, 1 << 19, (Q - 1) / 32, 55, 196, 4, 1952, 4032, 3309};
constexpr Params P87{8, 7, 60, 64, 20, 1 << 19, (Q - 1) / 32, 75, 120, 4, 2592, 4896, 4627};

// ---------------------------------------------------------------- tables
constexpr int powq(long b, int e) {
  long r = 1;
  for (; e; e >>= 1, b = b * b % Q)
    if (e & 1) r = r * b % Q;
  return (int)r;
}
constexpr int br8(int i) {
  int r = 0;
  for (int b = 0; b < 8; ++b) r |= ((i >> b) & 1) << (7 - b);
  return r;
}
constexpr int centered(long x) {
  x %= Q;
  if (x < 0) x += Q;
  return (int)(x > Q / 2 ? x - Q : x);
}
// zeta^br8(i) mod q, centered (|z| <= (q - 1) / 2), derived from zeta = 1753: as doubles, the form
// modmul takes its second factor in
struct Tables {
  double z[N];
};
constexpr Tables make_tables() {
  Tables t{};
  for (int i = 0; i < N; ++i) t.z[i] = (double)centered(powq(ZETA, br8(i)));
  return t;
}
__constant__ Tables TAB = make_tables();
constexpr double INV256 = (double)centered(powq(256, Q - 2));  // 256^-1 mod q = 8347681 = -32736

// ---------------------------------------------------------------- arithmetic
constexpr double QD = 8380417.0;
constexpr double QINVD = 1.0 / 8380417.0;
// a * b mod q, centered.  Domain: integers with |a * b| < 2^53 (b an exact integer in a double).
// p = a b is exact; k = rint(p / q) is off the true quotient by at most 1/2 + 2^-21 (the two
// roundings of p * fl(1 / q) are each below 2^-52 relative, |p / q| < 2^30); k q < 2^53 + 2^22, and
// p - k q, an integer below 2^23, comes out of one FMA exactly.  Range: |result| <= HALFQ.
__device__ __forceinline__ int modmul(int a, double b) {
  const double p = (double)a * b;
  const double k = __builtin_rint(p * QINVD);
  return (int)__builtin_fma(-k, QD, p);
}
// x mod q, centered, by the same route.  Domain: every int32.  Range: |result| <= HALFQ.
__device__ __forceinline__ int reduce(int x) { return modmul(x, 1.0); }
// x mod q in [0, q).  Domain: |x| < 2 q (every value the NTTs hand on is within HALFQ).
__device__ __forceinline__ int canon(int x) {
  x += (x >> 31) & Q;
  x += (x >> 31) & Q;
  const int y = x - Q;
  return y < 0 ? x : y;
}

// ---------------------------------------------------------------- NTT (Algorithms 41, 42)
// `polys` polynomials of 256 int coefficients, contiguous in LDS, transformed in place by all `nthr`
// threads of the workgroup (thread `tid`); every thread of the workgroup must call.
// Forward: Cooley-Tukey, no reduction between layers.  Input |x| <= B, output |X| <= B + 8 HALFQ
// (each layer adds one modmul result): for B < q that is below 5 q < 2^25.4, and the largest product a
// layer forms is (B + 7 HALFQ) (q - 1) / 2 < 2^48.
__device__ __forceinline__ void ntt_fwd(int* a, int polys, int tid, int nthr) {
  for (int len = 128; len >= 1; len >>= 1) {
    __syncthreads();
    for (int e = tid; e < polys * 128; e += nthr) {
      int* w = a + (e >> 7) * N;
      const int b = e & 127, blk = b / len, j = blk * 2 * len + (b & (len - 1));
      const int t = modmul(w[j + len], TAB.z[128 / len + blk]);
      const int u = w[j];
      w[j] = u + t;
      w[j + len] = u - t;
    }
  }
  __syncthreads();
}
// Inverse: Gentleman-Sande, output multiplied by 256^-1.  Input |x| < 2^30 (reduced on entry to
// HALFQ).  The sums double per layer: after layer i (1..8) |a| <= 2^i HALFQ < 2^30 at the end, and the
// differences that go into modmul are below 2^30 against twiddles below 2^22: products below 2^52.
// Output |x| <= HALFQ.
__device__ __forceinline__ void ntt_inv(int* a, int polys, int tid, int nthr) {
  __syncthreads();
  for (int e = tid; e < polys * N; e += nthr) a[e] = reduce(a[e]);
  for (int len = 1; len < N; len <<= 1) {
    __syncthreads();
    for (int e = tid; e < polys * 128; e += nthr) {
      int* w = a + (e >> 7) * N;
      const int nb = 128 / len;
      const int b = e & 127, blk = b / len, j = blk * 2 * len + (b & (len - 1));
      const int t = w[j], u = w[j + len];
      w[j] = t + u;
      w[j + len] = modmul(t - u, -TAB.z[2 * nb - 1 - blk]);
    }
  }
  __syncthreads();
  for (int e = tid; e < polys * N; e += nthr) a[e] = modmul(a[e], INV256);  // |a| <= 2^8 HALFQ, |256^-1| < 2^15
  __syncthreads();
}

// ---------------------------------------------------------------- Decompose / UseHint (Algorithms 36, 40)
// r in [0, q) -> (r1, r0) with r = r1 2 gamma2 + r0 (mod q), r0 in (-gamma2, gamma2], and the wrap
// r - r0 = q - 1 folded to r1 = 0, r0 - 1.  The quotient by 2 gamma2 is the round-3 reference's
// multiply-and-shift, exact on [0, q) (swept in full by the probe): (r + 127) >> 7 < 2^16, times
// 1025 or 11275 < 2^30.
template <int GAMMA2>
__device__ __forceinline__ void decompose(int r, int& r1, int& r0) {
  r1 = (r + 127) >> 7;
  if constexpr (GAMMA2 == (Q - 1) / 32) {
    r1 = (r1 * 1025 + (1 << 21)) >> 22;
    r1 &= 15;
  } else {
    r1 = (r1 * 11275 + (1 << 23)) >> 24;
    r1 ^= ((43 - r1) >> 31) & r1;
  }
  r0 = r - r1 * 2 * GAMMA2;
  r0 -= (((Q - 1) / 2 - r0) >> 31) & Q;
}
// h in {0, 1}, r in [0, q) -> the high bits the signer saw, in [0, m), m = (q - 1) / (2 gamma2)
template <int GAMMA2>
__device__ __forceinline__ int use_hint(int h, int r) {
  constexpr int M = (Q - 1) / (2 * GAMMA2);
  int r1, r0;
  decompose<GAMMA2>(r, r1, r0);
  if (!h) return r1;
  if (r0 > 0) return r1 + 1 == M ? 0 : r1 + 1;
  return r1 == 0 ? M - 1 : r1 - 1;
}

// ---------------------------------------------------------------- unpacking (Algorithms 17-19, 21)
// Coefficient i (0..255) of a polynomial packed at bits = 18 or 20 bits per coefficient starting at p:
// reads the three bytes that hold it (the bit offset within the first is even and at most 6, so the
// last coefficient ends with the polynomial's last byte and no read lies past it).
__device__ __forceinline__ uint32_t packed_coeff(const uint8_t* p, int bits, int i) {
  const int bit = i * bits, o = bit >> 3;
  const uint32_t v = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16);
  return (v >> (bit & 7)) & ((1u << bits) - 1);
}
// BitUnpack of z: gamma1 - value, in [-(gamma1 - 1), gamma1] for every input (zbits = 18 or 20)
__device__ __forceinline__ int z_coeff(const uint8_t* p, int zbits, int gamma1, int i) {
  return gamma1 - (int)packed_coeff(p, zbits, i);
}
// SimpleBitUnpack of t1 (10 bits) times 2^d: in [0, 1023 * 8192] = [0, q - 1]
__device__ __forceinline__ int t1_coeff_2d(const uint8_t* p, int i) {
  const int bit = i * 10, o = bit >> 3;
  const uint32_t v = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8);
  return (int)((v >> (bit & 7)) & 1023u) << D;
}
// HintBitUnpack, one thread: sets bit j of hbits[i * 8 + j / 32] for every hint (hbits: k * 8 words,
// zeroed by the caller) and returns false for a malformed encoding: a count below the running index or
// above omega, indices not strictly increasing within a polynomial, a nonzero byte after the last
// index.  y: omega + k bytes.  Index < y[omega + i] <= omega bounds every read of y.
__device__ __forceinline__ bool hint_unpack(const uint8_t* y, int k, int omega, uint32_t* hbits) {
  int index = 0;
  for (int i = 0; i < k; ++i) {
    const int cnt = y[omega + i];
    if (cnt < index || cnt > omega) return false;
    const int first = index;
    for (; index < cnt; ++index) {
      const int j = y[index];
      if (index > first && y[index - 1] >= j) return false;
      hbits[i * 8 + (j >> 5)] |= 1u << (j & 31);
    }
  }
  for (; index < omega; ++index)
    if (y[index]) return false;
  return true;
}

// ---------------------------------------------------------------- samplers (Algorithms 14, 29, 30)
// RejNTTPoly over a stream of SHAKE128 blocks (21 words = 56 candidates of three bytes, top bit
// dropped; a candidate below q is accepted).  next(w) delivers the next block, put(i, v) receives
// coefficient i = 0..255 in order, and after_block(total) runs after every block with the lanes of
// the wave converged (the loop ends when no lane of the wave needs another block, so after_block may
// use cross-lane operations).  The loop is general: a candidate is rejected with probability about
// 2^-10 and five blocks bring 280, so real seeds never need a sixth block; the probe reaches it with
// crafted bytes.  Returns the number of blocks this lane needed.
template <class Next, class Put, class After>
__device__ __forceinline__ int rej_ntt_poly(Next next, Put put, After after_block) {
  int total = 0, blocks = 0, used = 0;
  do {
    uint64_t w[21];
    next(w);
    ++blocks;
    if (total < N) used = blocks;
#pragma unroll
    for (int c = 0; c < 56; ++c) {
      const int bit = 24 * c, wi = bit >> 6, sh = bit & 63;
      uint32_t v = (uint32_t)(w[wi] >> sh);
      if (sh > 40) v |= (uint32_t)(w[wi + 1] << (64 - sh));
      v &= 0x7FFFFFu;
      if (v < (uint32_t)Q && total < N) {
        put(total, (int)v);
        ++total;
      }
    }
    after_block(total);
  } while (__any(total < N));
  return used;
}

// SampleInBall: c (256 int8 in LDS, one row per lane, zeroed here) gets tau entries of +-1.  The
// stream is SHAKE256(c~): next(buf) writes the next 136-byte block to this lane's LDS buffer.  The
// first 8 bytes are the sign bits; every later byte is a candidate index j, accepted when j <= i.  A
// second block is needed only when more than 128 candidates are used; the loop is general.  Returns
// the number of blocks used.
template <class Next>
__device__ __forceinline__ int sample_in_ball(int tau, int8_t* c, uint8_t* buf, Next next) {
  for (int i = 0; i < N; ++i) c[i] = 0;
  next(buf);
  int blocks = 1, pos = 8;
  uint64_t signs = 0;
  for (int i = 0; i < 8; ++i) signs |= (uint64_t)buf[i] << (8 * i);
  for (int i = N - tau; i < N; ++i) {
    int j;
    do {
      if (pos == 136) {
        next(buf);
        ++blocks;
        pos = 0;
      }
      j = buf[pos++];
    } while (j > i);
    c[i] = c[j];
    c[j] = (signs & 1) ? -1 : 1;
    signs >>= 1;
  }
  return blocks;
}

// ---------------------------------------------------------------- w1Encode (Algorithm 28)
// Byte `b` of one polynomial's encoding from its 256 high-bits values w (each below 2^bits).
// 6 bits: 192 bytes, byte b from coefficients 4 (b / 3) ..; 4 bits: 128 bytes, two coefficients each.
__device__ __forceinline__ uint8_t w1_byte(const uint8_t* w, int bits, int b) {
  if (bits == 4) return (uint8_t)(w[2 * b] | (w[2 * b + 1] << 4));
  const uint8_t* v = w + 4 * (b / 3);
  const uint32_t x = (uint32_t)v[0] | ((uint32_t)v[1] << 6) | ((uint32_t)v[2] << 12) | ((uint32_t)v[3] << 18);
  return (uint8_t)(x >> (8 * (b % 3)));
}

}  // namespace mldsa
}  // namespace qrk
