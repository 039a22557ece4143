// ML-KEM device primitives: the fp32 modular arithmetic, tables, Compress / Decompress, 12-bit
// decoding, CBD expansion, the fp32 NTTs and the base-case multiplication that the kernels of
// mlkem.hip are built from.  Everything here is a __forceinline__ device function or a constant:
// mlkem.hip includes this header for its kernels, and tests/mlkem_arith_probe.hip includes it to
// run each primitive alone over its documented domain.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace qrk {
namespace mlkem {

constexpr int Q = 3329;

// ---------------------------------------------------------------- tables
constexpr int powq(int b, int e) {
  long r = 1;
  for (int i = 0; i < e; ++i) r = (r * b) % Q;
  return (int)r;
}
constexpr int br7(int i) {
  int r = 0;
  for (int b = 0; b < 7; ++b) r |= ((i >> b) & 1) << (6 - b);
  return r;
}
constexpr int centered(long x) {
  x %= Q;
  if (x < 0) x += Q;
  return (int)(x > Q / 2 ? x - Q : x);
}

// Plain-domain twiddles as fp32 (centered integers, exact): the NTTs run in fp32.  zq is z
// divided by q (rounded to fp32) for the three-FMA modular product below.
struct TablesF {
  float z[128];  // zeta^br7(i) mod q
  float g[128];  // gamma_i = zeta^(2 br7(i) + 1) mod q
  float zq[128];
};
constexpr TablesF make_tables_f() {
  TablesF t{};
  for (int i = 0; i < 128; ++i) {
    t.z[i] = (float)centered(powq(17, br7(i)));
    t.g[i] = (float)centered(powq(17, 2 * br7(i) + 1));
    t.zq[i] = (float)((double)t.z[i] / 3329.0);
  }
  return t;
}
constexpr TablesF TABFC = make_tables_f();
__constant__ TablesF TABFD = make_tables_f();
constexpr float INV128F = (float)centered(3303);  // 128^-1 mod q (plain domain) = -26
// zeta_1 * 128^-1: the inverse NTT's last layer folds the 128^-1 scaling into its twiddle
constexpr float Z1INV128F = (float)centered((long)powq(17, br7(1)) * 3303);

// ---------------------------------------------------------------- arithmetic
// x < 0 ? -1 : 0 as one v_ashrrev_i32 (inline asm, so the compiler keeps the mask arithmetic
// instead of turning it back into v_cmp + v_cndmask_e64, whose SGPR lane mask costs a VOP3
// issue and hazard wait states)
__device__ __forceinline__ int sign_mask(int x) {
  int r;
  asm("v_ashrrev_i32 %0, 31, %1" : "=v"(r) : "v"(x));
  return r;
}
// ---- fp32 modular arithmetic (every value is an exact integer below 2^24)
// MAGIC = 1.5 * 2^23: x + MAGIC rounds x to an integer (round-to-nearest-even), and
// for |x| < 2^22 the bit pattern of x + MAGIC is 0x4B400000 + x, so its low 16 bits
// are x as int16.  All ops below are full-rate on gfx950 (v_mul/v_add/v_fmaak/v_fmamk
// _f32), unlike the 24/32-bit integer multiplies (half rate).
constexpr float QF = 3329.0f;
constexpr float QINVF = 1.0f / 3329.0f;
constexpr float MAGIC = 12582912.0f;
// p - t q.  (Forcing v_fmamk_f32 with a literal -q through inline asm, in place of the v_fmac_f32
// the compiler picks at ~0.65 of the full rate, made the cores 7-10 % slower: hazard s_nops and
// lost v_pk_fma_f32 pairing, profiles/r3/ab_fmamk_rejected_and_wrap_probe.jsonl.)
__device__ __forceinline__ float fms_q(float t, float p) {  // p - t q
  return __builtin_fmaf(t, -QF, p);
}
// The modular product / reduction as three FMAs with MAGIC folded into the constants (below), where
// the round-2 form spent a product, a rounding FMA, the MAGIC subtraction and an FMA.
// MAGIC * q = 9987 * 2^22, exact in fp32
constexpr float MQF = MAGIC * QF;
// x mod q, centered: |result| <= 1665 for |x| < 2^24 (|x / q - rint| <= 1/2 + 3e-4)
// Three-FMA form: k = x/q + MAGIC rounds to MAGIC + kint (the binade [2^23, 2^24) has ulp 1);
// fma(k, -q, MAGIC q) = -q kint exactly (|q kint| < 2^24 for |x| <= 1.677e7); x + that is exact.
__device__ __forceinline__ float reduce_f(float x) {
  const float k = __builtin_fmaf(x, QINVF, MAGIC);
  return x + __builtin_fmaf(k, -QF, MQF);
}
// x * z mod q, centered, exact when |x * z| < 2^24 (for |z| <= 1664: |x| < 10082).
// zq = fl(z / q).  Three FMAs: k = MAGIC + round(x zq) (|x zq - x z / q| < 3e-4, so the
// result stays within q/2 + 1), n = -q round(.) exactly, then x z + n with one rounding of an
// exact integer below 2^24.  The round-2 form spent a product, the MAGIC
// subtraction and a three-VGPR fmac (0.65 of the full rate, profiles/r1/valu_peak_r1b.json).
__device__ __forceinline__ float modmul_f(float x, float z, float zq) {
  const float k = __builtin_fmaf(x, zq, MAGIC);
  return __builtin_fmaf(x, z, __builtin_fmaf(k, -QF, MQF));
}
// The same product for lane-indexed twiddles (the NTT layers after the transpose, basemul gamma)
// stays on the round-2 form: its single constant per twiddle holds fewer live registers than z
// and z / q together.  The three-FMA form there (z / q from a table or from z * (1/q)) cost the
// encrypt core a wave per SIMD (170 VGPRs: 2.64 against 2.29 ms per 2^20 launch) and the decrypt
// core one too (106 against 91 VGPRs: 0.95 against 0.90 ms), profiles/r3/ab_core_arith_*.jsonl.
__device__ __forceinline__ float modmul_lf(float x, float z) {
  const float p = x * z;
  const float t = __builtin_fmaf(p, QINVF, MAGIC) - MAGIC;
  return fms_q(t, p);
}
__device__ __forceinline__ float i2f(int x) {  // |x| < 2^22
  return __int_as_float(0x4B400000 + x) - MAGIC;
}
__device__ __forceinline__ int f2i(float x) {  // exact integer, |x| < 2^22
  return __float_as_int(x + MAGIC) - 0x4B400000;
}
__device__ __forceinline__ uint32_t f2bits(float x) {  // low 16 bits = x as int16
  return __float_as_uint(x + MAGIC);
}
// canonical [0, q) integer of an exact fp32 integer
__device__ __forceinline__ int canon_f(float x) {
  const int r = f2i(reduce_f(x));
  return r + (sign_mask(r) & Q);
}
// basemul accumulator -> centered residue: acc = hi 2^16 + lo (hi = acc >> 16, 0 <= lo < 2^16) with
// 2^16 = -1044 (mod q), then one reduction of lo - 1044 hi.
// With HI = MAGIC + hi and LO = MAGIC + lo as bit patterns (no MAGIC subtractions),
// fma(HI, -1044, 1043 MAGIC) = -MAGIC - 1044 hi is exact (a multiple of 4 below 2^25) and adding LO
// leaves lo - 1044 hi exactly: two full-rate ops where the round-2 form spent two subtractions
// and a three-VGPR fmac.
// Domain: |lo - 1044 hi| must stay below 2^24 (the sum's exactness and reduce_f's domain), which
// holds for -16007 <= hi <= 16070, i.e. -1 049 034 752 <= acc <= 1 053 229 056 -- NOT all of int32:
// the first wrong results are at acc = +1 053 229 057 and -1 049 034 753.  The kernels stay below
// 3.11e8 (basemul_acc); tests/test_gpu_mlkem_arith.py sweeps every |acc| <= 2^29 on the device.
__device__ __forceinline__ float acc_to_f(int acc) {
  const float hi = __int_as_float(0x4B400000 + (acc >> 16)), lo = __int_as_float(0x4B400000 | (acc & 0xFFFF));
  return reduce_f(__builtin_fmaf(hi, -1044.0f, 1043.0f * MAGIC) + lo);
}

// Compress_d(x) = round(2^d x / q) mod 2^d for x in [0, q): exact via 24-bit mulhi
template <int D>
__device__ __forceinline__ int compress(int x) {
  const uint32_t y = ((uint32_t)x << D) + (Q / 2);
  return (int)(__umulhi(y, 1290168u) & ((1u << D) - 1));
}
// Compress_d of any exact fp32 integer v congruent to x mod q, |v| <= 4091 (no reduction first):
// fma(v, fl(2^d / q), MAGIC) rounds v 2^d / q to an integer whose low d bits are
// round(x 2^d / q) mod 2^d (adding q to v adds 2^d).  Correct rounding: v 2^(d+1) is even and
// (2k + 1) q odd, so v 2^d / q is at least 1 / (2q) = 1.5e-4 from every half-integer, and the
// constant's relative error 2^-24 moves it by at most 2517 * 2^-24 < 1.5e-4 for
// |v 2^d / q| <= 2517.  Two full-rate ops where canon_f + compress spent about twelve.
template <int D>
__device__ __forceinline__ int compress_f(float v) {
  constexpr float C = (float)((double)(1 << D) / 3329.0);
  return (int)(__float_as_uint(__builtin_fmaf(v, C, MAGIC)) & ((1u << D) - 1));
}
template <int D>
__device__ __forceinline__ int decompress(int y) {
  return (int)(((uint32_t)Q * (uint32_t)y + (1u << (D - 1))) >> D);
}

// 16-lane group synchronisation: a group never spans two waves, so ordering
// LDS traffic inside the wave is enough.
__device__ __forceinline__ void gsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 8 consecutive 12-bit fields of the little-endian 96-bit string w0|w1|w2
__device__ __forceinline__ void split12(uint32_t w0, uint32_t w1, uint32_t w2, int c[8]) {
  c[0] = (int)(w0 & 0xFFF);
  c[1] = (int)((w0 >> 12) & 0xFFF);
  c[2] = (int)(__builtin_amdgcn_alignbit(w1, w0, 24) & 0xFFF);
  c[3] = (int)((w1 >> 4) & 0xFFF);
  c[4] = (int)((w1 >> 16) & 0xFFF);
  c[5] = (int)(__builtin_amdgcn_alignbit(w2, w1, 28) & 0xFFF);
  c[6] = (int)((w2 >> 8) & 0xFFF);
  c[7] = (int)(w2 >> 20);
}

// One 8-coefficient chunk of the batched SampleNTT output: 12 bytes of 12-bit fields.
struct U3 {
  uint32_t x, y, z;
};

// ---- fp32 NTTs (plain domain).  Same data movement as the integer versions above.
struct PF16 {
  float v[16];
};

__device__ __forceinline__ void stride_to_contig_f(PF16& p, float* buf, int L) {
#pragma unroll
  for (int m = 0; m < 16; ++m) buf[L + 17 * m] = p.v[m];
  gsync();
#pragma unroll
  for (int t = 0; t < 16; ++t) p.v[t] = buf[17 * L + t];
  gsync();
}
__device__ __forceinline__ void contig_to_stride_f(PF16& p, float* buf, int L) {
#pragma unroll
  for (int t = 0; t < 16; ++t) buf[17 * L + t] = p.v[t];
  gsync();
#pragma unroll
  for (int m = 0; m < 16; ++m) p.v[m] = buf[L + 17 * m];
  gsync();
}

// FIPS 203 Alg. 9 in fp32.  In: stride layout (v[m] = f[L+16m]), |f| <= B0.
// Out: contiguous layout (v[t] = f[16L+t]).  Each layer adds at most 1665 to the
// bound and a layer's twiddle products must stay below 2^24 (|input| < 10082):
// B0 <= 3 (CBD) -> 3 + 6 * 1665 = 9993 before the last layer, output <= 11658.
// MIDRED (inputs up to q, e.g. decompressed u): reduce everything after layer 4;
// output <= 4 * 1665.
template <bool MIDRED>
__device__ __forceinline__ void ntt_fwd_f(PF16& p, float* buf, int L) {
#pragma unroll
  for (int lg = 0; lg < 4; ++lg) {
    const int step = 8 >> lg;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if (((m / step) & 1) == 0) {
        const int zi = (1 << lg) + m / (2 * step);
        const float t = modmul_f(p.v[m + step], TABFC.z[zi], TABFC.zq[zi]);
        p.v[m + step] = p.v[m] - t;
        p.v[m] = p.v[m] + t;
      }
    }
  }
  if (MIDRED) {
#pragma unroll
    for (int m = 0; m < 16; ++m) p.v[m] = reduce_f(p.v[m]);
  }
  stride_to_contig_f(p, buf, L);
  {
    const float z = TABFD.z[16 + L];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float u = modmul_lf(p.v[t + 8], z);
      p.v[t + 8] = p.v[t] - u;
      p.v[t] = p.v[t] + u;
    }
  }
  {
    const float z0 = TABFD.z[32 + 2 * L], z1 = TABFD.z[33 + 2 * L];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (((t >> 2) & 1) == 0) {
        const float u = modmul_lf(p.v[t + 4], t < 8 ? z0 : z1);
        p.v[t + 4] = p.v[t] - u;
        p.v[t] = p.v[t] + u;
      }
    }
  }
  {
    float z[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) z[s] = TABFD.z[64 + 4 * L + s];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (((t >> 1) & 1) == 0) {
        const float u = modmul_lf(p.v[t + 2], z[t >> 2]);
        p.v[t + 2] = p.v[t] - u;
        p.v[t] = p.v[t] + u;
      }
    }
  }
}

// FIPS 203 Alg. 10 in fp32 (including the 128^-1 scaling).  In: contiguous, |f| <= 1665.
// Out: stride layout, |f| <= 1665.  Gentleman-Sande sums double per layer; the sums of
// every second layer are reduced, so |y - x| <= 6660 at every twiddle product.  The last
// layer folds the scaling in: x + y times 128^-1 = -26 and y - x times
// zeta_1 128^-1, instead of a separate product for all 16 outputs.
__device__ __forceinline__ void ntt_inv_f(PF16& p, float* buf, int L) {
  {
    float z[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) z[s] = TABFD.z[127 - 4 * L - s];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (((t >> 1) & 1) == 0) {
        const float x = p.v[t], y = p.v[t + 2];
        p.v[t] = x + y;
        p.v[t + 2] = modmul_lf(y - x, z[t >> 2]);
      }
    }
  }
  {
    const float z0 = TABFD.z[63 - 2 * L], z1 = TABFD.z[62 - 2 * L];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (((t >> 2) & 1) == 0) {
        const float x = p.v[t], y = p.v[t + 4];
        p.v[t] = reduce_f(x + y);
        p.v[t + 4] = modmul_lf(y - x, t < 8 ? z0 : z1);
      }
    }
  }
  {
    const float z = TABFD.z[31 - L];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float x = p.v[t], y = p.v[t + 8];
      p.v[t] = x + y;
      p.v[t + 8] = modmul_lf(y - x, z);
    }
  }
  contig_to_stride_f(p, buf, L);
#pragma unroll
  for (int lg = 3; lg >= (1 ? 1 : 0); --lg) {
    const int step = 8 >> lg;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if (((m / step) & 1) == 0) {
        const int zi = (2 << lg) - 1 - m / (2 * step);
        const float x = p.v[m], y = p.v[m + step];
        p.v[m] = ((lg & 1) == 1) ? reduce_f(x + y) : x + y;  // layers 4 and 6 reduce their sums
        p.v[m + step] = modmul_f(y - x, TABFC.z[zi], TABFC.zq[zi]);
      }
    }
  }
  // layer 7 (step 8, zeta_1) with the scaling: |x + y|, |y - x| <= 2 * 6660, far inside the
  // modmul_f bound for the small factors
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float x = p.v[m], y = p.v[m + 8];
    p.v[m] = modmul_f(x + y, INV128F, (float)(INV128F / 3329.0));
    p.v[m + 8] = modmul_f(y - x, Z1INV128F, (float)(Z1INV128F / 3329.0));
  }
}

// ---- base-case multiplication (FIPS 203 Alg. 11/12) on packed int16 pairs
// A coefficient pair (a0, a1) lives in one dword (lo, hi) -- exactly the
// producer's sampled layout.  For the other operand b we precompute
//   B0 = (b0, b1*gamma)   and   B1 = (b1, b0)
// so that  c0 = a0 b0 + a1 b1 gamma = dot2(A, B0),  c1 = a0 b1 + a1 b0 = dot2(A, B1):
// two v_dot2c_i32_i16 per pair, accumulated unreduced over the k terms.
typedef short v2s __attribute__((ext_vector_type(2)));

struct PK8 {  // 16 coefficients as 8 packed int16 pairs (contiguous layout)
  uint32_t w[8];
};
struct BOp {  // basemul right operand
  uint32_t b0[8], b1[8];
};

__device__ __forceinline__ uint32_t pack16(int lo, int hi) {
  return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u);
}

// From an fp32 NTT output (|b| <= 11658, fits int16): B0 = (b0, b1 gamma mod q),
// B1 = (b1, b0).  b1 is reduced before the gamma product to keep it below 2^24.
__device__ __forceinline__ BOp make_bop_f(const PF16& b, int L) {
  BOp r;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const uint32_t e0 = f2bits(b.v[2 * u]), e1 = f2bits(b.v[2 * u + 1]);
    const uint32_t g = f2bits(modmul_lf(reduce_f(b.v[2 * u + 1]), TABFD.g[8 * L + u]));
    r.b0[u] = pack16((int)e0, (int)g);
    r.b1[u] = pack16((int)e1, (int)e0);
  }
  return r;
}

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, a), __builtin_bit_cast(v2s, b), c, false);
}

// acc += a o b  (a in [0, q), b centered: |b| <= 11658 from ntt_fwd_f, |b1 gamma| <= 1665).  One
// term adds at most 2 * 3328 * 11658 = 7.76e7, so |acc| <= 3.11e8 (2^28.2) for k <= 4 terms: inside
// int32 and inside acc_to_f's domain (1.049e9).
__device__ __forceinline__ void basemul_acc(int acc[16], const PK8& a, const BOp& b) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    acc[2 * u] = dot2(a.w[u], b.b0[u], acc[2 * u]);
    acc[2 * u + 1] = dot2(a.w[u], b.b1[u], acc[2 * u + 1]);
  }
}

// Split CBD: the PRF words are loaded first (so a caller can prefetch them one
// stage ahead) and expanded straight to fp32.
struct CbdRaw {
  uint32_t d[3];
};
// eta = 2 in SWAR form: per nibble (a0 a1 b0 b1), x holds a0+a1 and b0+b1 in two bit
// pairs, y = (a0+a1) + 4 - (b0+b1) per nibble (no borrow), coefficient = nibble - 4,
// built as an fp32 directly (0x4B400000 | nibble is 2^23 * 1.5 + nibble).
template <int ETA>
__device__ __forceinline__ void cbd_f(PF16& p, const CbdRaw& r) {
  if constexpr (ETA == 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t d = r.d[h];
      const uint32_t x = (d & 0x55555555u) + ((d >> 1) & 0x55555555u);
      const uint32_t y = (x & 0x33333333u) + 0x44444444u - ((x >> 2) & 0x33333333u);
#pragma unroll
      for (int t = 0; t < 8; ++t)
        p.v[8 * h + t] = __uint_as_float(((y >> (4 * t)) & 0xFu) | 0x4B400000u) - (MAGIC + 4.0f);
    }
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int bit = 6 * t, i = bit >> 5, sh = bit & 31;
      uint32_t f = r.d[i] >> sh;
      if (sh + 6 > 32) f |= r.d[i + 1] << (32 - sh);
      f &= 0x3F;
      p.v[t] = i2f((int)__popc(f & 7u) - (int)__popc(f & 0x38u));
    }
  }
}

// The batched producer's 12-bit chunks, spread back to int16 pairs: a pair is 24
// consecutive bits x, (x & 0xFFF) | (x << 4 & 0x0FFF0000) -- about 3 VALU per pair.
__device__ __forceinline__ PK8 unpack12(const U3& u, const U3& v) {
  const uint32_t w[6] = {u.x, u.y, u.z, v.x, v.y, v.z};
  PK8 r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t a = w[3 * h], b = w[3 * h + 1], c = w[3 * h + 2];
    const uint32_t x[4] = {a, __builtin_amdgcn_alignbit(b, a, 24), __builtin_amdgcn_alignbit(c, b, 16), c >> 8};
#pragma unroll
    for (int k = 0; k < 4; ++k) r.w[4 * h + k] = (x[k] & 0xFFFu) | ((x[k] << 4) & 0x0FFF0000u);
  }
  return r;
}

// ByteDecode_12 (reduced mod q) of a 384-byte NTT-domain polynomial into packed
// pairs; `bad` collects the FIPS 203 section 7.2 modulus-check failure.
// ByteDecode_12 of this lane's 24 bytes already in registers (a, b, c little-endian)
__device__ __forceinline__ PK8 decode12_w(uint64_t a, uint64_t b, uint64_t c, bool& bad) {
  int v[16];
  split12((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, v);
  split12((uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), v + 8);
  PK8 r;
  // unsigned min(v, v - q) is v mod q for v < 2q (v - q wraps when v < q); the largest
  // coefficient decides the modulus check (two full-rate ops and one max, no lane masks)
  uint32_t mx = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const uint32_t u = (uint32_t)v[t];
    mx = u > mx ? u : mx;
    v[t] = (int)__builtin_elementwise_min(u, u - (uint32_t)Q);
  }
  bad |= mx >= (uint32_t)Q;
#pragma unroll
  for (int u = 0; u < 8; ++u) r.w[u] = pack16(v[2 * u], v[2 * u + 1]);
  return r;
}

}  // namespace mlkem
}  // namespace qrk
