// 64-bit shift rates on gfx950 and a Keccak-f[1600] whose rotations use them.
//
// Every 64-bit rotation in keccak.cuh is two v_alignbit_b32 (half rate on gfx950,
// profiles/r1/valu_peak_r1b.json).  If v_lshlrev_b64 / v_lshrrev_b64 issue at full rate, a
// rotation becomes one 64-bit shift (the half that needs no merge) + one 32-bit shift + one
// OR: 3 issue slots instead of 4.  This probe measures the shift rates, the permutation rate
// of both variants with the state in registers, and checks the variant bit-exact against
// keccak_f on random states.
//
// Second question (profiles/keccak_rot/probe.json): does every rotation half need a funnel shift?
// rot-1 (five in theta, one in rho) is x + x with the carry wrapped round, three v_add_co/v_addc_co
// with SGPR-pair carries; offsets 8 and 56 are byte permutations, one v_perm_b32 per half.  The
// probe measures those instructions' issue rates next to v_alignbit_b32 and v_xor_b32, then the
// permutation loop in five forms, interleaved: (a) funnel shifts throughout (qrk::keccak_f),
// (b) carry rot-1, (c) v_perm for 8 and 56, (d) both, (e) theta's five rot-1 as one hand-scheduled
// carry statement (qrk::keccak_f_carry), each bit-exact against (a) on 4096 states before it is
// timed.
//
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/rot64_probe tools/rot64_probe.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../quantum-resistant-p2p_amd/csrc/keccak.cuh"

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      return 1;                                                               \
    }                                                                         \
  } while (0)

constexpr int ITERS = 4096;

#define MK64(NAME, INSTR)                                                                     \
  __global__ void k_##NAME(uint32_t* out, uint32_t seed) {                                  \
    uint64_t a0 = seed + threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 9,   \
             a5 = a0 * 11, a6 = a0 * 13, a7 = a0 * 15, b = seed;                            \
    for (int i = 0; i < ITERS; ++i) {                                                        \
      asm volatile(INSTR : "+v"(a0) : "v"(b)); asm volatile(INSTR : "+v"(a1) : "v"(b));      \
      asm volatile(INSTR : "+v"(a2) : "v"(b)); asm volatile(INSTR : "+v"(a3) : "v"(b));      \
      asm volatile(INSTR : "+v"(a4) : "v"(b)); asm volatile(INSTR : "+v"(a5) : "v"(b));      \
      asm volatile(INSTR : "+v"(a6) : "v"(b)); asm volatile(INSTR : "+v"(a7) : "v"(b));      \
    }                                                                                        \
    out[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)(a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7); \
  }
MK64(lshlrev_b64, "v_lshlrev_b64 %0, 7, %0 ; %1")
MK64(lshrrev_b64, "v_lshrrev_b64 %0, 7, %0 ; %1")
MK64(lshl_add_u64, "v_lshl_add_u64 %0, %0, 3, %1")
MK64(mov_b64, "v_mov_b64 %0, %1 ; %0")
MK64(pk_mov_b32, "v_pk_mov_b32 %0, %0, %1 op_sel:[0,1]")

// ---------------------------------------------------------------- 32-bit issue rates
// Eight independent chains per lane, like MK64.  STMT(a, c) is one instruction on chain value a
// with c the chain's own SGPR-pair carry; b is a per-lane operand, sel a v_perm selector in an SGPR.
#define MK32(NAME, STMT)                                                                       \
  __global__ void k_##NAME(uint32_t* out, uint32_t seed) {                                   \
    uint32_t a0 = seed + threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 9,    \
             a5 = a0 * 11, a6 = a0 * 13, a7 = a0 * 15, b = seed * 0x9E3779B9u + threadIdx.x; \
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;                 \
    const uint32_t sel = 0x06050403u;                                                         \
    for (int i = 0; i < ITERS; ++i) {                                                         \
      STMT(a0, c0) STMT(a1, c1) STMT(a2, c2) STMT(a3, c3)                                     \
      STMT(a4, c4) STMT(a5, c5) STMT(a6, c6) STMT(a7, c7)                                     \
    }                                                                                         \
    (void)sel;                                                                                \
    out[blockIdx.x * blockDim.x + threadIdx.x] =                                              \
        a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7 ^ (uint32_t)(c0 ^ c1 ^ c2 ^ c3 ^ c4 ^ c5 ^ c6 ^ c7); \
  }
#define I_XOR(a, c) asm volatile("v_xor_b32 %0, %1, %0" : "+v"(a) : "v"(b));
#define I_ALIGNBIT(a, c) asm volatile("v_alignbit_b32 %0, %0, %1, 7" : "+v"(a) : "v"(b));
#define I_PERM(a, c) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a) : "v"(b), "s"(sel));
#define I_ALIGNBYTE(a, c) asm volatile("v_alignbyte_b32 %0, %0, %1, 1" : "+v"(a) : "v"(b));
#define I_ADD_U32(a, c) asm volatile("v_add_u32 %0, %1, %0" : "+v"(a) : "v"(b));
// "+s": each chain keeps a carry pair of its own; sharing one draws an s_nop between statements
#define I_ADD_CO_S(a, c) asm volatile("v_add_co_u32 %0, %1, %0, %2" : "+v"(a), "+s"(c) : "v"(b));
#define I_ADDC_CO_S(a, c) asm volatile("v_addc_co_u32 %0, %1, %0, %2, %1" : "+v"(a), "+s"(c) : "v"(b));
MK32(xor_b32, I_XOR)
MK32(alignbit_b32, I_ALIGNBIT)
MK32(perm_b32, I_PERM)
MK32(alignbyte_b32, I_ALIGNBYTE)
MK32(add_u32, I_ADD_U32)
MK32(add_co_u32_sgpr, I_ADD_CO_S)
MK32(addc_co_u32_sgpr, I_ADDC_CO_S)

// ---------------------------------------------------------------- rotation forms under test
// rot-1 as x + x with the high half's carry added back into the low half (the last carry-out is
// always zero).  Written with the carry builtins, which hipcc lowers to v_add_co_u32 + two
// v_addc_co_u32: on gfx950 a VALU that reads an SGPR or VCC written by a VALU needs two wait
// states after the write, and only for instructions it emits itself does the compiler schedule
// round that or pad it (inline asm gets one s_nop 0 between statements, nothing inside a string).
__device__ __forceinline__ qrk::u2 rol1_carry(qrk::u2 x) {
  uint32_t t, lo, hi, c1, c2;
  const uint32_t c0 = __builtin_uadd_overflow(x.lo, x.lo, &t);
  hi = __builtin_addc(x.hi, x.hi, c0, &c1);
  lo = __builtin_addc(t, 0u, c1, &c2);
  return {lo, hi};
}

// Byte-multiple rotations as v_perm_b32 of the two halves.  Selector bytes 0-3 pick bytes of the
// second operand, 4-7 of the first: 0x06050403 = ({a, b} >> 24), 0x04030201 = ({a, b} >> 8).
__device__ __forceinline__ uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) {
  return __builtin_amdgcn_perm(a, b, sel);
}

// The rejected forms.  F_CARRY: every rot-1 through rol1_carry.  F_BYTE: offsets 8 and 56 through
// v_perm_b32.  F_FUNNEL and F_THETA5 are the library's two rounds (keccak.cuh): funnel shifts
// throughout, and theta's five rot-1 through qrk::rol1x5.
constexpr int F_FUNNEL = 0, F_CARRY = 1, F_BYTE = 2, F_THETA5 = 4;

template <int N, int F>
__device__ __forceinline__ qrk::u2 rolv(qrk::u2 x) {
  if constexpr (N == 1 && (F & F_CARRY)) {
    return rol1_carry(x);
  } else if constexpr (N == 8 && (F & F_BYTE)) {
    return {perm(x.lo, x.hi, 0x06050403u), perm(x.hi, x.lo, 0x06050403u)};
  } else if constexpr (N == 56 && (F & F_BYTE)) {
    return {perm(x.hi, x.lo, 0x04030201u), perm(x.lo, x.hi, 0x04030201u)};
  } else {
    return qrk::rol<N>(x);
  }
}

// qrk::keccak_fu<2> with every rotation through rolv<N, F>; nothing else differs.  Only the
// rejected forms run through this copy.
template <int F>
__device__ __forceinline__ void keccak_v(qrk::KState& s) {
  using qrk::u2;
  using qrk::xor3;
#pragma unroll 2
  for (int r = 0; r < 24; ++r) {
    u2 C[5], R[5], B[25];
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      C[x].lo = xor3(xor3(s.a[x].lo, s.a[x + 5].lo, s.a[x + 10].lo), s.a[x + 15].lo, s.a[x + 20].lo);
      C[x].hi = xor3(xor3(s.a[x].hi, s.a[x + 5].hi, s.a[x + 10].hi), s.a[x + 15].hi, s.a[x + 20].hi);
    }
#pragma unroll
    for (int x = 0; x < 5; ++x) R[x] = rolv<1, F>(C[x]);
#pragma unroll
    for (int i = 0; i < 25; ++i) {
      const int x = i % 5;
      s.a[i].lo = xor3(s.a[i].lo, C[(x + 4) % 5].lo, R[(x + 1) % 5].lo);
      s.a[i].hi = xor3(s.a[i].hi, C[(x + 4) % 5].hi, R[(x + 1) % 5].hi);
    }
    B[0] = s.a[0];
    B[10] = rolv<1, F>(s.a[1]);
    B[20] = rolv<62, F>(s.a[2]);
    B[5] = rolv<28, F>(s.a[3]);
    B[15] = rolv<27, F>(s.a[4]);
    B[16] = rolv<36, F>(s.a[5]);
    B[1] = rolv<44, F>(s.a[6]);
    B[11] = rolv<6, F>(s.a[7]);
    B[21] = rolv<55, F>(s.a[8]);
    B[6] = rolv<20, F>(s.a[9]);
    B[7] = rolv<3, F>(s.a[10]);
    B[17] = rolv<10, F>(s.a[11]);
    B[2] = rolv<43, F>(s.a[12]);
    B[12] = rolv<25, F>(s.a[13]);
    B[22] = rolv<39, F>(s.a[14]);
    B[23] = rolv<41, F>(s.a[15]);
    B[8] = rolv<45, F>(s.a[16]);
    B[18] = rolv<15, F>(s.a[17]);
    B[3] = rolv<21, F>(s.a[18]);
    B[13] = rolv<8, F>(s.a[19]);
    B[14] = rolv<18, F>(s.a[20]);
    B[24] = rolv<2, F>(s.a[21]);
    B[9] = rolv<61, F>(s.a[22]);
    B[19] = rolv<56, F>(s.a[23]);
    B[4] = rolv<14, F>(s.a[24]);
#pragma unroll
    for (int y = 0; y < 5; ++y)
#pragma unroll
      for (int x = 0; x < 5; ++x) {
        const u2 b0 = B[x + 5 * y], b1 = B[(x + 1) % 5 + 5 * y], b2 = B[(x + 2) % 5 + 5 * y];
        s.a[x + 5 * y].lo = b0.lo ^ (~b1.lo & b2.lo);
        s.a[x + 5 * y].hi = b0.hi ^ (~b1.hi & b2.hi);
      }
    s.a[0].lo ^= qrk::KRC_LO[r];
    s.a[0].hi ^= qrk::KRC_HI[r];
  }
}

template <int F>
__device__ __forceinline__ void keccak_form(qrk::KState& s) {
  if constexpr (F == F_FUNNEL) qrk::keccak_f(s);
  else if constexpr (F == F_THETA5) qrk::keccak_f_carry(s);
  else keccak_v<F>(s);
}

template <int F>
__global__ __launch_bounds__(256) void k_keccak_form(uint64_t* out, int perms) {
  qrk::KState s;
  qrk::kzero(s);
  s.a[0].lo = blockIdx.x * blockDim.x + threadIdx.x;
  for (int p = 0; p < perms; ++p) keccak_form<F>(s);
  uint64_t x = 0;
#pragma unroll
  for (int i = 0; i < 25; ++i) x ^= qrk::kword(s, i);
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

template <int F>
__global__ void k_check_form(const uint64_t* in, uint64_t* o) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  qrk::KState s;
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    const uint64_t w = in[t * 25 + i];
    s.a[i] = {(uint32_t)w, (uint32_t)(w >> 32)};
  }
  keccak_form<F>(s);
#pragma unroll
  for (int i = 0; i < 25; ++i) o[t * 25 + i] = qrk::kword(s, i);
}

// The rot-1 forms alone, each rotation depending on the one before: ten independent 64-bit values
// per lane, in two groups of five.  R1_ALIGNBIT: two v_alignbit_b32.  R1_CARRY_SGPR: qrk::rol1x5,
// the three adds with SGPR-pair carries stage by stage over five values, no padding.
// R1_CARRY_CXX: rol1_carry as the compiler schedules and pads it.
enum { R1_ALIGNBIT, R1_CARRY_SGPR, R1_CARRY_CXX };
constexpr int R1_VALUES = 10;
template <int MODE>
__global__ void k_rol1(uint32_t* out, uint32_t seed) {
  qrk::u2 v[2][5];
#pragma unroll
  for (int j = 0; j < R1_VALUES; ++j)
    v[j / 5][j % 5] = {(seed + threadIdx.x) * (2 * j + 1), seed * (2 * j + 3) + threadIdx.x};
#pragma unroll 2
  for (int i = 0; i < ITERS; ++i) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      qrk::u2 r[5];
      if constexpr (MODE == R1_CARRY_SGPR) {
        qrk::rol1x5(v[g], r);
      } else {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          if constexpr (MODE == R1_CARRY_CXX) {
            r[j] = rol1_carry(v[g][j]);
            asm volatile("" : "+v"(r[j].lo), "+v"(r[j].hi));  // keep every rotation
          } else {
            asm volatile("v_alignbit_b32 %0, %1, %2, 31" : "=v"(r[j].lo) : "v"(v[g][j].lo), "v"(v[g][j].hi));
            asm volatile("v_alignbit_b32 %0, %1, %2, 31" : "=v"(r[j].hi) : "v"(v[g][j].hi), "v"(v[g][j].lo));
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) v[g][j] = r[j];
    }
  }
  uint32_t x = 0;
#pragma unroll
  for (int j = 0; j < R1_VALUES; ++j) x ^= v[j / 5][j % 5].lo ^ v[j / 5][j % 5].hi;
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

// ---------------------------------------------------------------- Keccak with 64-bit shifts
struct S64 {
  uint64_t a[25];
};

__device__ __forceinline__ uint32_t lo32(uint64_t x) { return (uint32_t)x; }
__device__ __forceinline__ uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
__device__ __forceinline__ uint64_t mk(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

template <int N>
__device__ __forceinline__ uint64_t rot(uint64_t x) {
  if constexpr (N == 0) {
    return x;
  } else if constexpr (N == 32) {
    return mk(hi32(x), lo32(x));
  } else if constexpr (N < 32) {
    uint64_t t;  // t.hi = rot.hi exactly; rot.lo = t.lo | hi >> (32 - N)
    asm("v_lshlrev_b64 %0, %2, %1" : "=v"(t) : "v"(x), "i"(N));
    return mk(lo32(t) | (hi32(x) >> (32 - N)), hi32(t));
  } else {
    uint64_t t;  // t.lo = rot.lo exactly; rot.hi = t.hi | lo << (N - 32)
    asm("v_lshrrev_b64 %0, %2, %1" : "=v"(t) : "v"(x), "i"(64 - N));
    return mk(lo32(t), hi32(t) | (lo32(x) << (N - 32)));
  }
}

__device__ __forceinline__ uint64_t x3(uint64_t a, uint64_t b, uint64_t c) {
  return mk(qrk::xor3(lo32(a), lo32(b), lo32(c)), qrk::xor3(hi32(a), hi32(b), hi32(c)));
}

__device__ __forceinline__ uint32_t chi(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;  // a ^ (~b & c)
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xd2" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ void keccak64(S64& s) {
#pragma unroll 1
  for (int r = 0; r < 24; ++r) {
    uint64_t C[5], R[5], B[25];
#pragma unroll
    for (int x = 0; x < 5; ++x) C[x] = x3(x3(s.a[x], s.a[x + 5], s.a[x + 10]), s.a[x + 15], s.a[x + 20]);
#pragma unroll
    for (int x = 0; x < 5; ++x) R[x] = rot<1>(C[x]);
#pragma unroll
    for (int i = 0; i < 25; ++i) s.a[i] = x3(s.a[i], C[(i % 5 + 4) % 5], R[(i % 5 + 1) % 5]);
    B[0] = s.a[0];
    B[10] = rot<1>(s.a[1]);
    B[20] = rot<62>(s.a[2]);
    B[5] = rot<28>(s.a[3]);
    B[15] = rot<27>(s.a[4]);
    B[16] = rot<36>(s.a[5]);
    B[1] = rot<44>(s.a[6]);
    B[11] = rot<6>(s.a[7]);
    B[21] = rot<55>(s.a[8]);
    B[6] = rot<20>(s.a[9]);
    B[7] = rot<3>(s.a[10]);
    B[17] = rot<10>(s.a[11]);
    B[2] = rot<43>(s.a[12]);
    B[12] = rot<25>(s.a[13]);
    B[22] = rot<39>(s.a[14]);
    B[23] = rot<41>(s.a[15]);
    B[8] = rot<45>(s.a[16]);
    B[18] = rot<15>(s.a[17]);
    B[3] = rot<21>(s.a[18]);
    B[13] = rot<8>(s.a[19]);
    B[14] = rot<18>(s.a[20]);
    B[24] = rot<2>(s.a[21]);
    B[9] = rot<61>(s.a[22]);
    B[19] = rot<56>(s.a[23]);
    B[4] = rot<14>(s.a[24]);
#pragma unroll
    for (int y = 0; y < 5; ++y)
#pragma unroll
      for (int x = 0; x < 5; ++x) {
        const uint64_t b0 = B[x + 5 * y], b1 = B[(x + 1) % 5 + 5 * y], b2 = B[(x + 2) % 5 + 5 * y];
        s.a[x + 5 * y] = mk(chi(lo32(b0), lo32(b1), lo32(b2)), chi(hi32(b0), hi32(b1), hi32(b2)));
      }
    s.a[0] ^= mk(qrk::KRC_LO[r], qrk::KRC_HI[r]);
  }
}

__global__ __launch_bounds__(256) void k_keccak_ref(uint64_t* out, int perms) {
  qrk::KState s;
  qrk::kzero(s);
  s.a[0].lo = blockIdx.x * blockDim.x + threadIdx.x;
  for (int p = 0; p < perms; ++p) qrk::keccak_f(s);
  uint64_t x = 0;
#pragma unroll
  for (int i = 0; i < 25; ++i) x ^= qrk::kword(s, i);
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

template <int U>
__global__ __launch_bounds__(256) void k_keccak_u(uint64_t* out, int perms) {
  qrk::KState s;
  qrk::kzero(s);
  s.a[0].lo = blockIdx.x * blockDim.x + threadIdx.x;
  for (int p = 0; p < perms; ++p) qrk::keccak_fu<U>(s);
  uint64_t x = 0;
#pragma unroll
  for (int i = 0; i < 25; ++i) x ^= qrk::kword(s, i);
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

__global__ __launch_bounds__(256) void k_keccak_s64(uint64_t* out, int perms) {
  S64 s;
#pragma unroll
  for (int i = 0; i < 25; ++i) s.a[i] = 0;
  s.a[0] = blockIdx.x * blockDim.x + threadIdx.x;
  for (int p = 0; p < perms; ++p) keccak64(s);
  uint64_t x = 0;
#pragma unroll
  for (int i = 0; i < 25; ++i) x ^= s.a[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

// bit-exactness: random full states through both permutations
__global__ void k_check(const uint64_t* in, uint64_t* o_ref, uint64_t* o_s64) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  qrk::KState s;
  S64 u;
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    const uint64_t w = in[t * 25 + i];
    s.a[i] = {(uint32_t)w, (uint32_t)(w >> 32)};
    u.a[i] = w;
  }
  qrk::keccak_f(s);
  keccak64(u);
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    o_ref[t * 25 + i] = qrk::kword(s, i);
    o_s64[t * 25 + i] = u.a[i];
  }
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  printf("{\"cus\": %d", cus);
  const int blocks = cus * 8, threads = 256;
  uint32_t* d;
  uint64_t* d64;
  CHECK(hipMalloc(&d, (size_t)blocks * threads * 4));
  CHECK(hipMalloc(&d64, (size_t)cus * 16 * 256 * 8));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  // eight instructions per lane and loop iteration; for the rol1 lines, ten rotations
  struct K {
    const char* name;
    void (*fn)(uint32_t*, uint32_t);
    const char* unit = "Ginstr";
    int per_iter = 8;
  } ks[] = {{"lshlrev_b64", k_lshlrev_b64},
            {"lshrrev_b64", k_lshrrev_b64},
            {"lshl_add_u64", k_lshl_add_u64},
            {"mov_b64", k_mov_b64},
            {"pk_mov_b32", k_pk_mov_b32},
            {"xor_b32", k_xor_b32},
            {"alignbit_b32", k_alignbit_b32},
            {"perm_b32", k_perm_b32},
            {"alignbyte_b32", k_alignbyte_b32},
            {"add_u32", k_add_u32},
            {"add_co_u32_sgpr", k_add_co_u32_sgpr},
            {"addc_co_u32_sgpr", k_addc_co_u32_sgpr},
            {"rol1_alignbit_pair", k_rol1<R1_ALIGNBIT>, "Grot", R1_VALUES},
            {"rol1_carry_sgpr", k_rol1<R1_CARRY_SGPR>, "Grot", R1_VALUES},
            {"rol1_carry_cxx", k_rol1<R1_CARRY_CXX>, "Grot", R1_VALUES}};
  for (auto& k : ks) {
    hipLaunchKernelGGL(k.fn, dim3(blocks), dim3(threads), 0, 0, d, 1u);
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int r = 0; r < 5; ++r) {
      CHECK(hipEventRecord(a, 0));
      hipLaunchKernelGGL(k.fn, dim3(blocks), dim3(threads), 0, 0, d, (uint32_t)r);
      CHECK(hipEventRecord(b, 0));
      CHECK(hipEventSynchronize(b));
      float ms;
      CHECK(hipEventElapsedTime(&ms, a, b));
      best = ms < best ? ms : best;
    }
    printf(", \"%s_%s_lane_per_s\": %.1f", k.name, k.unit, (double)blocks * threads * ITERS * k.per_iter / (best * 1e-3) / 1e9);
  }
  // correctness on random states
  const int nchk = 4096;
  uint64_t *in, *o1, *o2;
  CHECK(hipMallocManaged(&in, nchk * 25 * 8));
  CHECK(hipMallocManaged(&o1, nchk * 25 * 8));
  CHECK(hipMallocManaged(&o2, nchk * 25 * 8));
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < nchk * 25; ++i) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    in[i] = x;
  }
  hipLaunchKernelGGL(k_check, dim3(nchk / 256), dim3(256), 0, 0, in, o1, o2);
  CHECK(hipDeviceSynchronize());
  int bad = 0;
  for (int i = 0; i < nchk * 25; ++i) bad += o1[i] != o2[i];
  printf(", \"s64_mismatch_words\": %d", bad);
  const char* vn[] = {"ref", "s64", "u2", "u3", "u4", "u6"};
  for (int v = 0; v < 6; ++v) {
    for (int wpc : {8, 16}) {
      const int kb = cus * wpc, perms = 64;
      void (*fns[])(uint64_t*, int) = {k_keccak_ref, k_keccak_s64, k_keccak_u<2>, k_keccak_u<3>, k_keccak_u<4>, k_keccak_u<6>};
      auto fn = fns[v];
      hipLaunchKernelGGL(fn, dim3(kb), dim3(256), 0, 0, d64, 2);
      CHECK(hipDeviceSynchronize());
      float best = 1e30f;
      for (int r = 0; r < 5; ++r) {
        CHECK(hipEventRecord(a, 0));
        hipLaunchKernelGGL(fn, dim3(kb), dim3(256), 0, 0, d64, perms);
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        best = ms < best ? ms : best;
      }
      const double p = (double)kb * 256 * perms;
      printf(", \"keccak_%s_wg%d_perms_per_s\": %.4e, \"keccak_%s_wg%d_Tops_at_4320\": %.3f", vn[v], wpc,
             p / (best * 1e-3), vn[v], wpc, p * 4320 / (best * 1e-3) / 1e12);
    }
  }
  // Rotation forms: (a) every rotation a funnel shift, (b) carry rot-1, (c) v_perm for offsets 8
  // and 56, (d) both, (e) theta's rot-1 as one five-column carry statement.
  // Bit-exact against (a) first; the first states are the ones a wrong carry or selector byte
  // would show on (one bit at each position, all ones, the half boundaries, distinct bytes).
  constexpr int NF = 5;
  void (*chk[NF])(const uint64_t*, uint64_t*) = {k_check_form<F_FUNNEL>, k_check_form<F_CARRY>, k_check_form<F_BYTE>,
                                                k_check_form<F_CARRY | F_BYTE>, k_check_form<F_THETA5>};
  void (*frm[NF])(uint64_t*, int) = {k_keccak_form<F_FUNNEL>, k_keccak_form<F_CARRY>, k_keccak_form<F_BYTE>,
                                     k_keccak_form<F_CARRY | F_BYTE>, k_keccak_form<F_THETA5>};
  const char* fn4[NF] = {"a", "b", "c", "d", "e"};
  const uint64_t edge[] = {~0ull, 0x8000000080000000ull, 0x0000000100000001ull, 0x8000000000000001ull,
                           0x0000000180000000ull, 0x0123456789abcdefull, 0xff00ff00ff00ff00ull};
  for (int k = 0; k < 64 + 7; ++k)
    for (int i = 0; i < 25; ++i) in[k * 25 + i] = k < 64 ? 1ull << ((k + i) & 63) : edge[k - 64];
  hipLaunchKernelGGL(chk[0], dim3(nchk / 256), dim3(256), 0, 0, in, o1);
  CHECK(hipDeviceSynchronize());
  int bad_any = 0;
  for (int v = 1; v < NF; ++v) {
    hipLaunchKernelGGL(chk[v], dim3(nchk / 256), dim3(256), 0, 0, in, o2);
    CHECK(hipDeviceSynchronize());
    bad = 0;
    for (int i = 0; i < nchk * 25; ++i) bad += o1[i] != o2[i];
    printf(", \"form_%s_mismatch_words\": %d", fn4[v], bad);
    bad_any += bad;
  }
  if (bad_any) {  // a wrong variant is not timed
    printf("}\n");
    return 2;
  }
  // Interleaved a b c d e rounds after a clock warm-up on (a); every round is kept, so that a
  // variant's gain can be held against the spread of (a)'s own rounds.
  constexpr int ROUNDS = 7;
  for (int wpc : {8, 16}) {
    const int kb = cus * wpc, perms = 256;
    for (int w = 0; w < 8; ++w) hipLaunchKernelGGL(frm[0], dim3(kb), dim3(256), 0, 0, d64, perms);
    CHECK(hipDeviceSynchronize());
    double tops[NF][ROUNDS];
    for (int r = 0; r < ROUNDS; ++r)
      for (int v = 0; v < NF; ++v) {
        CHECK(hipEventRecord(a, 0));
        hipLaunchKernelGGL(frm[v], dim3(kb), dim3(256), 0, 0, d64, perms);
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        tops[v][r] = (double)kb * 256 * perms * 4320 / (ms * 1e-3) / 1e12;
      }
    for (int v = 0; v < NF; ++v) {
      printf(", \"keccak_%s_wg%d_Tops_at_4320_rounds\": [", fn4[v], wpc);
      double s[ROUNDS];
      for (int r = 0; r < ROUNDS; ++r) {
        printf("%s%.3f", r ? ", " : "", tops[v][r]);
        s[r] = tops[v][r];
      }
      for (int i = 1; i < ROUNDS; ++i)  // insertion sort for min / median / max
        for (int j = i; j > 0 && s[j] < s[j - 1]; --j) {
          const double t = s[j];
          s[j] = s[j - 1];
          s[j - 1] = t;
        }
      printf("], \"keccak_%s_wg%d_Tops_at_4320\": %.3f, \"keccak_%s_wg%d_Tops_at_4320_min\": %.3f, "
             "\"keccak_%s_wg%d_Tops_at_4320_max\": %.3f",
             fn4[v], wpc, s[ROUNDS / 2], fn4[v], wpc, s[0], fn4[v], wpc, s[ROUNDS - 1]);
    }
  }
  printf("}\n");
  return 0;
}
