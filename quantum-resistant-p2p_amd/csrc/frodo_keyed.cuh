// FrodoKEM key sets: g keys expanded once, and Encaps / Decaps of n rows that name their key by index.
//
// What depends on the key alone is computed when the set is loaded and never again per row: Gen(A) (640: 5,120
// Keccak permutations, or 51,200 AES blocks), B unpacked and pkh = H(pk).  Per key the set holds
//   A      two int8 limb planes, A = 256 hi + lo (the balanced split of k_fr_gen_mm: lo = a & 0xFF,
//          hi = ((a + 128) >> 8) & 0xFF, both read as int8), each column-major [N columns][N rows]: the 16 bytes
//          a lane of the product kernel loads are 16 consecutive rows of one column.  2 N^2 bytes
//   B      u16 [N][8] (16 N bytes)      pkh    32 bytes (SEC used)
//   secret sets also: S^T int16 [8][N] (16 N bytes) and s, 32 bytes (SEC used); pkh is the one stored in sk
// so a public key takes 2 N^2 + 16 N + 32 bytes and a secret one 2 N^2 + 32 N + 64 (every part of the set starts
// 256-aligned, and the planes end with 256 bytes of slack: frodo_keyset_bytes).
//
// A row then costs (seedSE || k) = H(pkh || mu), the sampler stream (123 / 231 / 318 permutations, the launches
// of the per-row call), S'A + E', S'B + E'' and ss.  Nothing per row reads seedA or hashes a public key.
//
//   k_frk_group   1 workgroup       rows of the chunk grouped by key (one key: a compaction of the rows inside the set,
//                                   no sort): histogram, scan over the keys, a tile table of
//                                   at most FRK_TH same-key rows per tile (tiles end at key borders), and a stable
//                                   scatter of the row numbers into a permutation.  key_index is public.  A row whose
//                                   index is outside the set joins no tile
//   k_frk_sa      (tile, 128 cols)  S'A of one tile against its key's A on v_mfma_i32_16x16x64_i8: the tile's S'
//                                   (8 FRK_TH int8 rows) is staged in LDS 128 contraction rows at a time, the A
//                                   limbs come straight from the planes (each fragment is used by one wave, against
//                                   all 8 S' fragments of the tile); two MFMAs per 16 x 16 x 64 step (lo, hi), int32
//                                   accumulation over all N rows (|acc| <= N 128 SMAX < 2^21), lo + (hi << 8) mod
//                                   2^16.  Whole sums: k_frk_pack adds no partials
//   k_frk_front_enc, k_frk_g2_dec, k_frk_dec_m, k_frk_pack
//                                   k_fr_front_enc (without H(pk)), k_fr_g2_dec, k_fr_dec_m and k_fr_pack with pkh,
//                                   S^T, B and s read from the row's key in the set
//   k_frk_finish  lane / row        status; a refused row's ss is zeroed (its ct was by k_frk_pack)
// The sampler stream, the sampler and ss = H(ct || k) are the per-row launchers of frodo_kernels.cuh as they are.
//
// Scratch per row: the per-row call's without the per-wave partial sums ([NWV][8][N] u16 -> [8][N]) and the AES
// round-key records, plus 4 bytes of permutation: 64 N + 8 NP + 420 = 46.5 / 71.1 / 97.7 KB for 640 / 976 / 1344
// against 150 / 323 / 552 KB, and per chunk the tile table and 16 (g + 1) bytes of key tables.
#pragma once
#include "frodo_kernels.cuh"

namespace qrk {
namespace frodo {

constexpr int FRK_TH = 16;    // handshakes per tile: 128 rows of S', 8 MFMA column fragments
constexpr int FRK_KC = 128;   // contraction rows staged per step
constexpr int FRK_SP = FRK_KC + 16;  // LDS pitch (bytes) of a staged S' row
constexpr int FRK_CB = 128;   // columns of A per workgroup: 4 waves x 2 fragments of 16

struct KArgs {
  uint32_t g;
  const int8_t* planes;
  const uint16_t* B;
  const uint64_t* pkh;  // 4 words per key
  const int16_t* St;    // secret sets
  const uint64_t* s;    // secret sets, 4 words per key
  const uint32_t* key_index;
};

struct KeyRef {
  uint32_t key;  // < g: what addresses are formed from
  bool ok;       // the row's index was in range
};
__device__ __forceinline__ KeyRef key_of(const uint32_t* __restrict__ key_index, size_t hs, uint32_t g) {
  const uint32_t k = key_index ? key_index[hs] : 0u;
  const bool ok = k < g;
  return {ok ? k : 0u, ok};
}

// ------------------------------------------------------------ the set
struct SetLayout {
  size_t planes, b_off, pkh_off, st_off, s_off, total;
};
static SetLayout set_layout(size_t N, bool secret, size_t g) {
  SetLayout l;
  l.planes = al256(2 * N * N * g + 256);  // + slack: a fragment of the last column reads up to 48 bytes past it
  l.b_off = l.planes;
  l.pkh_off = l.b_off + al256(16 * N * g);
  l.st_off = l.pkh_off + al256(32 * g);
  l.s_off = l.st_off + (secret ? al256(16 * N * g) : 0);
  l.total = l.s_off + (secret ? al256(32 * g) : 0);
  return l;
}

__device__ __forceinline__ void store_limbs(int8_t* __restrict__ key_planes, int N, int c, int r, uint32_t a) {
  key_planes[(size_t)c * N + r] = (int8_t)(a & 0xFF);
  key_planes[(size_t)N * N + (size_t)c * N + r] = (int8_t)(((a + 128) >> 8) & 0xFF);
}

// Gen(A), SHAKE128: row r of key `key` = SHAKE128(LE16(r) || seedA), one lane per (key, row), stored as limbs
template <int N>
__global__ __launch_bounds__(256) void k_frk_gen_shake(size_t g, const uint8_t* __restrict__ keys, size_t stride,
                                                       size_t seed_off, int8_t* __restrict__ planes) {
  using P = FP<N>;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t key = t / N;
  const int r = (int)(t % N);
  if (key >= g) return;
  const uint64_t* sa = (const uint64_t*)(keys + key * stride + seed_off);
  const uint64_t s0 = sa[0], s1 = sa[1];
  uint64_t in[3] = {(uint64_t)(r & 0xFFFF) | (s0 << 16), (s0 >> 48) | (s1 << 16), s1 >> 48};
  KState s;
  kzero(s);
  absorb_short<21, 3>(s, in, 18);
  int8_t* kp = planes + key * 2 * (size_t)N * N;
#pragma unroll 1
  for (int b = 0; b < P::A_BLOCKS; ++b) {
    if (b) keccak_f(s);
    const int c0 = 84 * b;
    const int nc = (N - c0) < 84 ? (N - c0) : 84;  // a multiple of 4 for every parameter set
#pragma unroll
    for (int w = 0; w < 21; ++w) {
      if (4 * w < nc) {
        const uint32_t lo = s.a[w].lo, hi = s.a[w].hi;
        store_limbs(kp, N, c0 + 4 * w + 0, r, lo & 0xFFFF);
        store_limbs(kp, N, c0 + 4 * w + 1, r, lo >> 16);
        store_limbs(kp, N, c0 + 4 * w + 2, r, hi & 0xFFFF);
        store_limbs(kp, N, c0 + 4 * w + 3, r, hi >> 16);
      }
    }
  }
}

// Gen(A), AES-128: A[i][j .. j + 7] = the 8 little-endian u16 of AES128_seedA(LE16(i) || LE16(j) || 0^96), one lane
// per (key, row), plain T-table rounds (T0 and the S-box in LDS), stored as limbs
template <int N>
__global__ __launch_bounds__(256) void k_frk_gen_aes(size_t g, const uint8_t* __restrict__ keys, size_t stride,
                                                     size_t seed_off, int8_t* __restrict__ planes) {
  using namespace aes;
  __shared__ uint32_t t0[256];
  __shared__ uint8_t sb[256];
  t0[threadIdx.x] = TAB.t0[threadIdx.x];
  sb[threadIdx.x] = TAB.s[threadIdx.x];
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t key = t / N;
  const uint32_t i = (uint32_t)(t % N);
  if (key >= g) return;
  const uint32_t* sa = (const uint32_t*)(keys + key * stride + seed_off);
  const uint32_t kw[4] = {sa[0], sa[1], sa[2], sa[3]};
  uint32_t rk[44];
  expand_key(kw, rk);
  int8_t* kp = planes + key * 2 * (size_t)N * N;
#pragma unroll 1
  for (uint32_t j = 0; j < (uint32_t)N; j += 8) {
    uint32_t s[4] = {(i | (j << 16)) ^ rk[0], rk[1], rk[2], rk[3]}, o[4];
#pragma unroll 1
    for (int rd = 1; rd < 10; ++rd) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        o[c] = t0[B(s[c], 0)] ^ rot8(t0[B(s[(c + 1) & 3], 1)]) ^ rot16(t0[B(s[(c + 2) & 3], 2)]) ^
               rot24(t0[B(s[(c + 3) & 3], 3)]) ^ rk[4 * rd + c];
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = o[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      o[c] = ((uint32_t)sb[B(s[c], 0)] | (uint32_t)sb[B(s[(c + 1) & 3], 1)] << 8 |
              (uint32_t)sb[B(s[(c + 2) & 3], 2)] << 16 | (uint32_t)sb[B(s[(c + 3) & 3], 3)] << 24) ^
             rk[40 + c];
      store_limbs(kp, N, (int)j + 2 * c, (int)i, o[c] & 0xFFFF);
      store_limbs(kp, N, (int)j + 2 * c + 1, (int)i, o[c] >> 16);
    }
  }
}

// Tests only (tests/frodo_keyed_probe.hip): the limb planes of a caller's A, u16 [g][N][N] row-major
template <int N>
__global__ __launch_bounds__(256) void k_frk_split(size_t g, const uint16_t* __restrict__ A,
                                                   int8_t* __restrict__ planes) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;  // (key, c, r), r fastest: the stores coalesce
  const size_t key = t / ((size_t)N * N);
  const int c = (int)((t / N) % N), r = (int)(t % N);
  if (key >= g) return;
  store_limbs(planes + key * 2 * (size_t)N * N, N, c, r, A[(key * N + r) * N + c]);
}

// B unpacked; a secret set's S^T, s and pkh copied from sk.  One workgroup per key; row = pk (pk_off 0) or sk
template <int N>
__global__ __launch_bounds__(256) void k_frk_unpack(size_t g, const uint8_t* __restrict__ keys, size_t stride,
                                                    bool secret, uint16_t* __restrict__ B, int16_t* __restrict__ St,
                                                    uint64_t* __restrict__ s, uint64_t* __restrict__ pkh) {
  using P = FP<N>;
  const size_t key = blockIdx.x;
  if (key >= g) return;
  const int t = threadIdx.x;
  const uint8_t* row = keys + key * stride;
  const uint8_t* pkb = row + (secret ? P::SEC : 0) + 16;
  for (int gi = t; gi < N; gi += 256) {
    uint32_t v[8];
    unpack8<P::LOGQ>(pkb + gi * P::LOGQ, v);
    *(uint4*)(B + (key * N + gi) * 8) =
        make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
  }
  if (!secret) return;
  const uint64_t* sts = (const uint64_t*)(row + P::SEC + P::PK);  // S^T int16 LE [8][N]
  uint64_t* sto = (uint64_t*)(St + key * 8 * N);
  for (int w = t; w < 2 * N; w += 256) sto[w] = sts[w];
  if (t < P::SEC / 8) {
    s[key * 4 + t] = ((const uint64_t*)row)[t];
    pkh[key * 4 + t] = ((const uint64_t*)(row + P::SEC + P::PK + 2 * N * NBAR))[t];
  }
}

// pkh = H(pk) of a public set's keys, one wave per key
template <int N>
__global__ __launch_bounds__(64) void k_frk_pkh(size_t g, const uint8_t* __restrict__ pk, uint64_t* __restrict__ pkh) {
  using P = FP<N>;
  const size_t key = blockIdx.x;
  if (key >= g) return;
  const Coop c = coop_init();
  const CState h = pkh_coop<N>(pk + key * P::PK, c);
  if (coop_canon(c) && c.idx < P::SEC / 8) pkh[key * 4 + c.idx] = cs_word(h);
}

// ------------------------------------------------------------ grouping
// One workgroup.  cnt / start / tstart / cursor: g + 1 words each.  Out: perm (the rows with an index inside the set,
// ordered by key and, within a key, by row number), tiles {key, first slot of perm, rows, 0}, hdr[0] = tiles.
__device__ __forceinline__ uint32_t ld_l2(uint32_t* p) { return atomicAdd(p, 0u); }

static __global__ __launch_bounds__(1024) void k_frk_group(size_t n, uint32_t g, const uint32_t* __restrict__ key_index,
                                                    uint32_t* cnt, uint32_t* start, uint32_t* tstart, uint32_t* cursor,
                                                    uint32_t* perm, uint4* tiles, uint32_t* hdr) {
  __shared__ uint32_t sa[1024], sb[1024];
  __shared__ uint32_t base[2];
  const int t = threadIdx.x;
  for (uint32_t k = t; k <= g; k += 1024) cnt[k] = 0;
  if (t == 0) base[0] = base[1] = 0;
  __syncthreads();
  if (g == 1) {
    // One key (key_index NULL included): nothing to sort.  A stable compaction of the rows inside the set, 1024 at
    // a time -- a row's slot is the rows kept so far plus the kept rows before it in its wave and in the waves
    // below -- and tiles of consecutive slots.
    const int lane = t & 63, wv = t >> 6;
    for (size_t i0 = 0; i0 < n; i0 += 1024) {
      const size_t i = i0 + t;
      const bool ok = i < n && (key_index ? key_index[i] == 0u : true);
      const unsigned long long m = __ballot(ok);
      if (lane == 0) sa[wv] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t slot = base[0] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wv; ++w) slot += sa[w];
      if (ok) perm[slot] = (uint32_t)i;
      __syncthreads();
      if (t == 0) {
        uint32_t kept = 0;
        for (int w = 0; w < 16; ++w) kept += sa[w];
        base[0] += kept;
      }
      __syncthreads();
    }
    const uint32_t kept = base[0], ntiles = (kept + FRK_TH - 1) / FRK_TH;
    for (uint32_t b = t; b < ntiles; b += 1024) {
      const uint32_t left = kept - b * FRK_TH;
      tiles[b] = make_uint4(0u, b * FRK_TH, left < (uint32_t)FRK_TH ? left : (uint32_t)FRK_TH, 0u);
    }
    if (t == 0) hdr[0] = ntiles;
    return;
  }
  for (size_t i = t; i < n; i += 1024) {
    const uint32_t k = key_index ? key_index[i] : 0u;
    if (k < g) atomicAdd(&cnt[k], 1u);
  }
  __syncthreads();
  // exclusive scans over the keys of the rows and of the tiles, 1024 keys at a time
  for (uint32_t k0 = 0; k0 < g; k0 += 1024) {
    const uint32_t k = k0 + t;
    const uint32_t c = k < g ? ld_l2(&cnt[k]) : 0u;
    const uint32_t tl = (c + FRK_TH - 1) / FRK_TH;
    sa[t] = c, sb[t] = tl;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const uint32_t xa = t >= d ? sa[t - d] : 0u, xb = t >= d ? sb[t - d] : 0u;
      __syncthreads();
      sa[t] += xa, sb[t] += xb;
      __syncthreads();
    }
    if (k < g) {
      start[k] = base[0] + sa[t] - c;
      cursor[k] = base[0] + sa[t] - c;
      tstart[k] = base[1] + sb[t] - tl;
    }
    __syncthreads();
    if (t == 1023) base[0] += sa[t], base[1] += sb[t];
    __syncthreads();
  }
  const uint32_t ntiles = base[1];
  if (t == 0) start[g] = base[0], tstart[g] = ntiles, hdr[0] = ntiles;
  __syncthreads();
  // the tile table: tile b belongs to the key k with tstart[k] <= b < tstart[k + 1]
  for (uint32_t b = t; b < ntiles; b += 1024) {
    uint32_t lo = 0, hi = g;  // the first k in (lo, hi] with tstart[k] > b, minus one
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (tstart[mid] <= b) lo = mid; else hi = mid;
    }
    const uint32_t k = lo, tt = b - tstart[k], c = start[k + 1] - start[k];
    const uint32_t rows = c - tt * FRK_TH < (uint32_t)FRK_TH ? c - tt * FRK_TH : (uint32_t)FRK_TH;
    tiles[b] = make_uint4(k, start[k] + tt * FRK_TH, rows, 0u);
  }
  // stable scatter, 1024 rows at a time: a row's slot is its key's cursor plus the same-key rows before it here
  for (size_t i0 = 0; i0 < n; i0 += 1024) {
    const size_t i = i0 + t;
    const uint32_t kraw = i < n ? (key_index ? key_index[i] : 0u) : 0xFFFFFFFFu;
    const uint32_t k = kraw < g ? kraw : 0xFFFFFFFFu;
    sa[t] = k;
    __syncthreads();
    if (k != 0xFFFFFFFFu) {
      const int m = (int)(n - i0 < 1024 ? n - i0 : 1024);
      uint32_t before = 0, all = 0;
      for (int j = 0; j < m; ++j) {
        const uint32_t e = sa[j] == k;
        all += e;
        before += (j < t) ? e : 0u;
      }
      const uint32_t cur = cursor[k];
      perm[cur + before] = (uint32_t)i;
      sb[t] = before == 0 ? cur + all : 0u;
    }
    __syncthreads();
    if (k != 0xFFFFFFFFu && sb[t]) cursor[k] = sb[t];
    __syncthreads();
  }
}

// ------------------------------------------------------------ rows
// Encaps front: (seedSE || k) = H(pkh || mu), pkh from the row's key
template <int N>
__global__ __launch_bounds__(256) void k_frk_front_enc(KArgs a, const uint8_t* __restrict__ mu, size_t n,
                                                       uint64_t* __restrict__ seeds) {
  using P = FP<N>;
  const size_t hs = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (hs >= n) return;
  const KeyRef kr = key_of(a.key_index, hs, a.g);
  const uint64_t* pkh = a.pkh + (size_t)kr.key * 4;
  uint64_t in[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // pkh || mu: SEC + MU <= 64 bytes
#pragma unroll
  for (int w = 0; w < P::SEC / 8; ++w) in[w] = pkh[w];
  const uint64_t* muw = (const uint64_t*)(mu + hs * P::MU);
#pragma unroll
  for (int w = 0; w < P::MU / 8; ++w) in[P::SEC / 8 + w] = muw[w];
  uint64_t* sd = seeds + hs * 16;
#pragma unroll
  for (int w = 0; w < P::SEC / 8; ++w) sd[8 + w] = in[w];  // pkh
  KState s;
  kzero(s);
  absorb_short<P::RW, 8>(s, in, P::SEC + P::MU);
#pragma unroll
  for (int w = 0; w < 2 * P::SEC / 8; ++w) sd[w] = kword(s, w);  // seedSE || k
}

// Decaps: (seedSE' || k') = H(pkh || mu'), pkh from the row's key, mu' from seeds[12..]
template <int N>
__global__ __launch_bounds__(256) void k_frk_g2_dec(KArgs a, size_t n, uint64_t* __restrict__ seeds) {
  using P = FP<N>;
  const size_t hs = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (hs >= n) return;
  const KeyRef kr = key_of(a.key_index, hs, a.g);
  const uint64_t* pkh = a.pkh + (size_t)kr.key * 4;
  uint64_t* sd = seeds + hs * 16;
  uint64_t in[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int w = 0; w < P::SEC / 8; ++w) in[w] = pkh[w];
#pragma unroll
  for (int w = 0; w < P::MU / 8; ++w) in[P::SEC / 8 + w] = sd[12 + w];
  KState s;
  kzero(s);
  absorb_short<P::RW, 8>(s, in, P::SEC + P::MU);
#pragma unroll
  for (int w = 0; w < 2 * P::SEC / 8; ++w) sd[w] = kword(s, w);
}

// Decaps: M = C - B'S, mu' = Decode(M) -> seeds[12..]: k_fr_dec_m with S^T from the row's key (a refused row
// computes on key 0; nothing of it is kept)
template <int N>
__global__ __launch_bounds__(256) void k_frk_dec_m(size_t n, KArgs a, const uint8_t* __restrict__ ct,
                                                   uint64_t* __restrict__ seeds) {
  using P = FP<N>;
  constexpr int PIT = N + 8;
  __shared__ __attribute__((aligned(16))) uint16_t bq[NBAR * PIT];
  __shared__ __attribute__((aligned(16))) uint16_t sq[NBAR * PIT];
  __shared__ uint32_t red[256];
  const size_t hs = blockIdx.x;
  if (hs >= n) return;
  const int t = threadIdx.x;
  const KeyRef kr = key_of(a.key_index, hs, a.g);
  const uint8_t* c = ct + hs * P::CT;
  for (int g = t; g < N; g += 256) {  // B' group g = flat values 8g .. 8g+7 = row i, columns j .. j+7
    uint32_t v[8];
    unpack8<P::LOGQ>(c + g * P::LOGQ, v);
    const int i = (8 * g) / N, j = (8 * g) % N;
    *(uint4*)&bq[i * PIT + j] =
        make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
  }
  const uint64_t* sts = (const uint64_t*)(a.St + (size_t)kr.key * 8 * N);  // S^T int16 [8][N]
  for (int g = t; g < N; g += 256) {
    const int k = (8 * g) / N, j = (8 * g) % N;
    *(uint2*)&sq[k * PIT + j] = *(const uint2*)&sts[2 * g];
    *(uint2*)&sq[k * PIT + j + 4] = *(const uint2*)&sts[2 * g + 1];
  }
  __syncthreads();
  {
    const int p = t & 63, i = p >> 3, k = p & 7, qj = t >> 6;
    constexpr int JQ = N / 4;
    const uint32_t* b2 = (const uint32_t*)&bq[i * PIT + qj * JQ];
    const uint32_t* s2 = (const uint32_t*)&sq[k * PIT + qj * JQ];
    uint32_t acc = 0;
#pragma unroll 4
    for (int j = 0; j < JQ / 2; ++j) {
      const uint32_t bb = b2[j], ss = s2[j];
      acc += (bb & 0xFFFF) * (uint32_t)(int32_t)(int16_t)(ss & 0xFFFF);
      acc += (bb >> 16) * (uint32_t)(int32_t)(int16_t)(ss >> 16);
    }
    red[t] = acc;
  }
  __syncthreads();
  if (t >= 64) return;
  const uint32_t acc = red[t] + red[t + 64] + red[t + 128] + red[t + 192];
  const uint32_t cval = unpack_at<P::LOGQ>(c + P::LOGQ * N, (size_t)t);
  const uint32_t mval = (cval - acc) & P::QMASK;
  const uint32_t dv = ((mval + (1u << (P::LOGQ - P::EB - 1))) >> (P::LOGQ - P::EB)) & ((1u << P::EB) - 1);
  uint64_t* mu = seeds + hs * 16 + 12;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint64_t part = 0;
    const int b = P::EB * t - 64 * w;
    if (b >= 0 && b < 64) part = (uint64_t)dv << b;
    else if (b < 0 && b + P::EB > 0) part = (uint64_t)dv >> (-b);
    const uint32_t lo = wave_or((uint32_t)part), hi = wave_or((uint32_t)(part >> 32));
    if (t == 0 && w < (P::MU + 7) / 8) mu[w] = ((uint64_t)hi << 32) | lo;
  }
}

// S'A of one tile (at most FRK_TH rows of one key) and FRK_CB columns of that key's A.
//   D(16x16) = X(16x64) . Y(64x16),  m = column c of A, n = (handshake of a pair, k), K = row r of A,
//   X[c][r] = limb(A[r][c]) from the planes, Y[r][(h, k)] = S'[h][k][r] from LDS.
// Lane l supplies m / n = l & 15 and the K slice 16 (l >> 4) .. + 15 of both operands (the same pairing of
// contraction indices in X and Y, so the result does not depend on the hardware's order inside a fragment);
// D: col = l & 15 (h, k), row = 4 (l >> 4) + reg (c).  Rows of A past N (976: the last step's rows 976 .. 1023) are
// whatever follows in the planes, paired with the zero pad of S'.
template <int N>
__global__ __launch_bounds__(256) void k_frk_sa(const uint4* __restrict__ tiles, const uint32_t* __restrict__ hdr,
                                                const uint32_t* __restrict__ perm, const int8_t* __restrict__ planes,
                                                const int8_t* __restrict__ sp8, uint16_t* __restrict__ part) {
  using P = FP<N>;
  static_assert(P::NP % FRK_KC == 0 && N % 16 == 0, "staging steps, column fragments");
  __shared__ __attribute__((aligned(16))) int8_t ys[FRK_TH * NBAR * FRK_SP];
  if (blockIdx.x >= hdr[0]) return;
  const uint4 tl = tiles[blockIdx.x];  // key, first slot of perm, rows
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int kq = lane & 15, ks = 16 * (lane >> 4);
  const int c0 = (int)blockIdx.y * FRK_CB + wv * 32;  // the wave's two column fragments: c0, c0 + 16
  const int8_t* lo = planes + (size_t)tl.x * 2 * N * N;
  const int8_t* hi = lo + (size_t)N * N;
  // staging: thread t copies 64 bytes of S' row t >> 1 (= 8 slot + k) per step
  const int srow = t >> 1, sh = (t & 1) * 64;
  const bool son = (uint32_t)(srow >> 3) < tl.z;
  const size_t shs = son ? perm[tl.y + (srow >> 3)] : 0;
  const int8_t* ysrc = sp8 + (shs * NBAR + (srow & 7)) * P::NP + sh;
  v4i acc[2][FRK_TH / 2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nt = 0; nt < FRK_TH / 2; ++nt) acc[m][nt][0] = acc[m][nt][1] = (v4i){0, 0, 0, 0};
#pragma unroll 1
  for (int kc = 0; kc < P::NP; kc += FRK_KC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v4i v = {0, 0, 0, 0};
      if (son) v = *(const v4i*)(ysrc + kc + 16 * q);
      *(v4i*)(ys + srow * FRK_SP + sh + 16 * q) = v;
    }
    __syncthreads();
    if (c0 >= N) continue;  // whole wave; it still takes part in the barriers
#pragma unroll
    for (int kk = 0; kk < FRK_KC; kk += 64) {
      if (kc + kk >= N) break;  // 1344: the last 64 rows of the pitch are pad alone
      const int r = kc + kk + ks;
      v4i xl[2], xh[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int col = c0 + 16 * m < N ? c0 + 16 * m + kq : kq;  // a fragment past N repeats one inside
        xl[m] = *(const v4i*)(lo + (size_t)col * N + r);
        xh[m] = *(const v4i*)(hi + (size_t)col * N + r);
      }
#pragma unroll
      for (int nt = 0; nt < FRK_TH / 2; ++nt) {
        const v4i y = *(const v4i*)(ys + (nt * 16 + kq) * FRK_SP + kk + ks);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          acc[m][nt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xl[m], y, acc[m][nt][0], 0, 0, 0);
          acc[m][nt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xh[m], y, acc[m][nt][1], 0, 0, 0);
        }
      }
    }
  }
  if (c0 >= N) return;
#pragma unroll
  for (int nt = 0; nt < FRK_TH / 2; ++nt) {
    const uint32_t slot = 2 * nt + (kq >> 3);
    if (slot >= tl.z) continue;
    const size_t hs = perm[tl.y + slot];
    uint16_t* prt = part + (hs * NBAR + (kq & 7)) * N;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int cl = c0 + 16 * m;
      if (cl >= N) continue;
      uint32_t v[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) v[g] = ((uint32_t)acc[m][nt][0][g] + ((uint32_t)acc[m][nt][1][g] << 8)) & 0xFFFFu;
      *(uint2*)(prt + cl + 4 * (lane >> 4)) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    }
  }
}

// k_fr_pack with one whole sum instead of partials, and B (unpacked in the set) and s from the row's key.
// A refused row: a zero ct row (Encaps) and a zero kk, nothing else.
template <int N, int MODE>
__global__ __launch_bounds__(256) void k_frk_pack(size_t n, KArgs a, const int8_t* __restrict__ sp8,
                                                  const int16_t* __restrict__ ep16, const int16_t* __restrict__ epp16,
                                                  const uint16_t* __restrict__ part, const uint64_t* __restrict__ seeds,
                                                  const uint8_t* __restrict__ mu_base, size_t mu_stride,
                                                  uint8_t* __restrict__ ct_out, const uint8_t* __restrict__ ct_in,
                                                  uint64_t* __restrict__ kk) {
  using P = FP<N>;
  constexpr int CTW = P::CT / 8;
  __shared__ __attribute__((aligned(16))) uint16_t bsh[N * NBAR];  // B [j][i]
  __shared__ __attribute__((aligned(16))) uint8_t cbuf[(P::CT + 15) / 16 * 16];
  __shared__ uint32_t red[256];
  __shared__ uint32_t cv[64];
  const size_t hs = blockIdx.x;
  if (hs >= n) return;
  const int t = threadIdx.x;
  const KeyRef kr = key_of(a.key_index, hs, a.g);
  if (!kr.ok) {  // the whole workgroup: the index is public
    if (MODE == 0) {
      uint64_t* o = (uint64_t*)(ct_out + hs * P::CT);
      for (int x = t; x < CTW; x += 256) o[x] = 0;
    }
    if (t < 4) kk[hs * 4 + t] = 0;
    return;
  }
  // 1. B of the key
  const uint4* bsrc = (const uint4*)(a.B + (size_t)kr.key * N * NBAR);
  for (int g = t; g < N; g += 256) *(uint4*)&bsh[g * 8] = bsrc[g];
  // 2. B' groups: S'A + E', masked, packed into LDS
  const uint16_t* pp = part + hs * NBAR * N;
  const int16_t* ep = ep16 + hs * NBAR * N;
  for (int g = t; g < N; g += 256) {
    const uint4 e0 = *(const uint4*)(ep + 8 * g), x0 = *(const uint4*)(pp + 8 * g);
    const uint32_t e[4] = {e0.x, e0.y, e0.z, e0.w}, x[4] = {x0.x, x0.y, x0.z, x0.w};
    uint32_t v[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[2 * q] = (e[q] & 0xFFFF) + (x[q] & 0xFFFF), v[2 * q + 1] = (e[q] >> 16) + (x[q] >> 16);
    pack8<P::LOGQ>(v, cbuf + g * P::LOGQ);
  }
  __syncthreads();
  // 3. V[k][i] = sum_j S'[k][j] B[j][i]: thread (k, i) x quarter of j
  {
    const int p = t & 63, k = p >> 3, i = p & 7, qj = t >> 6;
    constexpr int JQ = N / 4;  // a multiple of 4
    const int8_t* sp = sp8 + (hs * NBAR + k) * P::NP + qj * JQ;
    const uint16_t* bc = bsh + qj * JQ * NBAR + i;
    uint32_t acc = 0;
#pragma unroll 4
    for (int j = 0; j < JQ; j += 4) {
      const uint32_t s4 = *(const uint32_t*)(sp + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (uint32_t)((int32_t)(int8_t)(s4 >> (8 * e)) * (int32_t)bc[(j + e) * NBAR]);
    }
    red[t] = acc;
  }
  __syncthreads();
  if (t < 64) {
    // Encode(mu): value t takes EB bits of mu at bit EB*t (little-endian bit order)
    const uint8_t* mu = mu_base + hs * mu_stride;
    const int bit0 = P::EB * t;
    uint32_t mv = 0;
#pragma unroll
    for (int b = 0; b < P::EB; ++b) mv |= (uint32_t)((mu[(bit0 + b) >> 3] >> ((bit0 + b) & 7)) & 1) << b;
    const uint32_t v = red[t] + red[t + 64] + red[t + 128] + red[t + 192] + (uint32_t)(int32_t)epp16[hs * 64 + t];
    cv[t] = (v + (mv << (P::LOGQ - P::EB))) & P::QMASK;
  }
  __syncthreads();
  if (t < 8) {
    uint32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = cv[8 * t + e];
    pack8<P::LOGQ>(v, cbuf + P::LOGQ * N + t * P::LOGQ);
  }
  __syncthreads();
  const uint64_t* cb = (const uint64_t*)cbuf;
  const uint64_t* sd = seeds + hs * 16;
  if (MODE == 0) {
    uint64_t* o = (uint64_t*)(ct_out + hs * P::CT);
    for (int x = t; x < CTW; x += 256) o[x] = cb[x];
    if (t < P::SEC / 8) kk[hs * 4 + t] = sd[P::SEC / 8 + t];
    return;
  }
  // 4. decaps: constant-time compare of ct' (LDS) with ct, select k' or s
  const uint64_t* c1 = (const uint64_t*)(ct_in + hs * P::CT);
  uint64_t d = 0;
  for (int x = t; x < CTW; x += 256) d |= cb[x] ^ c1[x];
  uint32_t diff = wave_or((uint32_t)d | (uint32_t)(d >> 32));
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = diff;
  __syncthreads();
  diff = red[0] | red[1] | red[2] | red[3];
  const uint64_t mask = (uint64_t)0 - (uint64_t)(diff == 0);
  if (t < P::SEC / 8) {
    const uint64_t kp = sd[P::SEC / 8 + t];
    const uint64_t sv = a.s[(size_t)kr.key * 4 + t];
    kk[hs * 4 + t] = (kp & mask) | (sv & ~mask);
  }
}

// status, and a refused row's ss zeroed (k_fr_ss hashed its zero ct and kk)
template <int N>
__global__ __launch_bounds__(256) void k_frk_finish(KArgs a, size_t n, uint8_t* __restrict__ ss,
                                                    int32_t* __restrict__ status) {
  using P = FP<N>;
  const size_t hs = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (hs >= n) return;
  const KeyRef kr = key_of(a.key_index, hs, a.g);
  if (status) status[hs] = kr.ok ? 0 : -1;
  if (!kr.ok) {
    uint64_t* o = (uint64_t*)(ss + hs * P::SEC);
#pragma unroll
    for (int w = 0; w < P::SEC / 8; ++w) o[w] = 0;
  }
}

// ------------------------------------------------------------ host
// The per-row View's regions (its launchers take it) with whole sums in `part` and no AES records, then the
// grouping: the permutation, the tile table, four tables of g + 1 words and the tile count.
template <int N>
struct KView : View<N> {
  uint32_t *perm, *cnt, *start, *tstart, *cursor, *hdr;
  uint4* tiles;
};
static size_t max_tiles(size_t C, size_t g) { return C / FRK_TH + std::min(C, g) + 1; }

template <int N>
static size_t keyed_scratch_t(size_t C, size_t g) {
  using P = FP<N>;
  return al256(C * P::SE_WORDS * 8) + al256(C * 8 * P::NP + 256) + al256(C * 8 * N * 2) + al256(C * 64 * 2) +
         al256(C * 8 * N * 2) + al256(C * 128) + al256(C * 32) + al256(C * 4) + al256(max_tiles(C, g) * 16) +
         4 * al256((g + 1) * 4) + 256;
}

template <int N>
static KView<N> keyed_carve(void* base, size_t C, size_t g) {
  using P = FP<N>;
  uint8_t* p = (uint8_t*)base;
  KView<N> v;
  auto take = [&](size_t bytes) {
    uint8_t* q = p;
    p += al256(bytes);
    return q;
  };
  v.raw = (uint64_t*)take(C * P::SE_WORDS * 8);
  v.sp8 = (int8_t*)take(C * 8 * P::NP + 256);
  v.ep16 = (int16_t*)take(C * 8 * N * 2);
  v.epp16 = (int16_t*)take(C * 64 * 2);
  v.part = (uint16_t*)take(C * 8 * N * 2);
  v.seeds = (uint64_t*)take(C * 128);
  v.kk = (uint64_t*)take(C * 32);
  v.aesp = nullptr;
  v.perm = (uint32_t*)take(C * 4);
  v.tiles = (uint4*)take(max_tiles(C, g) * 16);
  v.cnt = (uint32_t*)take((g + 1) * 4);
  v.start = (uint32_t*)take((g + 1) * 4);
  v.tstart = (uint32_t*)take((g + 1) * 4);
  v.cursor = (uint32_t*)take((g + 1) * 4);
  v.hdr = (uint32_t*)take(4);
  return v;
}

// the view of a set's allocation (frodo_keyset_view)
static FrodoKeys view_of(size_t N, bool secret, size_t g, const void* mem) {
  const SetLayout l = set_layout(N, secret, g);
  const uint8_t* base = (const uint8_t*)mem;
  FrodoKeys v;
  v.g = (uint32_t)g;
  v.planes = (const int8_t*)base;
  v.B = (const uint16_t*)(base + l.b_off);
  v.pkh = (const uint64_t*)(base + l.pkh_off);
  if (secret) {
    v.St = (const int16_t*)(base + l.st_off);
    v.s = (const uint64_t*)(base + l.s_off);
  }
  return v;
}

static KArgs args_of(const FrodoKeys& ks, const uint32_t* key_index) {
  return {ks.g, ks.planes, ks.B, ks.pkh, ks.St, ks.s, key_index};
}

template <int N>
static void launch_group(const KView<N>& v, const KArgs& a, size_t n, hipStream_t st) {
  QRK_LAUNCH("k_frk_group", st, k_frk_group, dim3(1), dim3(1024), 0, st, n, a.g, a.key_index, v.cnt, v.start,
             v.tstart, v.cursor, v.perm, v.tiles, v.hdr);
}

// S'A of every row with a key, whole sums -> v.part
template <int N>
static void launch_sa_keyed(const KView<N>& v, const KArgs& a, size_t n, hipStream_t st) {
  const unsigned tiles = (unsigned)(n / FRK_TH + std::min<size_t>(n, a.g));  // no fewer than k_frk_group can make
  QRK_LAUNCH("k_frk_sa", st, k_frk_sa<N>, dim3(tiles, (N + FRK_CB - 1) / FRK_CB), dim3(256), 0, st, v.tiles, v.hdr,
             v.perm, a.planes, v.sp8, v.part);
}

template <int N>
static hipError_t encaps_keyed_t(const FrodoKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ct, uint8_t* ss,
                                 const uint8_t* mu, int32_t* status, void* scratch, hipStream_t st) {
  using P = FP<N>;
  const KView<N> v = keyed_carve<N>(scratch, round64(n), ks.g);
  const KArgs a = args_of(ks, key_index);
  launch_group<N>(v, a, n, st);
  QRK_LAUNCH("k_frk_front_enc", st, k_frk_front_enc<N>, dim3(blocks_for(n)), dim3(256), 0, st, a, mu, n, v.seeds);
  launch_se<N>(v, n, 0x96, P::SE_WORDS, st);
  launch_sample<N, false>(v, n, st);
  launch_sa_keyed<N>(v, a, n, st);
  QRK_LAUNCH("k_frk_pack", st, (k_frk_pack<N, 0>), dim3((unsigned)n), dim3(256), 0, st, n, a, v.sp8, v.ep16, v.epp16,
             v.part, v.seeds, mu, (size_t)P::MU, ct, nullptr, v.kk);
  launch_ss<N>(ct, n, v, ss, st);
  QRK_LAUNCH("k_frk_finish", st, k_frk_finish<N>, dim3(blocks_for(n)), dim3(256), 0, st, a, n, ss, status);
  return launch_status();
}

template <int N>
static hipError_t decaps_keyed_t(const FrodoKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ss,
                                 const uint8_t* ct, int32_t* status, void* scratch, hipStream_t st) {
  using P = FP<N>;
  const KView<N> v = keyed_carve<N>(scratch, round64(n), ks.g);
  const KArgs a = args_of(ks, key_index);
  launch_group<N>(v, a, n, st);
  QRK_LAUNCH("k_frk_dec_m", st, k_frk_dec_m<N>, dim3((unsigned)n), dim3(256), 0, st, n, a, ct, v.seeds);
  QRK_LAUNCH("k_frk_g2_dec", st, k_frk_g2_dec<N>, dim3(blocks_for(n)), dim3(256), 0, st, a, n, v.seeds);
  launch_se<N>(v, n, 0x96, P::SE_WORDS, st);
  launch_sample<N, false>(v, n, st);
  launch_sa_keyed<N>(v, a, n, st);
  QRK_LAUNCH("k_frk_pack", st, (k_frk_pack<N, 1>), dim3((unsigned)n), dim3(256), 0, st, n, a, v.sp8, v.ep16, v.epp16,
             v.part, v.seeds, (const uint8_t*)(v.seeds + 12), (size_t)128, nullptr, ct, v.kk);
  launch_ss<N>(ct, n, v, ss, st);
  QRK_LAUNCH("k_frk_finish", st, k_frk_finish<N>, dim3(blocks_for(n)), dim3(256), 0, st, a, n, ss, status);
  return launch_status();
}

// Tests only (tests/frodo_keyed_probe.hip): the keyed launches after the sampler on chosen sample matrices (the
// regions k_fr_sample fills); writes ct
template <int N>
static hipError_t dbg_keyed_from_samples_t(const FrodoKeys& ks, size_t n, const uint32_t* key_index, const int8_t* s8,
                                           const int16_t* e16, const int16_t* epp16, const uint8_t* mu, uint8_t* ct,
                                           void* scratch, hipStream_t st) {
  using P = FP<N>;
  const KView<N> v = keyed_carve<N>(scratch, round64(n), ks.g);
  const KArgs a = args_of(ks, key_index);
  qrk_chk(hipMemcpyAsync(v.sp8, s8, n * NBAR * P::NP, hipMemcpyDeviceToDevice, st));
  qrk_chk(hipMemcpyAsync(v.ep16, e16, n * NBAR * N * 2, hipMemcpyDeviceToDevice, st));
  qrk_chk(hipMemcpyAsync(v.epp16, epp16, n * 64 * 2, hipMemcpyDeviceToDevice, st));
  launch_group<N>(v, a, n, st);
  launch_sa_keyed<N>(v, a, n, st);
  QRK_LAUNCH("k_frk_pack", st, (k_frk_pack<N, 0>), dim3((unsigned)n), dim3(256), 0, st, n, a, v.sp8, v.ep16, v.epp16,
             v.part, v.seeds, mu, (size_t)P::MU, ct, nullptr, v.kk);
  return launch_status();
}

// matrix: tests only (tests/frodo_keyed_probe.hip), A from this u16 [g][N][N] instead of generated; else NULL
template <int N>
static hipError_t expand_t(bool aes, bool secret, size_t g, const uint8_t* keys, const uint16_t* matrix, void* mem,
                           hipStream_t st) {
  using P = FP<N>;
  const SetLayout l = set_layout(N, secret, g);
  uint8_t* base = (uint8_t*)mem;
  qrk_chk(hipMemsetAsync(mem, 0, l.total, st));  // the padding between the parts too
  if (launch_status() != hipSuccess) return launch_status();
  const size_t stride = secret ? P::SK : P::PK, seed_off = secret ? P::SEC : 0;
  int8_t* planes = (int8_t*)base;
  if (matrix)
    QRK_LAUNCH("k_frk_split", st, k_frk_split<N>, dim3(blocks_for(g * N * N)), dim3(256), 0, st, g, matrix, planes);
  else if (aes)
    QRK_LAUNCH("k_frk_gen_aes", st, k_frk_gen_aes<N>, dim3(blocks_for(g * N)), dim3(256), 0, st, g, keys, stride,
               seed_off, planes);
  else
    QRK_LAUNCH("k_frk_gen_shake", st, k_frk_gen_shake<N>, dim3(blocks_for(g * N)), dim3(256), 0, st, g, keys, stride,
               seed_off, planes);
  QRK_LAUNCH("k_frk_unpack", st, k_frk_unpack<N>, dim3((unsigned)g), dim3(256), 0, st, g, keys, stride, secret,
             (uint16_t*)(base + l.b_off), (int16_t*)(base + l.st_off), (uint64_t*)(base + l.s_off),
             (uint64_t*)(base + l.pkh_off));
  if (!secret)
    QRK_LAUNCH("k_frk_pkh", st, k_frk_pkh<N>, dim3((unsigned)g), dim3(64), 0, st, g, keys,
               (uint64_t*)(base + l.pkh_off));
  return launch_status();
}

// f(FP<N>) for the parameter set of `a`
template <class F>
static hipError_t with_n(const AlgInfo& a, F&& f) {
  switch (a.k) {
    case 640: return f(std::integral_constant<int, 640>{});
    case 976: return f(std::integral_constant<int, 976>{});
    case 1344: return f(std::integral_constant<int, 1344>{});
  }
  return hipErrorInvalidValue;
}

}  // namespace frodo
}  // namespace qrk
