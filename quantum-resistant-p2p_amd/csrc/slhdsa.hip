// Batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple verification, the "f" parameter sets, for gfx950.
//
// The reference's SPHINCSSignature.verify (quantum_resistant_p2p/crypto/signatures.py:294-315, called like
// ML-DSA's from app/messaging.py:721, 933, 1174, 1480) over n rows at once.  Two names per parameter set:
// "SPHINCS+-SHA2-{128,192,256}f-simple" is the round-3.1 submission as liboqs ships it,
// "SLH-DSA-SHA2-{128,192,256}f" is FIPS 205 pure SLH-DSA (Algorithm 24 over Algorithm 20).  For SHA2
// "simple" verification they differ in two places only (Params::fips): the message framing in
// k_slhdsa_front (FIPS 205: M' = 0 || len(ctx) || ctx || M; round 3.1: M) and the FORS index extraction in
// fors_index (FIPS 205: base_2b, most significant bit first; round 3.1 message_to_indices: least
// significant bit first within each byte).  Everything else is shared.
//
// Two stream-ordered launches per chunk:
//
//   k_slhdsa_front  one lane per row: digest = H_msg(R, PK.seed, PK.root, M') = MGF1-SHA-X(R || PK.seed ||
//                   SHA-X(R || PK.seed || PK.root || M'), m), X = 256 for n = 16 and 512 otherwise; a row
//                   of 2^31 bytes or more (or with decreasing offsets) gets FLAG_LONG and nothing else
//   k_slhdsa_core   one 64-lane wave per row, four rows per workgroup: the SHA-256 (and for n > 16 the
//                   SHA-512) state after the PK.seed block once, so that every F, H and short T_l is one
//                   compression; FORS with lane i < k on tree i (F, then a H-steps), the k roots through
//                   LDS to T_k; then per hypertree layer the len WOTS+ chains over the lanes (67 > 64
//                   for n = 32: the lanes loop), each a uniform 15-step loop `if (s >= digit) x = F(x)`,
//                   the chain ends through LDS to T_len, h' H-steps to the layer's root; finally the
//                   comparison with PK.root
//
// The waves of a workgroup serve different rows and some lie past n, so the core kernel has no
// workgroup-wide barrier at all: each wave owns one slice of LDS and orders its own writes and reads
// (wave_sync).  T_k, T_len and the H-steps run redundantly in every lane of the wave (uniform values, so
// nothing is broadcast).  k_slhdsa_core is the only writer of status and writes every row exactly once:
// 0 when the flag word is 0, else -1.  Every input of verification is public, so the kernels branch on
// data.  Nothing here may be copied into a signing path.
#include <cstring>

#include "slhdsa_common.cuh"

namespace qrk {
namespace slhdsa {

// ------------------------------------------------------------------ H_msg
template <int PS>
__global__ __launch_bounds__(64) void k_slhdsa_front(size_t n, const uint8_t* __restrict__ pk,
                                                     const uint8_t* __restrict__ msg,
                                                     const uint64_t* __restrict__ off,
                                                     const uint8_t* __restrict__ sig,
                                                     const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                                     uint8_t* __restrict__ digest, uint32_t* __restrict__ flags) {
  constexpr Params P = make(PS);
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  uint64_t o0;
  uint32_t mlen;
  if (!row_span(off, row, o0, mlen)) {
    flags[row] = FLAG_LONG;
    return;
  }
  h_msg<PS>(sig + row * P.sig(), pk + row * P.pk(), msg + o0, mlen, ctx, ctx_len, digest + row * P.m);
  flags[row] = 0;
}

// The trace outputs (tests: qrk_dbg_slhdsa_verify_trace) are stored only by the TRACE instantiation.
template <int PS, bool TRACE>
__global__ __launch_bounds__(256) void k_slhdsa_core(size_t n, const uint8_t* __restrict__ pk,
                                                     const uint8_t* __restrict__ sig,
                                                     const uint8_t* __restrict__ digest,
                                                     const uint32_t* __restrict__ flags, int32_t* __restrict__ status,
                                                     SlhdsaTrace tr) {
  constexpr Params P = make(PS);
  constexpr int N = P.n, NW = N / 4, LEN = P.len();
  constexpr int MAXL = LEN > P.k ? LEN : P.k;
  constexpr int SLICE = (22 + MAXL * N + 2 + 15) / 16 * 8;  // uint16 units, slices 16-byte aligned
  __shared__ __attribute__((aligned(16))) uint16_t lds[4][SLICE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wv;
  if (row >= n) return;  // no barrier follows: the other waves of the workgroup go on alone
  uint16_t* slice = lds[wv];
  if (flags[row] & FLAG_LONG) {
    if (lane == 0) status[row] = -1;
    if (TRACE) {
      for (int b = lane; b < P.m; b += 64) tr.digest[row * P.m + b] = 0;
      for (int b = lane; b < N; b += 64) tr.fors_pk[row * N + b] = 0;
      for (int b = lane; b < P.d * N; b += 64) tr.roots[row * P.d * N + b] = 0;
      if (lane == 0) tr.flags[row] = FLAG_LONG;
    }
    return;
  }
  const uint8_t* pkr = pk + row * P.pk();
  const uint8_t* sg = sig + row * P.sig();
  const uint8_t* dg = digest + row * P.m;

  const Seeds<N> sd = seed_states<N>(pkr);
  uint64_t tree;
  uint32_t leaf;
  digest_indices<PS>(dg, tree, leaf);

  // ---- FORS: lane i < k reconstructs root i
  if (lane < P.k) {
    const uint32_t idx = fors_index<PS>(dg, lane);
    const uint8_t* fs = sg + N + (size_t)lane * (P.a + 1) * N;
    uint32_t x[NW], au[NW];
    load_node<N>(fs, x);
    Adrs A{0, tree, FORS_TREE, leaf, 0, ((uint32_t)lane << P.a) + idx};
    hash_f<N>(sd, A, x);
#pragma unroll 1
    for (int j = 0; j < P.a; ++j) {
      load_node<N>(fs + (j + 1) * N, au);
      A.w2 = j + 1;
      A.w3 = ((uint32_t)lane << (P.a - j - 1)) + (idx >> (j + 1));
      hash_h<N>(sd, A, x, au, (idx >> j) & 1);
    }
    lds_put_node<N>(slice, lane, x);
  }
  if (lane == 0) lds_put_adrs(slice, Adrs{0, tree, FORS_ROOTS, leaf, 0, 0});
  wave_sync();
  uint32_t node[NW];
  t_lds<N>(sd, slice, 22 + P.k * N, node);
  wave_sync();
  if (TRACE && lane == 0) store_node<N>(tr.fors_pk + row * N, node);

  // ---- hypertree
  const uint8_t* xs = sg + N + P.fors_bytes();
#pragma unroll 1
  for (int layer = 0; layer < P.d; ++layer, xs += P.xmss_bytes()) {
    const uint32_t csum = wots_csum<N>(node);
    for (int c = lane; c < LEN; c += 64) {
      uint32_t digit;
      if (c < P.len1()) {
        uint32_t wsel = 0;  // node[c >> 3], from registers
#pragma unroll
        for (int j = 0; j < NW; ++j) wsel = (c >> 3) == j ? node[j] : wsel;
        digit = wots_msg_digit(c, wsel);
      } else {
        digit = wots_csum_digit<N>(c, csum);
      }
      uint32_t x[NW];
      load_node<N>(xs + (size_t)c * N, x);
      Adrs A{(uint32_t)layer, tree, WOTS_HASH, leaf, (uint32_t)c, 0};
#pragma unroll 1
      for (uint32_t s = 0; s < 15; ++s) {
        if (s >= digit) {
          A.w3 = s;
          hash_f<N>(sd, A, x);
        }
      }
      lds_put_node<N>(slice, c, x);
    }
    if (lane == 0) lds_put_adrs(slice, Adrs{(uint32_t)layer, tree, WOTS_PK, leaf, 0, 0});
    wave_sync();
    t_lds<N>(sd, slice, 22 + LEN * N, node);
    wave_sync();
#pragma unroll 1
    for (int j = 0; j < P.hp; ++j) {
      uint32_t au[NW];
      load_node<N>(xs + (size_t)(LEN + j) * N, au);
      hash_h<N>(sd, Adrs{(uint32_t)layer, tree, TREE, 0, (uint32_t)j + 1, leaf >> (j + 1)}, node, au, (leaf >> j) & 1);
    }
    if (TRACE && lane == 0) store_node<N>(tr.roots + (row * P.d + layer) * N, node);
    next_layer<PS>(tree, leaf);
  }

  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < NW; ++j) diff |= node[j] ^ be32(pkr + N + 4 * j);
  const uint32_t fl = diff ? FLAG_ROOT : 0;
  if (lane == 0) status[row] = fl ? -1 : 0;
  if (TRACE) {
    for (int b = lane; b < P.m; b += 64) tr.digest[row * P.m + b] = dg[b];
    if (lane == 0) tr.flags[row] = fl;
  }
}

// scratch of a chunk of C rows: flags | digest
struct Layout {
  uint32_t* flags;
  uint8_t* digest;
  size_t bytes;
};
static Layout layout(const Params& P, size_t C, void* scratch) {
  uint8_t* p = (uint8_t*)scratch;
  Layout l;
  l.flags = (uint32_t*)p;
  l.digest = p + C * sizeof(uint32_t);
  l.bytes = C * (sizeof(uint32_t) + P.m);
  return l;
}

template <int PS>
static hipError_t run(size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* off, const uint8_t* sig,
                      const uint8_t* ctx, size_t ctx_len, int32_t* status, const SlhdsaTrace& tr, void* scratch,
                      hipStream_t st) {
  const Layout l = layout(make(PS), n, scratch);
  const dim3 lanes((unsigned)((n + 63) / 64)), waves((unsigned)((n + 3) / 4));
  QRK_LAUNCH("k_slhdsa_front", st, k_slhdsa_front<PS>, lanes, dim3(64), 0, st, n, pk, msg, off, sig, ctx,
             (uint32_t)ctx_len, l.digest, l.flags);
  if (tr.flags)
    QRK_LAUNCH("k_slhdsa_core", st, (k_slhdsa_core<PS, true>), waves, dim3(256), 0, st, n, pk, sig, l.digest, l.flags,
               status, tr);
  else
    QRK_LAUNCH("k_slhdsa_core", st, (k_slhdsa_core<PS, false>), waves, dim3(256), 0, st, n, pk, sig, l.digest, l.flags,
               status, tr);
  return launch_status();
}

}  // namespace slhdsa

int slhdsa_find(const char* name) {
  static const char* const NAMES[6] = {"SPHINCS+-SHA2-128f-simple", "SLH-DSA-SHA2-128f", "SPHINCS+-SHA2-192f-simple",
                                       "SLH-DSA-SHA2-192f",         "SPHINCS+-SHA2-256f-simple", "SLH-DSA-SHA2-256f"};
  for (int i = 0; name && i < 6; ++i)
    if (!strcmp(name, NAMES[i])) return i;
  return -1;
}

bool slhdsa_is_fips(int which) { return which & 1; }

SigSizes slhdsa_sizes(int which) {
  const slhdsa::Params P = slhdsa::make(which);
  return {(size_t)P.pk(), (size_t)P.sk(), (size_t)P.sig(), (size_t)P.n};
}

SlhdsaTrace slhdsa_trace_at(int which, const SlhdsaTrace& t, size_t row) {
  const slhdsa::Params P = slhdsa::make(which);
  if (!t.flags) return t;
  return {t.digest + row * P.m, t.fors_pk + row * P.n, t.roots + row * P.d * P.n, t.flags + row};
}

size_t slhdsa_scratch_bytes(int which, size_t chunk) {
  return slhdsa::layout(slhdsa::make(which), chunk, nullptr).bytes;
}

hipError_t slhdsa_verify(int which, size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* msg_off,
                         const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len, int32_t* status,
                         const SlhdsaTrace& trace, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || (ctx_len && !slhdsa_is_fips(which)) || n > (1u << 24)) return hipErrorInvalidValue;
  return with_which<6>(which, [&](auto ps) {
    return slhdsa::run<decltype(ps)::value>(n, pk, msg, msg_off, sig, ctx_str, ctx_len, status, trace, scratch, st);
  });
}

}  // namespace qrk
