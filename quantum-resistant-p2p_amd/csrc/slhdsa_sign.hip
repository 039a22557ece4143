// Batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple key generation and signing, the "f" parameter sets, for gfx950.
//
// The signing half of the reference's SPHINCSSignature (quantum_resistant_p2p/crypto/signatures.py:238-292):
// FIPS 205 Algorithm 18 (slh_keygen_internal) and Algorithm 19 (slh_sign_internal) over n rows at once, in the
// two flavours of slhdsa.hip (Params::fips: message framing and FORS bit order).  Byte-exact with
// tests/slhdsa_spec.py.
//
// A signature is almost only hashing of independent pieces: once H_msg has given the tree and leaf indices,
// every XMSS tree on the hypertree path is known (tree_j, leaf_j are shifts of the digest's index), and a tree
// depends on SK.seed and its address alone, not on what it signs.  Only the d WOTS+ signatures depend on
// roots (layer j signs root j - 1, layer 0 the FORS public key).  So, stream-ordered per chunk of rows:
//
//   k_slhsign_front  one lane per row: R = PRF_msg(SK.prf, opt_rand, M') (HMAC-SHA-256 / -512, truncated) into
//                    the signature, digest = H_msg(R, PK.seed, PK.root, M') (h_msg, shared with verification),
//                    the SHA-2 states after the PK.seed block (public; every later hash starts from them) and
//                    the flag word into scratch.  A row of 2^31 bytes or more, or with decreasing offsets, gets
//                    FLAG_LONG and nothing else.
//   k_slhsign_fors   one workgroup per (row, FORS tree i), 2^a threads: thread j makes sk_j = PRF(FORS_PRF
//                    address) and leaf j = F(sk_j); the tree is reduced through LDS in a levels between
//                    workgroup barriers (all waves serve one row here, so barriers are legal, unlike in the
//                    verify core).  The thread at idx_i stores sk, the one at (idx_i >> z) ^ 1 of level z the
//                    auth node, thread 0 root i to scratch.
//   k_slhsign_xmss   one workgroup per (row, layer): the 2^h' len chains of the tree (PRF, then the full
//                    uniform 15 steps of F) flattened over the threads, chain ends into the leaf's LDS stream,
//                    T_len per leaf, h' levels of H; the auth path of leaf_j goes straight into the signature,
//                    the root to scratch.  With KEYGEN (layer d - 1, tree 0, one workgroup per row) the root
//                    goes to pk and sk instead: key generation.
//   k_slhsign_wots   one workgroup per row, the only stage that needs the roots: the message of layer 0 is
//                    T_k over the FORS roots, of layer j root j - 1; the d len chains flattened over the
//                    threads, each PRF then a uniform 15-step loop `if (s < digit) x = F(x)`.  Before that it
//                    compares the top root with SK's PK.root: a difference (a corrupt key) or FLAG_LONG zeroes
//                    the whole signature row and gives status -1 instead.  The only writer of status; every
//                    row exactly once.
//
// One wave per WOTS+ leaf (2^h' waves per workgroup) would leave 29 of 64 lanes idle for len = 35 and need a
// second pass for 3 of the 67 chains of 256f; the flattened mapping runs the same chains on 5 / 7 / 8 waves
// (three passes for 256f) and keeps 256f off the 1024-thread, 128-VGPR launch bound (profiles/slhdsa/
// sign_resources.md).
//
// Secret handling:
//   * SK.seed and SK.prf are read only from the caller's device buffer (for KeyGen: from the sk the call is
//     writing), never passed as kernel arguments: the runtime's argument pool is not wiped.
//   * Global scratch holds public values only: PK.seed hash states, digest, flags, FORS and XMSS roots.
//   * PRF outputs, the HMAC key pads and every chain value below its published position live in registers
//     only.  LDS holds chain ends (WOTS+ public-key elements), tree nodes and messages: public.  No LDS ever
//     holds a secret, so there is none to overwrite at exit.
//   * Branches, loop bounds and addresses depend on public data only: digits, FORS indices, tree and leaf
//     indices, lengths, flags.  The SHA-2 rounds are straight-line code.
#include "slhdsa_common.cuh"

namespace qrk {
namespace slhdsa {

// scratch of a chunk of C rows, public values only: s512 | s256 | flags | digest | fors_roots | roots
struct SignLayout {
  uint64_t* s512;       // [C][8] the SHA-512 state after PK.seed || 0^(128 - n)   (n > 16 only)
  uint32_t* s256;       // [C][8] the SHA-256 state after PK.seed || 0^(64 - n)
  uint32_t* flags;      // [C]
  uint8_t* digest;      // [C][m]
  uint8_t* fors_roots;  // [C][k][n]
  uint8_t* roots;       // [C][d][n]
  size_t bytes;
};
static SignLayout sign_layout(const Params& P, size_t C, void* scratch) {
  uint8_t* p = (uint8_t*)scratch;
  SignLayout l;
  l.s512 = (uint64_t*)p, p += P.n > 16 ? C * 64 : 0;
  l.s256 = (uint32_t*)p, p += C * 32;
  l.flags = (uint32_t*)p, p += C * 4;
  l.digest = p, p += C * P.m;
  l.fors_roots = p, p += C * P.k * P.n;
  l.roots = p, p += C * P.d * P.n;
  l.bytes = (size_t)(p - (uint8_t*)scratch);
  return l;
}

constexpr int round64(int x) { return (x + 63) / 64 * 64; }
constexpr int fors_threads(int ps) { return 1 << make(ps).a; }
// all chains of one XMSS tree in one pass; 256f (1072 chains) in three passes of 512 threads: its SHA-512 T_len
// and H need more than the 168 VGPRs that nine or more waves per workgroup leave a lane (576 threads spilled)
constexpr int xmss_threads(int ps) { return make(ps).n == 32 ? 512 : round64((1 << make(ps).hp) * make(ps).len()); }
// the d len chains of a row in two passes
constexpr int wots_threads(int ps) { return round64((make(ps).d * make(ps).len() + 1) / 2); }

template <int N>
__device__ __forceinline__ void store_seeds(const uint8_t* pk_seed, const SignLayout& l, size_t row) {
  uint32_t w[16];
  seed_block<N>(pk_seed, w);
  const sha::H8 s = seed_state256(w);  // stored before the next is made: one state in registers at a time
#pragma unroll
  for (int t = 0; t < 8; ++t) l.s256[row * 8 + t] = s.h[t];
  if constexpr (N > 16) {
    const sha::H8x64 b = seed_state512<N>(w);
#pragma unroll
    for (int t = 0; t < 8; ++t) l.s512[row * 8 + t] = b.h[t];
  }
}
template <int N>
__device__ __forceinline__ Seeds<N> load_seeds(const SignLayout& l, size_t row) {
  Seeds<N> sd;
#pragma unroll
  for (int t = 0; t < 8; ++t) sd.s256.h[t] = l.s256[row * 8 + t];
  if constexpr (N > 16) {
#pragma unroll
    for (int t = 0; t < 8; ++t) sd.s512.h[t] = l.s512[row * 8 + t];
  }
  return sd;
}

// The indices of hypertree layer `layer` from those of layer 0 (digest_indices).
template <int PS>
__device__ __forceinline__ void layer_indices(int layer, uint64_t& tree, uint32_t& leaf) {
#pragma unroll 1
  for (int q = 0; q < layer; ++q) next_layer<PS>(tree, leaf);
}

// ------------------------------------------------------------------ R, H_msg, the PK.seed states
template <int PS>
__global__ __launch_bounds__(64) void k_slhsign_front(size_t n, const uint8_t* __restrict__ sk,
                                                      const uint8_t* __restrict__ msg,
                                                      const uint64_t* __restrict__ off,
                                                      const uint8_t* __restrict__ opt_rand,
                                                      const uint8_t* __restrict__ ctx, uint32_t ctx_len,
                                                      uint8_t* __restrict__ sig, SignLayout l) {
  using namespace sha;
  constexpr Params P = make(PS);
  constexpr uint32_t N = P.n, NW = N / 4;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  uint64_t o0;
  uint32_t mlen;
  if (!row_span(off, row, o0, mlen)) {
    l.flags[row] = FLAG_LONG;
    return;
  }
  const uint32_t pre = P.fips ? 2 + ctx_len : 0;
  const uint8_t* prf = sk + row * P.sk() + N;       // SK.prf
  const uint8_t* pkr = sk + row * P.sk() + 2 * N;   // PK.seed || PK.root
  const uint8_t* orand = opt_rand ? opt_rand + row * N : pkr;  // deterministic variant: opt_rand = PK.seed
  const uint8_t* m = msg + o0;
  uint8_t* r = sig + row * P.sig();
  // HMAC(SK.prf, opt_rand || M'): the key is shorter than a block, so the pads are key ^ 0x36.. / 0x5c..
  auto inner_at = [&](uint32_t p) -> uint32_t { return p < N ? orand[p] : frame_at<PS>(p - N, m, ctx, ctx_len); };
  auto zero_at = [](uint32_t) -> uint32_t { return 0u; };
  uint32_t R[NW];
  if constexpr (N == 16) {
    uint32_t kw[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) kw[t] = (t < (int)NW ? be32(prf + 4 * t) : 0u) ^ 0x36363636u;
    H8 in = init();
    compress(in, kw);
    tail(in, 64, N + pre + mlen, inner_at, [](uint32_t, int, uint32_t x) { return x; });
#pragma unroll
    for (int t = 0; t < 16; ++t) kw[t] ^= 0x36363636u ^ 0x5c5c5c5cu;
    H8 o = init();
    compress(o, kw);
    tail(o, 64, 32, zero_at, [&](uint32_t b, int t, uint32_t x) { return (b == 0 && t < 8) ? in.h[t] : x; });
#pragma unroll
    for (int j = 0; j < (int)NW; ++j) R[j] = o.h[j];
  } else {
    uint64_t kw[16];
#pragma unroll
    for (int t = 0; t < 16; ++t)
      kw[t] = (t < (int)NW / 2 ? ((uint64_t)be32(prf + 8 * t) << 32) | be32(prf + 8 * t + 4) : 0ull) ^
              0x3636363636363636ull;
    H8x64 in = init512();
    compress512(in, kw);
    tail512(in, 128, N + pre + mlen, inner_at, [](uint32_t, int, uint64_t x) { return x; });
#pragma unroll
    for (int t = 0; t < 16; ++t) kw[t] ^= 0x3636363636363636ull ^ 0x5c5c5c5c5c5c5c5cull;
    H8x64 o = init512();
    compress512(o, kw);
    tail512(o, 128, 64, zero_at, [&](uint32_t b, int t, uint64_t x) { return (b == 0 && t < 8) ? in.h[t] : x; });
#pragma unroll
    for (int j = 0; j < (int)NW; ++j) R[j] = (uint32_t)(o.h[j >> 1] >> ((j & 1) ? 0 : 32));
  }
  store_node<N>(r, R);
  h_msg<PS>(r, pkr, m, mlen, ctx, ctx_len, l.digest + row * P.m);  // reads back this lane's own R
  store_seeds<N>(pkr, l, row);
  l.flags[row] = 0;
}

// ------------------------------------------------------------------ FORS: one workgroup per (row, tree)
template <int PS>
__global__ __launch_bounds__(fors_threads(PS)) void k_slhsign_fors(const uint8_t* __restrict__ sk,
                                                                   uint8_t* __restrict__ sig, SignLayout l) {
  constexpr Params P = make(PS);
  constexpr int N = P.n, NW = N / 4, T = 1 << P.a;
  __shared__ uint32_t nodes[T][NW];
  const size_t row = blockIdx.x;
  const uint32_t i = blockIdx.y, j = threadIdx.x;
  if (l.flags[row] & FLAG_LONG) return;  // the whole workgroup
  const Seeds<N> sd = load_seeds<N>(l, row);
  const uint8_t* dg = l.digest + row * P.m;
  uint64_t tree;
  uint32_t leaf;
  digest_indices<PS>(dg, tree, leaf);
  const uint32_t idx = fors_index<PS>(dg, (int)i);
  uint8_t* fs = sig + row * P.sig() + N + (size_t)i * (P.a + 1) * N;

  uint32_t x[NW];
  load_node<N>(sk + row * P.sk(), x);  // SK.seed
  Adrs A{0, tree, FORS_PRF, leaf, 0, (i << P.a) + j};
  hash_f<N>(sd, A, x);  // sk_j: published for j = idx_i only
  if (j == idx) store_node<N>(fs, x);
  A.type = FORS_TREE;
  hash_f<N>(sd, A, x);  // leaf j
#pragma unroll 1
  for (int z = 0; z < P.a; ++z) {
    if (j < (uint32_t)(T >> z)) {
      if (j == ((idx >> z) ^ 1)) store_node<N>(fs + (z + 1) * N, x);
#pragma unroll
      for (int w = 0; w < NW; ++w) nodes[j][w] = x[w];
    }
    __syncthreads();
    if (j < (uint32_t)(T >> (z + 1))) {
      uint32_t right[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) x[w] = nodes[2 * j][w], right[w] = nodes[2 * j + 1][w];
      hash_h<N>(sd, Adrs{0, tree, FORS_TREE, leaf, (uint32_t)z + 1, (i << (P.a - z - 1)) + j}, x, right, false);
    }
    __syncthreads();
  }
  if (j == 0) store_node<N>(l.fors_roots + (row * P.k + i) * N, x);
}

// ------------------------------------------------------------------ one XMSS tree per workgroup
// sign: grid (rows, d), sk = the caller's keys, kg_pk = kg_sk = NULL.  KEYGEN: grid (rows), sk = kg_sk = the
// secret keys being written (SK.seed already in place), the root goes to kg_pk and kg_sk.
template <int PS, bool KEYGEN>
__global__ __launch_bounds__(xmss_threads(PS)) void k_slhsign_xmss(const uint8_t* sk, uint8_t* sig, uint8_t* kg_pk,
                                                                   uint8_t* kg_sk, SignLayout l) {
  constexpr Params P = make(PS);
  constexpr int N = P.n, NW = N / 4, LEN = P.len(), LEAVES = 1 << P.hp, THREADS = xmss_threads(PS);
  constexpr int SLICE = (22 + LEN * N + 2 + 15) / 16 * 8;  // uint16 units, slices 16-byte aligned
  __shared__ __attribute__((aligned(16))) uint16_t lds[LEAVES][SLICE];
  __shared__ uint32_t tn[LEAVES][NW];
  const size_t row = blockIdx.x;
  const uint32_t layer = KEYGEN ? P.d - 1 : blockIdx.y, tid = threadIdx.x;
  if (!KEYGEN && (l.flags[row] & FLAG_LONG)) return;  // the whole workgroup
  const Seeds<N> sd = load_seeds<N>(l, row);
  uint64_t tree = 0;
  uint32_t leaf = 0;
  if (!KEYGEN) {
    digest_indices<PS>(l.digest + row * P.m, tree, leaf);
    layer_indices<PS>((int)layer, tree, leaf);
  }
  uint32_t seed[NW];
  load_node<N>(sk + row * P.sk(), seed);  // SK.seed

#pragma unroll 1
  for (uint32_t it = tid; it < (uint32_t)(LEAVES * LEN); it += THREADS) {
    const uint32_t lf = it / LEN, c = it % LEN;
    uint32_t x[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] = seed[w];
    Adrs A{layer, tree, WOTS_PRF, lf, c, 0};
    hash_f<N>(sd, A, x);  // the chain's secret start; x leaves registers only as the chain end
    A.type = WOTS_HASH;
#pragma unroll 1
    for (uint32_t s = 0; s < 15; ++s) {
      A.w3 = s;
      hash_f<N>(sd, A, x);
    }
    lds_put_node<N>(lds[lf], (int)c, x);
  }
  if (tid < (uint32_t)LEAVES) lds_put_adrs(lds[tid], Adrs{layer, tree, WOTS_PK, tid, 0, 0});
  __syncthreads();
  uint32_t node[NW] = {};
  if (tid < (uint32_t)LEAVES) t_lds<N>(sd, lds[tid], 22 + LEN * N, node);  // leaf tid
#pragma unroll 1
  for (int z = 0; z < P.hp; ++z) {
    if (tid < (uint32_t)(LEAVES >> z)) {
      if (!KEYGEN && tid == ((leaf >> z) ^ 1))  // the auth path of leaf_j, after the layer's len chain values
        store_node<N>(sig + row * P.sig() + N + P.fors_bytes() + (size_t)layer * P.xmss_bytes() + (size_t)(LEN + z) * N,
                      node);
#pragma unroll
      for (int w = 0; w < NW; ++w) tn[tid][w] = node[w];
    }
    __syncthreads();
    if (tid < (uint32_t)(LEAVES >> (z + 1))) {
      uint32_t right[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) node[w] = tn[2 * tid][w], right[w] = tn[2 * tid + 1][w];
      hash_h<N>(sd, Adrs{layer, tree, TREE, 0, (uint32_t)z + 1, tid}, node, right, false);
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (KEYGEN) {
      store_node<N>(kg_pk + row * P.pk() + N, node);
      store_node<N>(kg_sk + row * P.sk() + 3 * N, node);
    } else {
      store_node<N>(l.roots + (row * P.d + layer) * N, node);
    }
  }
}

// ------------------------------------------------------------------ the d WOTS+ signatures, status
template <int PS>
__global__ __launch_bounds__(wots_threads(PS)) void k_slhsign_wots(const uint8_t* __restrict__ sk,
                                                                   uint8_t* __restrict__ sig,
                                                                   int32_t* __restrict__ status, SignLayout l) {
  constexpr Params P = make(PS);
  constexpr int N = P.n, NW = N / 4, LEN = P.len(), THREADS = wots_threads(PS);
  constexpr int SLICE = (22 + P.k * N + 2 + 15) / 16 * 8;
  __shared__ __attribute__((aligned(16))) uint16_t slice[SLICE];  // ADRSc || the k FORS roots
  __shared__ uint32_t msgs[P.d * NW];                             // the message of every layer
  __shared__ uint32_t csum[P.d];
  const size_t row = blockIdx.x;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint8_t* skr = sk + row * P.sk();
  uint8_t* sg = sig + row * P.sig();

  // a row the front refused, or a key whose PK.root is not the root of its SK.seed: zeros and -1
  uint32_t bad = l.flags[row] & FLAG_LONG;
  if (!bad) {
    const uint8_t* top = l.roots + (row * P.d + P.d - 1) * N;
#pragma unroll
    for (int j = 0; j < NW; ++j) bad |= be32(top + 4 * j) ^ be32(skr + 3 * N + 4 * j);
  }
  if (bad) {  // the whole workgroup
    for (uint32_t b = tid; b < (uint32_t)P.sig(); b += THREADS) sg[b] = 0;
    if (tid == 0) status[row] = -1;
    return;
  }

  const Seeds<N> sd = load_seeds<N>(l, row);
  uint64_t tree0;
  uint32_t leaf0;
  digest_indices<PS>(l.digest + row * P.m, tree0, leaf0);
  if (tid < 64) {  // wave 0: T_k over the FORS roots, every lane redundantly as in the verify core
    if (lane < (uint32_t)P.k) {
      uint32_t x[NW];
      load_node<N>(l.fors_roots + (row * P.k + lane) * N, x);
      lds_put_node<N>(slice, (int)lane, x);
    }
    if (lane == 0) lds_put_adrs(slice, Adrs{0, tree0, FORS_ROOTS, leaf0, 0, 0});
    wave_sync();
    uint32_t node[NW];
    t_lds<N>(sd, slice, 22 + P.k * N, node);
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) msgs[w] = node[w];
    }
  }
  for (uint32_t t = tid; t < (uint32_t)((P.d - 1) * NW); t += THREADS)  // layer j signs root j - 1
    msgs[NW + t] = be32(l.roots + row * P.d * N + 4 * t);
  __syncthreads();
  if (tid < (uint32_t)P.d) csum[tid] = wots_csum<N>(msgs + tid * NW);
  __syncthreads();

  uint32_t seed[NW];
  load_node<N>(skr, seed);  // SK.seed
#pragma unroll 1
  for (uint32_t it = tid; it < (uint32_t)(P.d * LEN); it += THREADS) {
    const uint32_t layer = it / LEN, c = it % LEN;
    const uint32_t digit = c < (uint32_t)P.len1() ? wots_msg_digit(c, msgs[layer * NW + (c >> 3)])  // from LDS
                                                   : wots_csum_digit<N>(c, csum[layer]);
    uint64_t tree = tree0;
    uint32_t leaf = leaf0;
    layer_indices<PS>((int)layer, tree, leaf);
    uint32_t x[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] = seed[w];
    Adrs A{layer, tree, WOTS_PRF, leaf, c, 0};
    hash_f<N>(sd, A, x);
    A.type = WOTS_HASH;
#pragma unroll 1
    for (uint32_t s = 0; s < 15; ++s) {  // uniform trip count; the digit is public (it is in the signature)
      if (s < digit) {
        A.w3 = s;
        hash_f<N>(sd, A, x);
      }
    }
    store_node<N>(sg + N + P.fors_bytes() + (size_t)layer * P.xmss_bytes() + (size_t)c * N, x);
  }
  if (tid == 0) status[row] = 0;
}

// ------------------------------------------------------------------ KeyGen: seeds into place
template <int PS>
__global__ __launch_bounds__(64) void k_slhsign_kg_front(size_t n, const uint8_t* __restrict__ seeds,
                                                         uint8_t* __restrict__ pk, uint8_t* __restrict__ sk,
                                                         SignLayout l) {
  constexpr Params P = make(PS);
  constexpr int N = P.n;
  const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  const uint8_t* s = seeds + row * 3 * N;  // SK.seed || SK.prf || PK.seed
  for (int b = 0; b < 3 * N; ++b) sk[row * P.sk() + b] = s[b];
  for (int b = 0; b < N; ++b) pk[row * P.pk() + b] = s[2 * N + b];
  store_seeds<N>(s + 2 * N, l, row);
}

// Only the front (framing) and FORS (index bit order) kernels depend on the flavour: the others are instantiated
// once per parameter set (SET = the round-3.1 member of the pair).
template <int PS>
static hipError_t run_keypair(size_t n, const uint8_t* seeds, uint8_t* pk, uint8_t* sk, void* scratch, hipStream_t st) {
  const SignLayout l = sign_layout(make(PS), n, scratch);
  QRK_LAUNCH("k_slhsign_kg_front", st, k_slhsign_kg_front<PS>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n,
             seeds, pk, sk, l);
  QRK_LAUNCH("k_slhsign_xmss", st, (k_slhsign_xmss<PS, true>), dim3((unsigned)n), dim3(xmss_threads(PS)), 0, st,
             (const uint8_t*)sk, (uint8_t*)nullptr, pk, sk, l);
  return launch_status();
}

template <int PS>
static hipError_t run_sign(size_t n, const uint8_t* sk, const uint8_t* msg, const uint64_t* off,
                           const uint8_t* opt_rand, const uint8_t* ctx, size_t ctx_len, uint8_t* sig, int32_t* status,
                           void* scratch, hipStream_t st) {
  constexpr Params P = make(PS);
  constexpr int SET = PS & ~1;
  const SignLayout l = sign_layout(P, n, scratch);
  const unsigned rows = (unsigned)n;
  QRK_LAUNCH("k_slhsign_front", st, k_slhsign_front<PS>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, sk, msg,
             off, opt_rand, ctx, (uint32_t)ctx_len, sig, l);
  QRK_LAUNCH("k_slhsign_fors", st, k_slhsign_fors<PS>, dim3(rows, P.k), dim3(fors_threads(PS)), 0, st, sk, sig, l);
  QRK_LAUNCH("k_slhsign_xmss", st, (k_slhsign_xmss<SET, false>), dim3(rows, P.d), dim3(xmss_threads(PS)), 0, st, sk, sig,
             (uint8_t*)nullptr, (uint8_t*)nullptr, l);
  QRK_LAUNCH("k_slhsign_wots", st, k_slhsign_wots<SET>, dim3(rows), dim3(wots_threads(PS)), 0, st, sk, sig, status, l);
  return launch_status();
}

}  // namespace slhdsa

size_t slhdsa_sign_scratch_bytes(int which, size_t chunk) {
  return slhdsa::sign_layout(slhdsa::make(which), chunk, nullptr).bytes;
}

hipError_t slhdsa_keypair(int which, size_t n, const uint8_t* seeds, uint8_t* pk, uint8_t* sk, void* scratch,
                          hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > SLHDSA_SIGN_MAX_ROWS) return hipErrorInvalidValue;
  return with_which<6>(which, [&](auto ps) {  // Algorithm 18 has no flavour
    return slhdsa::run_keypair<decltype(ps)::value & ~1>(n, seeds, pk, sk, scratch, st);
  });
}

hipError_t slhdsa_sign(int which, size_t n, const uint8_t* sk, const uint8_t* msg, const uint64_t* msg_off,
                       const uint8_t* opt_rand, const uint8_t* ctx_str, size_t ctx_len, uint8_t* sig, int32_t* status,
                       void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (ctx_len > 255 || (ctx_len && !slhdsa_is_fips(which)) || n > SLHDSA_SIGN_MAX_ROWS) return hipErrorInvalidValue;
  return with_which<6>(which, [&](auto ps) {
    return slhdsa::run_sign<decltype(ps)::value>(n, sk, msg, msg_off, opt_rand, ctx_str, ctx_len, sig, status, scratch,
                                                 st);
  });
}

}  // namespace qrk
