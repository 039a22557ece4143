// Internal host-side interface between the C-ABI (abi_*.cpp) and the kernel
// launchers (mlkem.hip and its path files mlkem_batch.cuh, mlkem_one.cuh, mlkem_kg.cuh, mlkem_keyed.hip, frodo.hip (frodo_kernels.cuh), frodo_keyed.hip (frodo_keyed.cuh), hqc.hip, util.hip, hkdf.hip, wire.hip, aead.hip, aead_long.hip,
// mldsa.hip, mldsa_sign.hip, mldsa_keyed.hip, slhdsa.hip, slhdsa_sign.hip).  Not part of the public ABI.
// The exported test hooks (qrk_dbg_*) are declared in qrkem_debug.h and bound for ctypes in qrkem/_debug.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace qrk {

enum class Family { MLKEM, FRODO, HQC };

struct AlgInfo {
  const char* name;
  Family family;
  int level;        // claimed NIST level (OQS_KEM.claimed_nist_level)
  int k;            // ML-KEM module rank, Frodo n, or HQC security bits (128/192/256)
  size_t pk, sk, ct, ss;
  size_t kp_coins, enc_coins;  // bytes drawn by one keypair / encaps randombytes call
  bool aes;         // Frodo A generated with AES-128 (else SHAKE128)
  bool enabled;     // has a HIP implementation in this build
};

const AlgInfo* find_alg(const char* name);

// Size helpers of the host glue and the launchers: a slot rounded up to 256 bytes, a chunk rounded up to whole
// 64-lane tiles, the grid of `threads` threads in workgroups of `per`.
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t round64(size_t x) { return (x + 63) & ~(size_t)63; }
inline unsigned blocks_for(size_t threads, int per = 256) { return (unsigned)((threads + per - 1) / per); }

// Optional per-kernel HIP-event timing (qrk_ctx_profile): when a context has
// profiling enabled, every QRK_LAUNCH brackets the launch with two events on the
// launch stream; durations are summed per kernel name.
struct KernelTimer {
  virtual void before(const char* name, hipStream_t st) = 0;
  virtual void after(const char* name, hipStream_t st) = 0;
  virtual ~KernelTimer() = default;
};
extern thread_local KernelTimer* g_timer;
// First kernel-launch error of the current library call (HIP resets its last-error state on every
// later successful API call, so a failed launch followed by successful ones would otherwise go
// unnoticed).  The one error channel of the launchers: QRK_LAUNCH and qrk_chk record into it, every
// launcher returns launch_status(), and only launch_begin() clears it.  An ABI call (abi_ctx.h: its
// CallScope, and run_batch / run_rows before each chunk) calls launch_begin() before it launches.
// A launcher's return value is therefore the answer and there is no merge step for an entry point
// to forget; the one thing left to forget is launch_begin(), and that reports an earlier call's
// failure loudly instead of losing this call's.
extern thread_local hipError_t g_launch_err;
// tests only (qrk_dbg_fail_launch): launch_begin() records hipErrorLaunchFailure, as if the call's
// first launch had been rejected (0 = off).  One relaxed load per launch_begin(), none per launch.
extern std::atomic<int> g_dbg_fail_launch;

// stream / event / memset calls inside the launchers: a failure joins g_launch_err
inline void qrk_chk(hipError_t e) {
  if (e != hipSuccess && g_launch_err == hipSuccess) g_launch_err = e;
}
inline void launch_begin() {
  g_launch_err = hipSuccess;
  (void)hipGetLastError();  // discard HIP's stale error state (e.g. a caller's hipErrorNotReady query)
  if (g_dbg_fail_launch.load(std::memory_order_relaxed)) qrk_chk(hipErrorLaunchFailure);
}
inline hipError_t launch_status() { return g_launch_err; }

#define QRK_LAUNCH(NAME, ST, ...)                   \
  do {                                              \
    if (::qrk::g_timer) ::qrk::g_timer->before(NAME, ST); \
    hipLaunchKernelGGL(__VA_ARGS__);                \
    {                                               \
      const hipError_t qrk_le_ = hipGetLastError(); \
      if (qrk_le_ != hipSuccess && qrk_le_ != hipErrorNotReady && ::qrk::g_launch_err == hipSuccess) \
        ::qrk::g_launch_err = qrk_le_;                \
    }                                               \
    if (::qrk::g_timer) ::qrk::g_timer->after(NAME, ST);  \
  } while (0)

// Per-chunk scratch requirement (bytes) for `chunk` handshakes of `a`.
size_t mlkem_scratch_bytes(const AlgInfo& a, size_t chunk);
size_t frodo_scratch_bytes(const AlgInfo& a, size_t chunk);
size_t hqc_scratch_bytes(const AlgInfo& a, size_t chunk);
// Zero the per-handshake key-material records one chunk of n handshakes left in scratch
// (ML-KEM: seeds, m', K', Kbar; FrodoKEM: seedSE || k || pkh || mu', the hashed key; HQC: the
// K-hash message m || u || v and m'), stream-ordered: called after every chunk.
hipError_t mlkem_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st);
// byte offset and length of the ML-KEM per-handshake records (seeds | m' | K' | Kbar) in the
// scratch of a chunk of C handshakes (tests: qrk_dbg_mlkem_records_residue)
void mlkem_records_span(const AlgInfo& a, size_t C, size_t* off, size_t* bytes);
// ML-KEM batches up to this size run as one launch per operation with no scratch key material
size_t mlkem_small_max();
// ML-KEM KeyGen batches up to this size run one workgroup per SampleNTT / PRF item (latency)
size_t mlkem_kg_multi_max();
// flag / counter words of the single-shot multi-workgroup KeyGen (mlkem::CtxState, Streams::kg_cnt)
size_t mlkem_kg_flag_words();
// bytes of the batched sampled matrix of a chunk of `chunk` handshakes (Streams::xof_keep)
size_t mlkem_matrix_bytes(const AlgInfo& a, size_t chunk);
// bytes at the start of the scratch that the n <= mlkem_kg_multi_max() KeyGen kernels use
size_t mlkem_kg_scratch_bytes();
// tests only (qrk_dbg_kg_late): the k_keygen_pipe workgroup role (PRF item or t_hat row) that
// publishes past every bounded wait, -1 (default) none.  Both switches are read (relaxed) at launch
// by whichever thread drives a context while a test thread writes them.
extern std::atomic<int> g_kg_dbg_late;
// tests only (qrk_dbg_fail_after_flip): batched ML-KEM Encaps / Decaps chunks <= 2^15 fail right after
// the fix-up counter parity flip, before any launch (0 = off)
extern std::atomic<int> g_dbg_fail_after_flip;
hipError_t frodo_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st);
hipError_t hqc_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st);

// Launch context of one call: every kernel of the call runs on `main`, the caller's stream (no
// side streams, no cross-stream events: a call is stream-ordered and never blocks the host).
struct Streams {
  hipStream_t main = nullptr;
  // serial schedule: one kernel per launch (per-kernel timings in isolation); otherwise
  // independent kernels of one operation share multi-role launches (ML-KEM, mlkem_batch.cuh)
  bool serial = false;
  // ---- ML-KEM only, from here to the end of the struct (FrodoKEM and HQC read none of it)
  // single-shot completion flag (fine-grained host memory, device address): the one-launch ML-KEM
  // kernels store `ticket` there once their outputs are visible to the host
  uint32_t* done = nullptr;
  uint32_t ticket = 0;
  // per-handshake arrival counters of the multi-workgroup single-shot ML-KEM KeyGen (device,
  // QRK_KG_MULTI_MAX words, zero between calls: the last workgroup of a handshake resets its word)
  uint32_t* kg_cnt = nullptr;
  // host-pointer ML-KEM KeyGen of n <= mlkem_kg_multi_max(): the call's error word (fine-grained host
  // memory, device address, zeroed by the host before the launch).  When set, k_keygen_pipe runs and
  // stores 1 there if a bounded cross-workgroup wait expired; the host then fails the call.
  uint32_t* kg_err = nullptr;
  // single-shot ML-KEM (n == 1, host-pointer call): the public input in host memory (Encaps: pk;
  // Decaps: c), passed as a kernel argument instead of read over PCIe.  Secret inputs are never
  // passed by value: the runtime's kernel-argument pool is not wiped.
  const uint8_t* host_in1 = nullptr;
  // batched ML-KEM Encaps / Decaps at chunks <= 2^15: the context's two SampleNTT fix-up counters
  // (device, zero at allocation) and which one the next call counts into (host; the call flips it
  // and its first launch zeroes the other word, mlkem_batch.cuh rho_source).  Set only by
  // mlkem::CtxState::prepare, which re-zeroes both words after any failed chunk.
  uint32_t* fixc = nullptr;
  int* fixp = nullptr;
  // batched ML-KEM chunks (n > mlkem_small_max()), the KeyGen -> Decaps hand-over of the sampled matrix
  // A_hat (SampleNTT(rho || x || y), a function of rho alone; mlkem::CtxState's kept region).  Set per
  // chunk by CtxState::keep_chunk / kept_chunk alone, null where the chunk takes no part in it.
  // KeyGen writes the chunk's matrix (the batched tiled layout, mlkem_matrix_bytes) to xof_keep instead of
  // the scratch, and every row's rho, 32 bytes apart, to rho_keep: the row's tag.
  uint64_t* xof_keep = nullptr;
  uint64_t* rho_keep = nullptr;
  // Decaps of a chunk of the same geometry reads a row's matrix entries from xof_kept where the rho in
  // its dk equals the row's tag in rho_kept (rows below kept_rows), and samples the other rows as ever.
  const uint64_t* xof_kept = nullptr;
  const uint64_t* rho_kept = nullptr;
  size_t kept_rows = 0;
};

enum class Op { KEYPAIR, ENCAPS, DECAPS };

// Which chunks of a batched ML-KEM KeyGen of n handshakes, in chunks of `chunk` rows (a multiple of 64),
// the context keeps the sampled matrix of: whole batched chunks (more than small_max rows; only the last
// chunk can be shorter), in order, as many as cap_bytes allow.  A kept chunk takes chunk_bytes: its rho
// tags (32 bytes per row, rounded up to 256) and then its matrix (row_bytes = K^2 384 per row), so chunk
// i of the region starts at i * chunk_bytes.  Pure arithmetic: the one place that decides what is kept.
struct KeepPlan {
  size_t batched, kept, tag_bytes, chunk_bytes, bytes;
};
inline KeepPlan mlkem_keep_plan(size_t row_bytes, size_t n, size_t chunk, size_t small_max, size_t cap_bytes) {
  KeepPlan p{0, 0, 0, 0, 0};
  if (n == 0 || chunk == 0) return p;
  const size_t nchunks = (n + chunk - 1) / chunk, last = n - (nchunks - 1) * chunk;
  p.batched = chunk > small_max ? nchunks - (last > small_max ? 0 : 1) : 0;
  p.tag_bytes = (32 * chunk + 255) & ~(size_t)255;
  p.chunk_bytes = p.tag_bytes + row_bytes * chunk;
  p.kept = std::min(p.batched, cap_bytes / p.chunk_bytes);
  p.bytes = p.kept * p.chunk_bytes;
  return p;
}
// The cap on the kept region in bytes: QRK_KEEP_MIB (environment, read at every KeyGen; 0 keeps nothing),
// 8192 MiB by default -- a 2^20 chunk of ML-KEM-1024 is 6.2 GiB, of ML-KEM-768 3.5 GiB.
size_t mlkem_keep_cap_bytes();

// What a context keeps for ML-KEM alone between calls (a member of qrk_ctx; functions and the
// invariants they keep in mlkem_batch.cuh, beside rho_source).  The driver calls these under the
// context lock and touches no field.
namespace mlkem {
struct CtxState {
  // Before the chunks of a call of n handshakes (chunks of `chunk`) on S.main: allocates what the call
  // needs on first use, queues the re-zero an earlier failure left owing, and sets S.kg_cnt, S.fixc and
  // S.fixp.  S.kg_err comes in as the caller was asked for it and is cleared where it does not apply
  // to this call.  scratch: the context's.  On failure *what names the step.
  hipError_t prepare(Streams& S, Op op, size_t n, size_t chunk, void* scratch, size_t scratch_bytes,
                     const char** what);
  // a chunk failed after prepare()
  void chunk_failed(const Streams& S);
  // a zero-copy host call on `st` failed and the stream is idle; pipe_call: it was a KeyGen that handed
  // out the error word
  void keygen_failed(bool pipe_call, void* scratch, size_t scratch_bytes, hipStream_t st);
  void free();
  // tests (qrk_dbg_fixc_words, qrk_dbg_kg_flags_residue): the two fix-up counters and the parity;
  // nonzero words among the KeyGen flag words.  On failure *what names the step.
  hipError_t fix_words(uint32_t* out, int* parity, const char** what) const;
  hipError_t kg_flags_residue(uint64_t* out) const;

  // ---- the kept region: the sampled matrices of the last batched KeyGen and a 32-byte rho tag per row,
  // for Decaps of the same keys on this context (layout: KeepPlan).  Public data, a function of the
  // public rho: wiped with the context's buffers but never for secrecy.  Outputs never depend on the
  // region, only time does: a Decaps row uses a kept entry only where the rho in its dk equals the tag
  // KeyGen stored with that entry, and the region is read only while `keep_valid` (host state, never
  // inferred from device bytes), which every call that writes, fills or frees the region clears first.
  // A KeyGen of n handshakes in chunks of `chunk` begins: the region is invalid from here.  Sizes it for
  // plan.kept chunks; before a larger one replaces it quiesce(arg) must wait for the context's last use.
  // An allocation that fails leaves no region (and no HIP error): the KeyGen keeps nothing.
  void keep_begin(const AlgInfo& a, size_t n, size_t chunk, size_t cap_bytes, void (*quiesce)(void*), void* arg);
  // chunk `idx` of that KeyGen: S.xof_keep / S.rho_keep, null when the chunk is not kept
  void keep_chunk(Streams& S, size_t idx) const;
  // every chunk of that KeyGen is queued: the region is valid for its kept chunks
  void keep_commit();
  // chunk `idx` (m rows) of a Decaps in chunks of `chunk`: S.xof_kept / S.rho_kept / S.kept_rows where the
  // region is valid and holds a chunk of the same parameter set and geometry, null otherwise
  void kept_chunk(Streams& S, const AlgInfo& a, size_t chunk, size_t idx, size_t m) const;
  // the region is invalid from here; its span, for the context's fill and cleanse
  void keep_invalidate(void** p, size_t* bytes);

 private:
  uint8_t* keep = nullptr;  // the kept region
  size_t keep_bytes = 0;    // ... as allocated
  bool keep_valid = false;
  int keep_k = 0;           // what it holds: the parameter set, and the KeyGen's n, chunk and kept chunks
  size_t keep_n = 0, keep_chunk_rows = 0, keep_chunks = 0;
  hipError_t kg_rezero(void* scratch, size_t scratch_bytes, hipStream_t st);
  uint32_t* kg_cnt = nullptr;  // single-shot KeyGen arrival counters / flag words (mlkem_kg_flag_words)
  bool kg_dirty = false;       // a pipelined KeyGen failed: a straggler may have set a flag word
                               // after the collector's reset, or stored scratch after its wipe
  uint32_t* fixc = nullptr;    // SampleNTT fix-up counters of chunks <= 2^15 (Streams::fixc)
  int fixp = 0;                // the counter the next such chunk counts into
  bool fixc_dirty = false;     // a chunk's launches failed after the parity flip: re-zero both
};
}  // namespace mlkem

// All pointers are device pointers; n handshakes processed as one chunk
// (the caller splits large batches).  Return hipError_t.  The three families share one signature
// per operation (abi_kem.cpp keeps them in a table): `status` may be NULL, and a launcher that reports
// nothing ignores it.  ML-KEM Encaps writes status[i] = -1 when ek fails the FIPS 203 modulus check,
// HQC Decaps when the re-encryption check fails (ss = K(sigma || ct) is still written, the
// OQS_KEM_decaps return of liboqs), and both write 0 otherwise.
hipError_t mlkem_keypair(const AlgInfo& a, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins,
                         void* scratch, const Streams& st);
hipError_t mlkem_encaps(const AlgInfo& a, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk,
                        const uint8_t* coins, int32_t* status, void* scratch, const Streams& st);
hipError_t mlkem_decaps(const AlgInfo& a, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk,
                        int32_t* status, void* scratch, const Streams& st);

// ML-KEM key sets (mlkem_keyed.hip): g keys expanded once into one device allocation of mlkem_keyset_bytes, and
// Encaps / Decaps of n rows that name their key by index.  MlkemKeys is the view of that allocation
// (mlkem_keyset_view; device pointers): A_hat, one contiguous 384-byte entry of 12-bit coefficients per
// (key, x, y), [g][k k][384]; the key bytes [g][stride], ek rows for a public set and dk rows (secret: they hold
// s_hat and z) for a secret one; a public set adds H(ek) [g][32] and a word per key that is nonzero where ek
// fails the FIPS 203 modulus check.  key_index [n] (device; NULL: every row uses key 0) is checked against g on
// the device before any address is formed from it: a row with an index >= g gets status -1 and an all-zero ct /
// ss row.  Everything else as mlkem_encaps / mlkem_decaps, whose bytes these return.  The scratch
// (mlkem_keyed_scratch_bytes) holds the PRF words and seeds | m' | K' | Kbar per row and no matrix;
// mlkem_keyed_cleanse zeroes the four records after every chunk.
struct MlkemKeys {
  uint32_t g = 0;
  const void* A = nullptr;
  const uint8_t* keys = nullptr;
  size_t stride = 0;
  const void* h = nullptr;
  const uint32_t* bad = nullptr;
};
size_t mlkem_keyset_bytes(const AlgInfo& a, bool secret, size_t g);
MlkemKeys mlkem_keyset_view(const AlgInfo& a, bool secret, size_t g, void* mem);
// keys: pk [g][pk] or sk [g][sk]; mem: mlkem_keyset_bytes, every byte of it is written
hipError_t mlkem_keyset_expand(const AlgInfo& a, bool secret, size_t g, const uint8_t* keys, void* mem,
                               hipStream_t st);
size_t mlkem_keyed_scratch_bytes(const AlgInfo& a, size_t chunk);
hipError_t mlkem_keyed_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st);
hipError_t mlkem_encaps_keyed(const AlgInfo& a, const MlkemKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ct,
                              uint8_t* ss, const uint8_t* coins, int32_t* status, void* scratch, const Streams& s);
hipError_t mlkem_decaps_keyed(const AlgInfo& a, const MlkemKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ss,
                              const uint8_t* ct, int32_t* status, void* scratch, const Streams& s);

hipError_t frodo_keypair(const AlgInfo& a, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins,
                         void* scratch, const Streams& st);
hipError_t frodo_encaps(const AlgInfo& a, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk,
                        const uint8_t* coins, int32_t* status, void* scratch, const Streams& st);
hipError_t frodo_decaps(const AlgInfo& a, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk,
                        int32_t* status, void* scratch, const Streams& st);

// tests only (qrk_dbg_frodo_decaps_trace): after frodo_decaps on the same chunk and scratch and before
// frodo_cleanse, mu' = Decode(C - B'S) of each handshake to mu_out[n][32] (len_mu bytes, then zeros)
hipError_t frodo_trace_mu(const AlgInfo& a, size_t n, void* scratch, uint8_t* mu_out, hipStream_t st);
// tests only (qrk_dbg_frodo_sample): k_fr_sample (kg: its KeyGen instantiation) on the caller's 16-bit words, spec
// order, laid out as the stream kernels write them; the sampled regions of the scratch copied out whole:
// s8 [n][8][NP], e16 [n][8 N] and, Encaps only, epp16 [n][64]
hipError_t frodo_dbg_sample(const AlgInfo& a, bool kg, size_t n, const uint16_t* words, int8_t* s8, int16_t* e16,
                            int16_t* epp16, void* scratch, hipStream_t st);
// tests only (qrk_dbg_frodo_from_samples): the launches of frodo_encaps (kg: frodo_keypair) after the sampler, on
// sample matrices in the layout above.  Encaps: in = pk, out = ct.  KeyGen: in = seedA [n][16], out = pk, and
// k_fr_kg_pack's part of sk.  The caller has checked the samples against frodo_sample_max / zero pad columns.
hipError_t frodo_dbg_from_samples(const AlgInfo& a, bool kg, size_t n, const int8_t* s8, const int16_t* e16,
                                  const int16_t* epp16, const uint8_t* in, const uint8_t* mu, uint8_t* out,
                                  uint8_t* sk, void* scratch, hipStream_t st);
int frodo_sample_max(const AlgInfo& a);       // largest |sample| of the parameter set's CDF table: 12 / 10 / 6
size_t frodo_sample_pitch(const AlgInfo& a);  // NP, the row pitch of S' / S^T in the scratch: n rounded up to 128

// FrodoKEM key sets (frodo_keyed.hip): g keys expanded once into one device allocation of frodo_keyset_bytes, and
// Encaps / Decaps of n rows that name their key by index.  FrodoKeys is the view of that allocation
// (frodo_keyset_view; device pointers): A as two int8 limb planes per key, [g][lo, hi][N columns][N rows]
// (A = 256 hi + lo); B u16 [g][N][8]; pkh [g][32]; a secret set adds S^T int16 [g][8][N] and s [g][32] (both
// secret).  key_index [n] (device; NULL: every row uses key 0) is checked against g on the device before any address
// is formed from it: a row with an index >= g joins no tile of the product, gets status -1 and an all-zero ct / ss
// row.  Everything else as frodo_encaps / frodo_decaps, whose bytes these return; status is written for every row.
// The scratch (frodo_keyed_scratch_bytes, which depends on g for the grouping tables) holds the per-row call's
// regions with whole sums of S'A in place of the per-wave partials; frodo_keyed_cleanse zeroes seeds | kk after
// every chunk.
struct FrodoKeys {
  uint32_t g = 0;
  const int8_t* planes = nullptr;
  const uint16_t* B = nullptr;
  const uint64_t* pkh = nullptr;
  const int16_t* St = nullptr;
  const uint64_t* s = nullptr;
};
size_t frodo_keyset_bytes(const AlgInfo& a, bool secret, size_t g);
FrodoKeys frodo_keyset_view(const AlgInfo& a, bool secret, size_t g, void* mem);
// keys: pk [g][pk] or sk [g][sk]; mem: frodo_keyset_bytes, every byte of it is written
hipError_t frodo_keyset_expand(const AlgInfo& a, bool secret, size_t g, const uint8_t* keys, void* mem,
                               hipStream_t st);
int frodo_keyed_tile_rows();  // same-key rows per tile of the product kernel
size_t frodo_keyed_scratch_bytes(const AlgInfo& a, size_t chunk, size_t g);
hipError_t frodo_keyed_cleanse(const AlgInfo& a, size_t n, size_t g, void* scratch, hipStream_t st);
hipError_t frodo_encaps_keyed(const AlgInfo& a, const FrodoKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ct,
                              uint8_t* ss, const uint8_t* coins, int32_t* status, void* scratch, const Streams& s);
hipError_t frodo_decaps_keyed(const AlgInfo& a, const FrodoKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ss,
                              const uint8_t* ct, int32_t* status, void* scratch, const Streams& s);

hipError_t hqc_keypair(const AlgInfo& a, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                       const Streams& st);
hipError_t hqc_encaps(const AlgInfo& a, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                      int32_t* status, void* scratch, const Streams& st);
hipError_t hqc_decaps(const AlgInfo& a, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, int32_t* status,
                      void* scratch, const Streams& st);
// Fixed-weight supports from n vectors of random words r[n][w] (kind 0: w = the key weight,
// 1: w = the encryption weight w_r = w_e): sup_i = i + floor(r_i (n - i) / 2^32), deduplicated.
hipError_t hqc_supports(const AlgInfo& a, int kind, size_t n, const uint32_t* r, uint32_t* sup, hipStream_t st);
// The decoder stages of Decaps alone (dec_expand, RM decode, RS decode) on `scratch`: the RM
// symbols syms[n][n1] and the decoded message mprime[n][k], dense.  With t_out (tests only,
// qrk_dbg_hqc_decaps_trace; else NULL) k_hqc_decode also stores T = v - u y to t_out[n][VB].
hipError_t hqc_code_decode(const AlgInfo& a, size_t n, const uint8_t* sk, const uint8_t* ct, uint8_t* t_out,
                           uint8_t* syms, uint8_t* mprime, void* scratch, hipStream_t st);

// SHAKE256("qrk-bench" || LE64(seed) || LE64(first + i), len) for i < n, len <= 136.
hipError_t bench_coins(size_t n, size_t len, uint64_t seed, uint64_t first, uint8_t* out, hipStream_t st);

// out_i = SHA3-256(a_i || b_i) (32 B per record); b may be NULL with bl = 0.
hipError_t digest_rows(size_t n, const uint8_t* a, size_t al, const uint8_t* b, size_t bl, uint8_t* out,
                       hipStream_t st);

// Flip one bit of ct_i for the indices selected by SHAKE256-derived Bernoulli(1/2)
// (bench config 5).  mode: 0 none, 1 all, 2 mixed.
hipError_t tamper_ciphertexts(size_t n, size_t ctlen, uint64_t seed, int mode, uint8_t* ct, hipStream_t st);

// HKDF-SHA256 (RFC 5869), one lane per key (hkdf.hip).  info_off (n+1 offsets) may be
// NULL, then every key uses info[0 .. info_len).  L <= 8160.
hipError_t hkdf_sha256(size_t n, const uint8_t* ikm, size_t ikm_len, size_t ikm_stride, const uint8_t* salt,
                       size_t salt_len, const uint8_t* info, const uint64_t* info_off, size_t info_len, size_t L,
                       uint8_t* okm, size_t okm_stride, hipStream_t st);
// agree_i = (a_i == b_i), len bytes each
hipError_t keys_equal(size_t n, const uint8_t* a, const uint8_t* b, size_t len, int32_t* agree, hipStream_t st);

// AEAD over n messages, one lane per message (aead.hip).  keys [n][32]; nonces [n][12]; ragged bytes with
// n+1 offsets; aad_off may be NULL (every row uses aad[0 .. aad_len)).  Seal writes row i = nonce | ct |
// tag at pt_off[i] + 28 i; Open reads rows by sealed_off, writes plaintext i at sealed_off[i] - 28 i
// (zeros where the tag does not match) and status[i] = 0 / -1.
enum class AeadAlg { AES_256_GCM, CHACHA20_POLY1305 };
hipError_t aead_seal(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* nonces, const uint8_t* pt,
                     const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                     uint8_t* sealed, hipStream_t st);
hipError_t aead_open(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* sealed, const uint64_t* sealed_off,
                     const uint8_t* aad, const uint64_t* aad_off, size_t aad_len, uint8_t* pt, int32_t* status,
                     hipStream_t st);
// tests only: Poly1305 (key32 = r | s, any message length) and GHASH (whole blocks) on chosen inputs
hipError_t dbg_poly1305(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, uint8_t* tag,
                        hipStream_t st);
hipError_t dbg_ghash(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, uint8_t* out,
                     hipStream_t st);

// AEAD with one row spread over many workgroups (aead_long.hip): the contracts of aead_seal / aead_open, rows of
// at most max_len plaintext bytes (0 < max_len < 2^31; a longer row is refused like a row with a bad span).
// aead_long_layout: { segment bytes S, bytes per lane C, tail fan-in, scratch bytes per segment partial }.
// scratch: aead_long_scratch_bytes, of which the first aead_long_part_bytes hold the segment partials (secret-
// derived; zero again when the call's kernels have run, or wiped by the launcher if a launch failed) and the
// rest one verdict word per row.  The grid is aead_long_workgroups(n, max_len), which must be below 2^31.
void aead_long_layout(AeadAlg alg, size_t out[4]);
size_t aead_long_part_bytes(AeadAlg alg, size_t n, size_t max_len);
size_t aead_long_scratch_bytes(AeadAlg alg, size_t n, size_t max_len);
size_t aead_long_workgroups(size_t n, size_t max_len);
hipError_t aead_seal_long(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* nonces, const uint8_t* pt,
                          const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                          size_t max_len, uint8_t* sealed, void* scratch, hipStream_t st);
hipError_t aead_open_long(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* sealed, const uint64_t* sealed_off,
                          const uint8_t* aad, const uint64_t* aad_off, size_t aad_len, size_t max_len, uint8_t* pt,
                          int32_t* status, void* scratch, hipStream_t st);
// tests only: the same segment and tail machinery as a bare MAC under a chosen H ([n][16]) or key32 = r | s
// ([n][32]) over whole 16-byte blocks; scratch as the GCM / ChaCha20-Poly1305 call of the same n and max_len
hipError_t dbg_ghash_long(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, size_t max_len,
                          uint8_t* out, void* scratch, hipStream_t st);
hipError_t dbg_poly1305_long(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, size_t max_len,
                             uint8_t* tag, void* scratch, hipStream_t st);

// A signature launcher's parameter-set index as a compile-time constant: f(std::integral_constant<int, W>{}) for
// the W < N that equals `which`, hipErrorInvalidValue for any other value.
template <int N, class F>
inline hipError_t with_which(int which, F&& f) {
  if constexpr (N == 0) return hipErrorInvalidValue;
  else return which == N - 1 ? f(std::integral_constant<int, N - 1>{}) : with_which<N - 1>(which, f);
}

// Bytes per row of a signature parameter set; n: the hash-based family's n (seeds 3 n, opt_rand n), 0 for ML-DSA.
struct SigSizes {
  size_t pk, sk, sig, n;
};

// ML-DSA.Verify over n rows of one chunk (mldsa.hip; FIPS 204, pure ML-DSA).  which = mldsa_find(name):
// 0, 1, 2 for ML-DSA-44 / 65 / 87, -1 for any other name.  pk [n][pk], sig [n][sig], messages ragged
// (msg + n + 1 offsets), one context string of ctx_len <= 255 bytes for all rows (device pointer; not
// read when ctx_len = 0).  status[i] = 0 (valid) or -1, written for every row.  The trace pointers are
// all set or all NULL (tests): mu [n][64] and ctilde [n][64] 8-byte aligned, w1 [n][w1 bytes], flags [n];
// mldsa_trace_at gives the same trace `row` rows further on.
struct MldsaTrace {
  uint8_t* mu = nullptr;
  uint8_t* ctilde = nullptr;
  uint8_t* w1 = nullptr;
  uint32_t* flags = nullptr;
};
int mldsa_find(const char* name);
SigSizes mldsa_sizes(int which);
MldsaTrace mldsa_trace_at(int which, const MldsaTrace& t, size_t row);
size_t mldsa_scratch_bytes(int which, size_t chunk);
hipError_t mldsa_verify(int which, size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* msg_off,
                        const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len, int32_t* status,
                        const MldsaTrace& trace, void* scratch, hipStream_t st);

// ML-DSA.KeyGen and ML-DSA.Sign over n rows of one chunk (mldsa_sign.hip; FIPS 204 Algorithms 6 and 2 / 7); which
// as above.  xi [n][32]; rnd NULL (deterministic: 32 zero bytes) or [n][32]; messages and context as mldsa_verify.
// status[i] = 0, or -1 with an all-zero signature row (a row of 2^31 bytes or more, decreasing offsets, a secret
// key with an s1 / s2 field outside [-eta, eta], or max_iters iterations without an accepted signature);
// MLDSA_SIGN_MAX_ITERS in production.  trace_mu [n][64] and trace_iters [n] are both set or both NULL (tests).
// The scratch holds public values only (mldsa_sign_scratch_bytes: A_hat, mu, a flag word: k l KiB + 68 bytes per row).
constexpr uint32_t MLDSA_SIGN_MAX_ITERS = 814;  // FIPS 204 Appendix C: the least cap an implementation may set
size_t mldsa_sign_scratch_bytes(int which, size_t chunk);
hipError_t mldsa_keypair(int which, size_t n, const uint8_t* xi, uint8_t* pk, uint8_t* sk, void* scratch,
                         hipStream_t st);
hipError_t mldsa_sign(int which, size_t n, const uint8_t* sk, const uint8_t* msg, const uint64_t* msg_off,
                      const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len, uint8_t* sig, int32_t* status,
                      uint32_t max_iters, uint8_t* trace_mu, uint32_t* trace_iters, void* scratch, hipStream_t st);

// ML-DSA key sets (mldsa_keyed.hip): g keys expanded once into one device allocation of mldsa_keyset_bytes, and
// verification / signing of n rows that name their key by index.  MldsaKeys is the view of that allocation
// (mldsa_keyset_view; device pointers): A_hat [g][k][l][256] for both kinds; a public set adds (t1 2^d)_hat
// [g][k][256] reduced to [0, q) and tr [g][64]; a secret set adds NTT(s1) [g][l][256], NTT(s2) and NTT(t0)
// [g][k][256], head [g][128] = rho | K | tr as in the secret key, and a refusal word per key (nonzero: an
// s1 / s2 field outside [-eta, eta]).  Of these K and the three NTT'd vectors are secret.
// key_index [n] (device; NULL: every row uses key 0) is checked against g on the device before any address is
// formed from it: a row with an index >= g is refused (verification: status -1 and the flag word FLAG_KEY = 16;
// signing: status -1 and an all-zero signature).  Everything else as mldsa_verify / mldsa_sign.  The scratch
// holds public values only: mu, w1, c and a flag word per verified row, mu and a flag word per signed row.
struct MldsaKeys {
  uint32_t g = 0;
  const int32_t* A = nullptr;
  const int32_t* t1h = nullptr;
  const int32_t *s1h = nullptr, *s2h = nullptr, *t0h = nullptr;
  const uint8_t* head = nullptr;  // public: tr, 64 bytes per key; secret: rho | K | tr, 128 bytes per key
  const uint32_t* bad = nullptr;
};
// Which form of the signing core a key-set launch takes: 1 copies the NTT'd secret vectors into LDS once per
// workgroup, 2 reads them from the set in every iteration.  Same results; tools/mldsa_keyed_bench.py measures both
// through qrk_dbg_mldsa_keyed_sign_mode, read (relaxed) at launch.  Measured equal within the run's spread at 2^14
// rows, so the default is the form that is marginally ahead for a single signature ("ML-DSA key sets").
constexpr int MLDSA_KEYED_SIGN_DEFAULT = 1;
extern std::atomic<int> g_mldsa_keyed_sign_mode;
size_t mldsa_keyset_bytes(int which, bool secret, size_t g);
MldsaKeys mldsa_keyset_view(int which, bool secret, size_t g, void* mem);
// keys: pk [g][pk] or sk [g][sk]; mem: mldsa_keyset_bytes, every byte of it is written
hipError_t mldsa_keyset_expand(int which, bool secret, size_t g, const uint8_t* keys, void* mem, hipStream_t st);
size_t mldsa_keyed_scratch_bytes(int which, size_t chunk);
size_t mldsa_keyed_sign_scratch_bytes(int which, size_t chunk);
hipError_t mldsa_verify_keyed(int which, const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* msg,
                              const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                              int32_t* status, const MldsaTrace& trace, void* scratch, hipStream_t st);
hipError_t mldsa_sign_keyed(int which, const MldsaKeys& ks, size_t n, const uint32_t* key_index, const uint8_t* msg,
                            const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len,
                            uint8_t* sig, int32_t* status, uint32_t max_iters, uint8_t* trace_mu,
                            uint32_t* trace_iters, void* scratch, hipStream_t st);

// SLH-DSA-SHA2 / SPHINCS+-SHA2-simple "f" verification over n rows of one chunk (slhdsa.hip).  which =
// slhdsa_find(name): 2 set + flavour (set 0, 1, 2 = 128f, 192f, 256f; flavour 0 = "SPHINCS+-SHA2-*f-simple",
// round 3.1; 1 = "SLH-DSA-SHA2-*f", FIPS 205), -1 for any other name.  Arguments as mldsa_verify; a context
// string exists only in the FIPS 205 flavour.  The trace pointers are all set or all NULL (tests):
// digest [n][m], fors_pk [n][n], roots [n][d][n], flags [n]; slhdsa_trace_at as mldsa_trace_at.
struct SlhdsaTrace {
  uint8_t* digest = nullptr;
  uint8_t* fors_pk = nullptr;
  uint8_t* roots = nullptr;
  uint32_t* flags = nullptr;
};
int slhdsa_find(const char* name);
bool slhdsa_is_fips(int which);
SigSizes slhdsa_sizes(int which);
SlhdsaTrace slhdsa_trace_at(int which, const SlhdsaTrace& t, size_t row);
size_t slhdsa_scratch_bytes(int which, size_t chunk);
hipError_t slhdsa_verify(int which, size_t n, const uint8_t* pk, const uint8_t* msg, const uint64_t* msg_off,
                         const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len, int32_t* status,
                         const SlhdsaTrace& trace, void* scratch, hipStream_t st);

// SLH-DSA-SHA2 / SPHINCS+-SHA2-simple "f" key generation and signing over n <= SLHDSA_SIGN_MAX_ROWS rows of one
// chunk (slhdsa_sign.hip); which as above.  seeds [n][3 n_bytes] = SK.seed || SK.prf || PK.seed; opt_rand NULL
// (deterministic: PK.seed) or [n][n_bytes]; status[i] = 0, or -1 with an all-zero signature row (a row of
// 2^31 bytes or more, decreasing offsets, or a key whose PK.root is not the root of its SK.seed).  The scratch
// holds public values only (slhdsa_sign_scratch_bytes: 0.9 to 1.8 KB per row).
constexpr size_t SLHDSA_SIGN_MAX_ROWS = (size_t)1 << 16;  // rows are grid.x of (rows, trees) launches
size_t slhdsa_sign_scratch_bytes(int which, size_t chunk);
hipError_t slhdsa_keypair(int which, size_t n, const uint8_t* seeds, uint8_t* pk, uint8_t* sk, void* scratch,
                          hipStream_t st);
hipError_t slhdsa_sign(int which, size_t n, const uint8_t* sk, const uint8_t* msg, const uint64_t* msg_off,
                       const uint8_t* opt_rand, const uint8_t* ctx_str, size_t ctx_len, uint8_t* sig, int32_t* status,
                       void* scratch, hipStream_t st);

// Standard base64 (RFC 4648, '=' padding) of n records of L bytes -> [n][4 ceil(L/3)] chars,
// and strict decoding back (status[i] = -1 for a malformed record; caller zeroes status).
hipError_t base64_encode(size_t n, const uint8_t* in, size_t L, uint8_t* out, hipStream_t st);
hipError_t base64_decode(size_t n, const uint8_t* in, size_t L, uint8_t* out, int32_t* status, hipStream_t st);

}  // namespace qrk
