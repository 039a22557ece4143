// ML-KEM-512/768/1024 (FIPS 203) batched KeyGen / Encaps / Decaps for gfx950.
//
// Replaces, for N handshakes at once, the liboqs calls the reference makes one
// at a time: OQS_KEM_keypair / OQS_KEM_encaps / OQS_KEM_decaps
// (quantum_resistant_p2p/vendor/oqs.py:318, :348, :372), reached from
// MLKEMKeyExchange.generate_keypair / encapsulate / decapsulate
// (quantum_resistant_p2p/crypto/key_exchange.py:125-186).
//
// Decomposition (DESIGN.md "Kernels"): every handshake is split into
// independent Keccak instances, each run by one lane, and polynomial stages,
// each run by a 16-lane group per handshake.
//
//   front / J / G  lane / handshake   H(ek), G(.), J(z||c)            (SHA3 / SHAKE256)
//   PRFs           lane / (nonce, hs)  PRF_eta(seed, N) raw bytes     (SHAKE256)
//   SampleNTT      lane / (x, y, hs)   3 SHAKE128 blocks, compacted to 12-bit chunks in the
//                                      producer; the ~0.7 % of entries that need a 4th block
//                                      go on a fix-up list (lane or wave per entry)
//   keygen / encrypt / decrypt cores
//                  16 lanes / hs       CBD, NTT, basemul, invNTT, compress/encode,
//                                      FO re-encrypt compare + implicit rejection
//
// Independent stages of one operation share multi-role launches (k_multi, roles in grid order,
// every kernel on the caller's stream); n <= 1024 runs one-launch kernels with wave-cooperative
// sponges instead (the reference's one-call-per-handshake pattern).  Keccak output goes to device
// scratch in a 64-instance tiled SoA layout (word w of instance i at ((i/64)*W + w)*64 + i%64):
// every lane-per-instance store is a fully coalesced 512-byte wave store.
//
// Where the code is.  This file: the entry points qrkem_internal.h declares, i.e. the sizes, the
// cleanse and the dispatch between the execution paths.  One file per path, each with its kernels
// and plain host launchers (mlkem_paths.h), included below:
//   mlkem_batch.cuh   n > 1024: k_front_keygen, k_back_keygen, k_rho_copy, k_rho_match, k_keygen_core, the roles
//                     (RXof, RXofFixCoop, RFrontEnc[Pair], RJDec, RGDec[Pair], RPrf, RDecrypt, RCore)
//                     with k_multi / k_role, rho_source, and the per-context state (mlkem::CtxState)
//   mlkem_one.cuh     n <= 1024: k_encaps_one, k_decaps_one, k_keygen_one; qrk_dbg_ss_trace
//   mlkem_kg.cuh      KeyGen, n <= 16: k_keygen_multi, k_keygen_pipe (sc1 hand-offs, bounded waits)
// The three are one translation unit on purpose.  Every device function is inlined, but the compiler
// specialises a helper on what all its callers in the unit pass it (pack_bits, flush_bits, xof_coop
// and their like are shared between paths), so compiling the paths apart changes the code of the
// one-launch kernels and of k_keygen_multi (tools/kernel_hashes.py shows it: nine kernels, the
// batched ones untouched).  A tool that needs one path includes that file alone.
// The headers they share:
//   mlkem_layout.cuh  XOF_W / PRF_W, tidx, XUnit / XChunk, P<K>, ScratchView / scratch_words / carve
//   mlkem_sample.cuh  lane-per-instance SampleNTT (compact_block, xof_*) and prf_inst
//   mlkem_poly.cuh    16-lane group polynomial I/O (GroupLds, load / pack / flush, encode / decode 12)
//                     and the K-PKE.Decrypt core
//   mlkem_coop.cuh    wave-cooperative SampleNTT and PRF (xof_coop*, prf_coop)
//   mlkem_trace.cuh   the QRK_SS_TRACE phase marks
//   mlkem_arith.cuh   tables, fp32 modular arithmetic, NTTs, basemul
#include "mlkem_layout.cuh"
#include "mlkem_paths.h"
#include "qrkem_debug.h"  // qrk_dbg_ss_trace (mlkem_one.cuh)

#include "mlkem_batch.cuh"
#include "mlkem_one.cuh"
#include "mlkem_kg.cuh"

namespace qrk {

size_t mlkem_scratch_bytes(const AlgInfo& a, size_t chunk) {
  // the multi-workgroup KeyGen (n <= QRK_KG_MULTI_MAX) keeps one MkScr (16 KiB) per handshake in
  // the scratch; every other path needs scratch_words (about 5.1 KB per ML-KEM-768 handshake)
  const size_t C = round64(chunk);
  return std::max(mlkem::scratch_words(a.k, C) * 8, mlkem::keygen_scratch_bytes(C));
}
size_t mlkem_matrix_bytes(const AlgInfo& a, size_t chunk) {
  return (size_t)a.k * a.k * round64(chunk) * mlkem::XOF_W * sizeof(uint64_t);
}

size_t mlkem_keep_cap_bytes() {
  const char* v = std::getenv("QRK_KEEP_MIB");
  return (size_t)((v && *v) ? std::strtoull(v, nullptr, 10) : 8192) << 20;
}

void mlkem_records_span(const AlgInfo& a, size_t C, size_t* off, size_t* bytes) {
  // mlkem::carve: the sampled matrix, the PRF words, then seeds | m' | K' | Kbar (4 C words each)
  const size_t K = (size_t)a.k;
  *off = (K * K * C * mlkem::XOF_W + (2 * K + 1) * C * mlkem::PRF_W) * sizeof(uint64_t);
  *bytes = 16 * C * sizeof(uint64_t);
}

hipError_t mlkem_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st) {
  // the one-launch kernels (n <= QRK_SMALL_MAX) keep their key material in LDS and wipe it
  if (n == 0 || n <= mlkem_small_max()) return hipSuccess;
  const size_t C = round64(n);
  const mlkem::ScratchView v = mlkem::carve(scratch, a.k, C);
  return hipMemsetAsync(v.seeds, 0, 16 * C * sizeof(uint64_t), st);  // seeds | mprime | kprime | kbar
}

// The dispatch between the paths (each launcher switches on a.k in its own file)
hipError_t mlkem_keypair(const AlgInfo& a, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                         const Streams& s) {
  if (n == 0) return hipSuccess;
  if (mlkem::keygen_pipe_built() && n <= mlkem_kg_multi_max() && s.kg_cnt && s.kg_err)  // host-pointer calls
    return mlkem::keygen_pipe(a.k, n, pk, sk, coins, scratch, s);
  if (n <= mlkem_kg_multi_max() && s.kg_cnt)  // device-pointer calls (no error word), QRK_KG_PIPE=0 builds
    return mlkem::keygen_multi(a.k, n, pk, sk, coins, scratch, s);
  if (n <= mlkem_small_max()) return mlkem::keygen_one(a.k, n, pk, sk, coins, s);
  return mlkem::keygen_batched(a.k, n, pk, sk, coins, scratch, s);
}

hipError_t mlkem_encaps(const AlgInfo& a, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk,
                        const uint8_t* coins, int32_t* status, void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  if (n <= mlkem_small_max()) return mlkem::encaps_one(a.k, n, ct, ss, pk, coins, status, s);
  return mlkem::encaps_batched(a.k, n, ct, ss, pk, coins, status, scratch, s);
}

hipError_t mlkem_decaps(const AlgInfo& a, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, int32_t*,
                        void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  if (n <= mlkem_small_max()) return mlkem::decaps_one(a.k, n, ss, ct, sk, s);
  return mlkem::decaps_batched(a.k, n, ss, ct, sk, scratch, s);
}

}  // namespace qrk
