// The library's test hooks: every exported qrk_dbg_* function (include/qrkem.h declares none).  Not part of the
// public ABI: tests and tools call them through ctypes, and qrkem/_debug.py holds their one binding table, which
// tests/test_debug_abi.py checks against this file parameter by parameter.  The abi_*.cpp files, mlkem.hip and
// hqc.hip include it, so a definition that drifts from its declaration does not compile.  Keep the declarations
// plain: pointers, size_t, int and uint32_t parameters, an int result (0, or -1 with qrk_last_error() set).
#pragma once
#include "../../include/qrkem.h"

#ifdef __cplusplus
extern "C" {
#endif

// -DQRK_HOST_TRACE=1 builds only (abi_kem.cpp): the steady-clock stamps, in ns, at the phases of the last
// single-shot call, out[16] (tools/host_trace.py).
#if QRK_HOST_TRACE
int qrk_dbg_host_trace(long long* out);
#endif

// -DQRK_SS_TRACE=1 builds only (mlkem_one.cuh): the 100 MHz wall-clock phase marks of the last ML-KEM
// single-shot kernel, g_ss_trace of mlkem_trace.cuh copied out whole (tools/single_shot_trace.py).
#if QRK_SS_TRACE
int qrk_dbg_ss_trace(unsigned long long* out);
#endif

// -DQRK_HQC_TRACE=1 builds only (hqc.hip): the phase marks workgroup QRK_HQC_TRACE_WG of k_hqc_enc_mul /
// k_hqc_decode stamped, g_hqc_trace copied out whole (tools/hqc_trace.py).
#if QRK_HQC_TRACE
int qrk_dbg_hqc_trace(unsigned long long* out);
#endif

// The workgroup of role `role` of the pipelined single-shot ML-KEM KeyGen (PRF item N = role < 2K,
// row r = role - 2K + 1) publishes its payload and flags 150 ms late, past every bounded wait
// (-1: off).  Process-wide.
int qrk_dbg_kg_late(int role);

// Every ABI call (every chunk of a chunked one) fails as if its first launch had been rejected
// (0: off): launch_begin() records hipErrorLaunchFailure.  The kernels themselves still launch, on
// valid buffers, except where a launcher stops at the first failure.  Process-wide.
int qrk_dbg_fail_launch(int on);

// Writes `byte` (0..255) over the full current size of every buffer qrk_ctx_cleanse zeroes: the scratch,
// the handshake scratch, dio, dstage, the ML-KEM kept region (which is invalid from then on: no later Decaps
// reads the fill) and the pinned hio / hstage (one list, walked by both).  Synchronous,
// after the previous call's device work.  What a call relies on from one call to the next is left alone:
// the ML-KEM counter words, the single-shot flag, preloaded key sets, and the record of which region the
// last long AEAD call used.  The next call then finds, in every word it does not write itself, a value no
// earlier call of the same shape would have left there (tests/test_gpu_ctx_fill.py).
int qrk_dbg_ctx_fill(qrk_ctx* ctx, int byte);

// Batched ML-KEM Encaps / Decaps chunks of at most 2^15 handshakes fail right after the SampleNTT
// fix-up counter parity flip, before their first launch (0: off), and the context's two fix-up
// counter words and its parity read back (the re-zero path).
int qrk_dbg_fail_after_flip(int on);
int qrk_dbg_fixc_words(qrk_ctx* ctx, uint32_t* out, int* parity);

// Nonzero words among the context's single-shot KeyGen flag / counter words, which must be zero
// between calls (after a failed pipelined KeyGen too).
int qrk_dbg_kg_flags_residue(qrk_ctx* ctx, uint64_t* out);

// Nonzero bytes left in the ML-KEM per-handshake records of a chunk of n handshakes (mlkem_cleanse
// wipes them after every chunk).
int qrk_dbg_mlkem_records_residue(qrk_ctx* ctx, const char* alg, size_t n, uint64_t* out);

// Poly1305 and GHASH on chosen keys.  Through the AEADs r, s and H are cipher outputs and cannot be
// steered to their edge cases (r = 1 with an accumulator of exactly p + k, single-bit and all-ones H).
// Device pointers; tag_i = Poly1305(key32_i = r | s, msg_i), msg ragged by msg_off [n+1];
// out_i = GHASH_{h_i}(data_i), data_i a whole number of 16-byte blocks.
int qrk_dbg_poly1305_batch(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, uint8_t* tag,
                           void* stream);
int qrk_dbg_ghash_batch(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, uint8_t* out,
                        void* stream);

// The handshake driver's key compare (k_keys_equal) on chosen rows: agree_i = 1 iff a_i == b_i, a and b
// [n][len] device bytes, len 1..8160 as the driver's key_len, agree [n].  Through qrk_handshake_batch both
// keys come out of the same KEM and HKDF, so honest handshakes never disagree and the word bench.py counts
// as key_disagreements cannot be made 0 there: a compare that ignored a byte, or strode rows wrongly, shows
// only on inputs that differ in one chosen bit.
int qrk_dbg_keys_equal(size_t n, const uint8_t* a, const uint8_t* b, size_t len, int32_t* agree, void* stream);

// The segment and tail kernels' MAC machinery of the long AEAD calls as a bare MAC under a caller-chosen
// H (h [n][16]) or Poly1305 key32 = r | s ([n][32]), as qrk_dbg_ghash_batch / qrk_dbg_poly1305_batch above:
// device pointers, rows ragged by n + 1 offsets, whole 16-byte blocks (a trailing
// partial block is ignored), rows above max_len left unwritten; out / tag [n][16].  Through the AEADs
// H, r and s are cipher outputs and cannot be steered to their edge cases, and the block counts at which
// a wrong power of the multiplier would show cannot be met with a chosen multiplier.
// qrk_dbg_aead_long_residue: out[0] = the OR of every byte of the segment-partial region the context's
// last long call (or hook) used; 0 after any completed call.
int qrk_dbg_ghash_long_batch(qrk_ctx* ctx, size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off,
                             size_t max_len, uint8_t* out, void* stream);
int qrk_dbg_poly1305_long_batch(qrk_ctx* ctx, size_t n, const uint8_t* key32, const uint8_t* msg,
                                const uint64_t* msg_off, size_t max_len, uint8_t* tag, void* stream);
int qrk_dbg_aead_long_residue(qrk_ctx* ctx, uint64_t* out);

// qrk_mldsa_sign_batch with the loop's cap as an argument, which also writes, per row, mu [n][64] (zeros
// for a row refused for its offsets or length) and the iterations run, iters [n] (0 for a refused row,
// max_iters for one that exhausted them).  The production kernel stores them itself, in an instantiation
// no other call launches; this is what pins the rejection loop against tests/mldsa_spec.py iteration by
// iteration, and what lets a test reach the cap.
int qrk_dbg_mldsa_sign_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* msg,
                             const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len,
                             uint8_t* sig, int32_t* status, uint32_t max_iters, uint8_t* mu, uint32_t* iters,
                             void* stream);

// qrk_sig_verify_batch that also writes, per row, mu [n][64], the recomputed c~' [n][64] (lambda / 4
// bytes, then zeros), the w1Encode bytes [n][k 32 (6 or 4)] and a flag word (bit 0: hint encoding
// malformed, bit 1: ||z||_inf >= gamma1 - beta, bit 2: c~ != c~'; bit 3, internal: a row of 2^31 bytes
// or more).  A row with bit 0 or bit 3 set has zeros in the other three.  This is what makes parity with
// tests/mldsa_spec.py byte-level instead of one boolean per row.
int qrk_dbg_mldsa_verify_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* pk, const uint8_t* msg,
                               const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                               int32_t* status, uint8_t* mu, uint8_t* ctilde, uint8_t* w1, uint32_t* flags,
                               void* stream);

// qrk_mldsa_verify_keyed_batch with the trace outputs of qrk_dbg_mldsa_verify_trace; the flag word has one
// more bit, 16: the row's key index is outside the set (zeros in the other three outputs).
int qrk_dbg_mldsa_verify_keyed_trace(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                     const uint8_t* msg, const uint64_t* msg_off, const uint8_t* sig,
                                     const uint8_t* ctx_str, size_t ctx_len, int32_t* status, uint8_t* mu,
                                     uint8_t* ctilde, uint8_t* w1, uint32_t* flags, void* stream);

// qrk_mldsa_sign_keyed_batch with the loop's cap as an argument and the outputs of qrk_dbg_mldsa_sign_trace:
// mu [n][64] (zeros for a refused row) and the iterations run, iters [n].
int qrk_dbg_mldsa_sign_keyed_trace(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                   const uint8_t* msg, const uint64_t* msg_off, const uint8_t* rnd,
                                   const uint8_t* ctx_str, size_t ctx_len, uint8_t* sig, int32_t* status,
                                   uint32_t max_iters, uint8_t* mu, uint32_t* iters, void* stream);

// Tests and tools: which form of the keyed signing core later launches take (1: the NTT'd secret vectors
// held in LDS, 2: read from the set; anything else: the default).  Returns the mode now set.
int qrk_dbg_mldsa_keyed_sign_mode(int mode);

// qrk_sig_verify_batch for an SLH-DSA / SPHINCS+ name that also writes, per row, the H_msg digest [n][m],
// the FORS public key [n][n], the root every hypertree layer reconstructed [n][d][n] and a flag word
// (bit 0: the top root differs from PK.root; bit 1, internal: a row of 2^31 bytes or more, whose other
// three outputs are zeros).  The production kernel stores them itself, in an instantiation no other call
// launches; parity with tests/slhdsa_spec.py is byte-level per layer.
int qrk_dbg_slhdsa_verify_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* pk, const uint8_t* msg,
                                const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                                int32_t* status, uint8_t* digest, uint8_t* fors_pk, uint8_t* roots, uint32_t* flags,
                                void* stream);

// qrk_kem_decaps_batch for a FrodoKEM parameter set that also writes, per row, mu' = Decode(C - B'S) to
// mu_out [n][32] (len_mu = 16 / 24 / 32 bytes, then zeros).  The launches are those of the public call;
// mu' is read from the scratch record k_fr_dec_m wrote (seeds[12..]) before each chunk's cleanse.  On a
// ciphertext that fails the re-encryption check ss = H(ct || s) whatever Decode returned, so this is the
// only place a wrong mu' on such a row shows.
int qrk_dbg_frodo_decaps_trace(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ss, const uint8_t* ct,
                               const uint8_t* sk, uint8_t* mu_out, void* stream);

// The FrodoKEM sampler alone, on a stream of the caller's choice instead of SHAKE(0x96 / 0x5F || seedSE): n rows
// of raw 16-bit words in the specification's order, (2 N + 8) 8 per row for Encaps (kg = 0) and 2 N 8 for KeyGen
// (kg != 0), are laid out as the stream kernels write them and sampled by k_fr_sample<N, KG>, the launch of the
// public calls, on the context's scratch; its regions are copied out whole.  Encaps: s8 = S' int8 [n][8][NP]
// (NP = N rounded up to 128: the zeroed pad columns are part of the output), e16 = E' int16 [n][8][N],
// epp16 = E'' int16 [n][64].  KeyGen: s8 = S^T int8 [n][8][NP], e16 = E int16 [n][N][8], epp16 unused (may be
// NULL).  Device pointers; n at most the context chunk (one chunk, no chunking).  Through the public calls the
// words are hash output, which meets a given table boundary about once in 2^15 words and the top entries hardly ever.
int qrk_dbg_frodo_sample(qrk_ctx* ctx, const char* alg, int kg, size_t n, const uint16_t* words, int8_t* s8,
                         int16_t* e16, int16_t* epp16, void* stream);

// Everything after the sampler, on sample matrices of the caller's choice in the layout above (pad columns zero).
// Encaps (kg = 0): in = pk [n][pk bytes], mu [n][len_mu]; Gen(A) fused with S'A (SHAKE or AES as the name says) and
// k_fr_pack in its Encaps mode write out = ct [n][ct bytes]; sk unused.  KeyGen (kg != 0): in = seedA [n][16];
// k_fr_kg_spairs where the variant uses it, the A S + E kernel and k_fr_kg_pack write out = seedA || Pack(B)
// [n][pk bytes] and, into sk [n][sk bytes], the pk copy and S^T as int16 (s and pkh, other kernels' work, are left
// as the caller had them); epp16 and mu unused.  The launches are those of the public calls.  Every sample must
// lie in the parameter set's sampler range, |v| <= 12 / 10 / 6 for 640 / 976 / 1344, which is what the kernels'
// accumulator bounds assume: the hook reads the matrices back first and returns -1 without launching otherwise.
// Device pointers; n at most the context chunk.  Hash-derived samples have magnitude 2-3 and never fill a tile.
int qrk_dbg_frodo_from_samples(qrk_ctx* ctx, const char* alg, int kg, size_t n, const int8_t* s8, const int16_t* e16,
                               const int16_t* epp16, const uint8_t* in, const uint8_t* mu, uint8_t* out, uint8_t* sk,
                               void* stream);

// qrk_hqc_code_decode (same contract, same limit on n) that also
// returns the word the decoder is given.  t_out [n][n1 n2 / 8]: the n1 n2 bits of v - u y exactly as
// the kernel hands them to the Reed-Muller stage, little-endian bytes as in the ciphertext's v.  The
// sparse-dense product u y is otherwise visible only through a decoder that absorbs dozens of wrong
// bits per block; stored by the production kernel's own code under a compile-time switch that is off
// in every other call.
int qrk_dbg_hqc_decaps_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* ct,
                             uint8_t* t_out, uint8_t* syms, uint8_t* mprime, void* stream);

#ifdef __cplusplus
}
#endif
