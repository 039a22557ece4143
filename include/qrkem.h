/* qrkem -- MI355X-native batched post-quantum KEM engine: public C ABI.
 *
 * Built as quantum-resistant-p2p_amd/qrkem/libqrkem.so (hipcc, gfx950).
 *
 * Part 1 is the liboqs-compatible subset that the reference's vendored ctypes
 * wrapper binds (quantum_resistant_p2p/vendor/oqs.py).  A maintainer can drop
 * libqrkem.so in place of vendor/lib/linux/liboqs.so and the reference's own
 * oqs.py loads it unchanged.  Part 2 adds the batched,
 * stream-ordered, device-pointer entry points the reference has no equivalent
 * for (it calls liboqs once per handshake on the asyncio thread).
 *
 * Ownership: callers allocate every output buffer (as oqs.py:316-317, 342-347,
 * 369-371 do); the library owns only OQS_KEM handles, static strings and the
 * device scratch inside a qrk_ctx.  Errors: OQS_SUCCESS (0) / OQS_ERROR (-1),
 * as oqs.py:38-39; qrk_last_error() gives a message.
 */
#ifndef QRKEM_H
#define QRKEM_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ *
 * Part 1: liboqs-compatible subset                                    *
 * ------------------------------------------------------------------ */

typedef enum { OQS_ERROR = -1, OQS_SUCCESS = 0 } OQS_STATUS;

/* Struct prefix read by oqs.py:241-253 (liboqs <= 0.12 layout): the wrapper
 * reads method_name .. length_shared_secret and treats the three callbacks as
 * opaque pointers. */
typedef struct OQS_KEM {
  const char *method_name;
  const char *alg_version;
  uint8_t claimed_nist_level;
  bool ind_cca;
  size_t length_public_key;
  size_t length_secret_key;
  size_t length_ciphertext;
  size_t length_shared_secret;
  OQS_STATUS (*keypair)(uint8_t *public_key, uint8_t *secret_key);
  OQS_STATUS (*encaps)(uint8_t *ciphertext, uint8_t *shared_secret, const uint8_t *public_key);
  OQS_STATUS (*decaps)(uint8_t *shared_secret, const uint8_t *ciphertext, const uint8_t *secret_key);
} OQS_KEM;

/* oqs.py:192 */
void OQS_init(void);
/* oqs.py:197-198 */
const char *OQS_version(void);
/* oqs.py:409 */
size_t OQS_KEM_alg_count(void);
/* oqs.py:397, 409 */
const char *OQS_KEM_alg_identifier(size_t i);
/* oqs.py:406 */
int OQS_KEM_alg_is_enabled(const char *method_name);
/* oqs.py:271, 396 -- NULL for unknown or not-enabled names */
OQS_KEM *OQS_KEM_new(const char *method_name);
/* oqs.py:318-322: host pointers, one handshake, randomness from the OS CSPRNG */
OQS_STATUS OQS_KEM_keypair(const OQS_KEM *kem, uint8_t *public_key, uint8_t *secret_key);
/* oqs.py:348-353 */
OQS_STATUS OQS_KEM_encaps(const OQS_KEM *kem, uint8_t *ciphertext, uint8_t *shared_secret,
                          const uint8_t *public_key);
/* oqs.py:372-377 */
OQS_STATUS OQS_KEM_decaps(const OQS_KEM *kem, uint8_t *shared_secret, const uint8_t *ciphertext,
                          const uint8_t *secret_key);
/* oqs.py:390 */
void OQS_KEM_free(OQS_KEM *kem);
/* oqs.py:386-389 */
void OQS_MEM_cleanse(void *ptr, size_t len);

/* Derandomised single-shot forms (names of liboqs >= 0.13's *_derand API):
 * KeyGen coins = d||z (ML-KEM, 64 B) or s||seedSE||z (FrodoKEM); Encaps coins
 * = m (32 B) or mu.  Host pointers. */
OQS_STATUS OQS_KEM_keypair_derand(const OQS_KEM *kem, uint8_t *public_key, uint8_t *secret_key,
                                  const uint8_t *seed);
OQS_STATUS OQS_KEM_encaps_derand(const OQS_KEM *kem, uint8_t *ciphertext, uint8_t *shared_secret,
                                 const uint8_t *public_key, const uint8_t *seed);

/* Signature half of the liboqs ABI: the reference's oqs.py binds these at
 * import time (oqs.py:684-697).  Neither signature family has a single-shot
 * path here, and a registry that listed names whose calls fail would be a
 * trap.  So the registry stays empty (count 0) and every call here fails.
 * The batched calls of Part 2 verify for both families
 * (qrk_sig_verify_batch) and generate keys and sign: for the hash-based one
 * qrk_sig_keypair_batch / qrk_sig_sign_batch, for ML-DSA
 * qrk_mldsa_keypair_batch / qrk_mldsa_sign_batch. */
typedef struct OQS_SIG OQS_SIG;
size_t OQS_SIG_alg_count(void);
const char *OQS_SIG_alg_identifier(size_t i);
int OQS_SIG_alg_is_enabled(const char *method_name);
OQS_SIG *OQS_SIG_new(const char *method_name);
OQS_STATUS OQS_SIG_keypair(const OQS_SIG *sig, uint8_t *public_key, uint8_t *secret_key);
OQS_STATUS OQS_SIG_sign(const OQS_SIG *sig, uint8_t *signature, size_t *signature_len, const uint8_t *message,
                        size_t message_len, const uint8_t *secret_key);
OQS_STATUS OQS_SIG_verify(const OQS_SIG *sig, const uint8_t *message, size_t message_len,
                          const uint8_t *signature, size_t signature_len, const uint8_t *public_key);
void OQS_SIG_free(OQS_SIG *sig);

/* ------------------------------------------------------------------ *
 * Part 2: batched device API (no reference equivalent)                *
 * ------------------------------------------------------------------ */

typedef struct qrk_ctx qrk_ctx;

/* One context per (process, device).  Holds device scratch, grown on demand. */
int qrk_ctx_create(qrk_ctx **out, int device);
void qrk_ctx_destroy(qrk_ctx *ctx);
/* Handshakes per internal chunk (scratch = chunk * per-handshake bytes). */
int qrk_ctx_set_chunk(qrk_ctx *ctx, size_t chunk);
size_t qrk_ctx_scratch_bytes(const qrk_ctx *ctx);
/* Zero every buffer of the context that can hold keys or secret intermediates (device
 * scratch, handshake scratch, device and pinned host staging); synchronous.  Every call
 * already zeroes the per-handshake key records it leaves in scratch (seeds, m', K', Kbar,
 * ...) and the staged copies of host secrets (coins included).  The other intermediates stay
 * in scratch until a later call overwrites them, and some of them are expanded secret-key
 * material: ML-KEM's PRF output for s and e (KeyGen) and for the re-encryption noise (Decaps),
 * FrodoKEM's sampled S / S', HQC's seedexpander rows x, y (KeyGen, Decaps) and r1, r2, e.
 * Call this (or qrk_ctx_destroy, which does the same before freeing) when a context that
 * handled secret keys is idle. */
int qrk_ctx_cleanse(qrk_ctx *ctx);
/* Diagnostics (tests): waits for the context's last call, then counts the nonzero bytes left
 * in its pinned host staging (out[0]) and device staging (out[1]) -- the buffers that carry
 * OS-drawn coins (coins == NULL) to the device, wiped before every call returns -- and in the
 * first 64 MiB of device scratch (out[2], zero after qrk_ctx_cleanse). */
int qrk_ctx_staging_residue(qrk_ctx *ctx, uint64_t out[3]);
/* Handshakes per chunk actually used for `alg` (FrodoKEM and HQC cap the chunk so their
 * scratch stays within QRK_SCRATCH_GIB = 48 GiB); 0 for an unknown algorithm. */
size_t qrk_ctx_effective_chunk(const qrk_ctx *ctx, const char *alg);
/* What a context keeps of a batched ML-KEM KeyGen for its own Decaps of the same keys: the sampled
 * matrix A_hat (K^2 384 bytes per handshake) and a 32-byte rho tag per handshake, of whole batched
 * chunks (more than 1024 rows) in order, as many as the cap allows.  For a KeyGen of n handshakes on a
 * context whose chunk is `chunk`: out[0] = rows per chunk, out[1] = batched chunks, out[2] = chunks
 * kept, out[3] = bytes kept.  cap_bytes = (size_t)-1: the cap in force, QRK_KEEP_MIB MiB from the
 * environment (read at every KeyGen; 0 keeps nothing), 8192 by default.  Pure arithmetic, no device.
 * Outputs never depend on what is kept, only time does. */
int qrk_mlkem_keep_plan(const char *alg, size_t n, size_t chunk, size_t cap_bytes, size_t out[4]);
/* Schedule of one operation's kernels, all on the caller's stream: 0 (default): independent
 * kernels share multi-role launches (each role's workgroups a contiguous range of one grid, in
 * grid order); 1: serial, one kernel per launch (kernel timings in isolation).  Any other value
 * returns -1 with qrk_last_error() set.  (Round 3's value 2, the forked split pipeline, was
 * removed in round 4 and is rejected now.) */
int qrk_ctx_set_streams(qrk_ctx *ctx, int streams);

/* Sizes of `alg`: out[0..5] = pk, sk, ct, ss, keypair coin bytes, encaps coin bytes. */
int qrk_kem_sizes(const char *alg, size_t out[6]);

/* Batched operations.  ALL buffers are device pointers, contiguous AoS
 * [n][len].  `coins` may be NULL (the library draws n*len bytes from the OS
 * CSPRNG and uploads them); otherwise it is [n][keypair/encaps coin bytes].
 * `status` (nullable, device int32[n]) receives -1 for encapsulation keys that
 * fail the FIPS 203 section 7.2 modulus check, else 0.  `stream` is a
 * hipStream_t (NULL = default stream).  Calls are stream-ordered and
 * asynchronous: every kernel of a call runs on `stream`, and with caller-supplied
 * coins (or none needed) a call returns to the host before its kernels finish.
 * With coins == NULL the call returns once the OS coins are uploaded (their pinned
 * copy is wiped then).  Re-entrant across contexts.  Calls on one context may use
 * different streams: each call's stream first waits, on the device, until the
 * previous call on that context is done with the context's scratch. */
int qrk_kem_keypair_batch(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *pk, uint8_t *sk,
                          const uint8_t *coins, void *stream);
int qrk_kem_encaps_batch(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *ct, uint8_t *ss,
                         const uint8_t *pk, const uint8_t *coins, int32_t *status, void *stream);
int qrk_kem_decaps_batch(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *ss, const uint8_t *ct,
                         const uint8_t *sk, void *stream);
/* Decaps with a per-record return code (device int32[n]): HQC writes -1 where the
 * re-encryption check fails -- the OQS_ERROR liboqs's HQC decaps returns, which makes the
 * reference's KeyEncapsulation.decap_secret raise (oqs.py:372-380); ss_i = K(sigma || ct_i)
 * is written either way.  ML-KEM and FrodoKEM (implicit rejection, return 0) write 0. */
int qrk_kem_decaps_batch_status(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *ss, const uint8_t *ct,
                                const uint8_t *sk, int32_t *status, void *stream);

/* Same, with host buffers (synchronous; copies through pinned staging). */
int qrk_kem_keypair_batch_host(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *pk, uint8_t *sk,
                               const uint8_t *coins);
int qrk_kem_encaps_batch_host(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *ct, uint8_t *ss,
                              const uint8_t *pk, const uint8_t *coins, int32_t *status);
int qrk_kem_decaps_batch_host(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *ss, const uint8_t *ct,
                              const uint8_t *sk);
int qrk_kem_decaps_batch_status_host(qrk_ctx *ctx, const char *alg, size_t n, uint8_t *ss, const uint8_t *ct,
                                     const uint8_t *sk, int32_t *status);

/* Bench inputs generated on device: out_i = SHAKE256("qrk-bench"||LE64(seed)||LE64(first+i), len),
 * len a multiple of 8, <= 136.  Device pointer. */
int qrk_bench_coins(qrk_ctx *ctx, size_t n, size_t len, uint64_t seed, uint64_t first, uint8_t *out,
                    void *stream);
/* Flip one ciphertext bit per selected index (mode 0 none, 1 all, 2 Bernoulli(1/2)):
 * h_i = SHAKE256("qrk-tamper"||LE64(seed)||LE64(i))[0..8), bit (h_i>>1) mod 8*ctlen. */
int qrk_tamper(qrk_ctx *ctx, size_t n, size_t ctlen, uint64_t seed, int mode, uint8_t *ct, void *stream);
/* Per-record digests: out_i = SHA3-256(a_i || b_i), 32 bytes, for n records of a_len and
 * b_len bytes (b may be NULL with b_len = 0).  Device pointers.  The sharded bench hashes
 * each rank's (ct, ss) records with it and combines them per block of global indices, so
 * the digests do not depend on the GPU count. */
int qrk_digest_rows(qrk_ctx *ctx, size_t n, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                    uint8_t *out, void *stream);
/* HQC fixed-weight supports (the sampling inside KeyGen / Encaps / Decaps, exposed so the
 * duplicate-removal step can be tested on inputs crafted to collide): for each of n vectors,
 * sup[v][i] = i + floor(r[v][i] * (n_HQC - i) / 2^32), then the spec's removal of duplicates.
 * kind 0: weight w (x, y), kind 1: weight w_r = w_e (r1, r2, e).  Device uint32 pointers,
 * [n][weight] each. */
int qrk_hqc_supports(qrk_ctx *ctx, const char *alg, int kind, size_t n, const uint32_t *r, uint32_t *sup,
                     void *stream);
/* HQC concatenated-code decoder alone (the first stages of Decaps, exposed so the decoder can be
 * tested on chosen inputs: with u = 0 in ct the decoded word is v itself): for each of n records,
 * syms[i] = the n1 Reed-Muller symbols decoded from v - u y, mprime[i] = the k message bytes the
 * Reed-Solomon decoder returns for them.  No re-encryption, no shared secret.  Device pointers:
 * sk [n][sk_len], ct [n][ct_len], syms [n][n1], mprime [n][k].  n must not exceed the context's
 * chunk for the algorithm (qrk_ctx_effective_chunk). */
int qrk_hqc_code_decode(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *sk, const uint8_t *ct,
                        uint8_t *syms, uint8_t *mprime, void *stream);
/* (Its traced twin, the test hook qrk_dbg_hqc_decaps_trace, is declared in csrc/qrkem_debug.h.) */

/* HKDF-SHA256 (RFC 5869) over n keys, one GPU lane per key.  Replaces
 * SecureMessaging._derive_symmetric_key (messaging.py:350-382: HKDF(SHA256,
 * length=key_size, salt=None, info=...).derive(shared_secret)).
 * Device pointers: ikm [n][ikm_len]; salt [salt_len] shared by all keys (NULL/0 =
 * HashLen zero bytes, as salt=None); okm [n][okm_len], 1 <= okm_len <= 8160.
 * info: with info_off (device uint64[n+1]) key i uses info[info_off[i] .. info_off[i+1]);
 * with info_off NULL every key uses info[0 .. info_len). */
int qrk_hkdf_sha256_batch(qrk_ctx *ctx, size_t n, const uint8_t *ikm, size_t ikm_len, const uint8_t *salt,
                          size_t salt_len, const uint8_t *info, const uint64_t *info_off, size_t info_len,
                          uint8_t *okm, size_t okm_len, void *stream);

/* n complete protocol key exchanges with the reference's per-handshake operation mix
 * (messaging.py:546-1146): initiator KeyGen (:590); responder KeyGen (:809, its pk is
 * sent back at :853), Encaps of the initiator's pk (:830) and HKDF (:845); initiator
 * Decaps (:1038) and HKDF (:1068).  Device pointers.  Coins (each nullable = OS CSPRNG):
 * coins_kp_i / coins_kp_r [n][keypair coin bytes], coins_enc [n][encaps coin bytes].
 * info / info_off / info_len as qrk_hkdf_sha256_batch (salt = None).  Outputs (the wire
 * and the keys): pk_i, pk_r [n][pk], ct [n][ct], key_i, key_r [n][key_len]; agree
 * (nullable, int32[n]) = 1 where both sides derived the same key.  Ephemeral secret keys
 * and shared secrets stay in context scratch and are zeroed before the call returns
 * (stream-ordered). */
int qrk_handshake_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *coins_kp_i,
                        const uint8_t *coins_kp_r, const uint8_t *coins_enc, const uint8_t *info,
                        const uint64_t *info_off, size_t info_len, size_t key_len, uint8_t *pk_i, uint8_t *pk_r,
                        uint8_t *ct, uint8_t *key_i, uint8_t *key_r, int32_t *agree, void *stream);

/* Authenticated encryption under n session keys, one GPU lane per message: what the reference does
 * with every derived key (SymmetricAlgorithm.encrypt / decrypt, crypto/symmetric.py:95-161, 193-259),
 * first for the key_exchange_test message that completes a handshake (messaging.py:1102-1114,
 * 1224-1250).  alg: "AES-256-GCM" (SP 800-38D, 96-bit IV, 128-bit tag) or "ChaCha20-Poly1305"
 * (RFC 8439), the reference's `name` strings; any other name returns -1.  Device pointers, of the
 * kinds qrk_hkdf_sha256_batch accepts: keys [n][32]; nonces [n][12], or NULL for n nonces from the OS
 * CSPRNG (the call then returns once they are uploaded, as with coins == NULL; never seal two messages
 * under one key with one nonce); messages are ragged: bytes plus device uint64[n+1] offsets; aad /
 * aad_off / aad_len as info / info_off / info_len of qrk_hkdf_sha256_batch (all NULL / 0: no
 * associated data).  Row lengths are 32-bit: aad_len >= 2^31 returns -1.
 *
 * Seal: row i of `sealed` = nonce || ciphertext || tag, exactly the bytes `encrypt` returns
 * (symmetric.py:116-119), at byte pt_off[i] + 28 i; `sealed` holds pt_off[n] + 28 n bytes.  A row whose
 * plaintext or aad span is 2^31 bytes or more is left unwritten.
 * Open: row i = sealed[sealed_off[i] .. sealed_off[i+1]); its plaintext goes to byte
 * sealed_off[i] - 28 i of `pt`, which holds sealed_off[n] - 28 bytes (sealed_off[n] - 28 n are used
 * when every row has its 28 bytes of overhead).  status (device int32[n], required): 0, or -1 for a row shorter than 28 bytes, of 2^31
 * bytes or more, or whose tag does not verify.  The tag is computed and compared (without early exit)
 * before any plaintext is written; where it does not match, zeros are written over that row's plaintext
 * span: no unauthenticated plaintext is released.  A row shorter than 28 bytes writes nothing; the
 * offset rule then places the following rows' plaintext up to 28 bytes early, over the tail of the
 * preceding one (a row whose place would start before `pt` gets status -1), so a caller that cannot
 * rule such rows out pads them to 28 bytes (they fail to verify).
 * Authentication failure is reported only in status; the calls return 0 / -1 as the rest of Part 2. */
int qrk_aead_seal_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *keys, const uint8_t *nonces,
                        const uint8_t *pt, const uint64_t *pt_off, const uint8_t *aad, const uint64_t *aad_off,
                        size_t aad_len, uint8_t *sealed, void *stream);
int qrk_aead_open_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *keys, const uint8_t *sealed,
                        const uint64_t *sealed_off, const uint8_t *aad, const uint64_t *aad_off, size_t aad_len,
                        uint8_t *pt, int32_t *status, void *stream);

/* The same two operations for long rows: one row is sealed or opened by many workgroups instead of one
 * lane (a file sent whole, messaging.py:1707-1713).  The bytes written are those of qrk_aead_seal_batch /
 * qrk_aead_open_batch, and so are the arguments, the row layout, NULL nonces, the o < 28 i rule of Open,
 * n == 0 and stream ordering.  max_len is the caller's bound on any row's plaintext length (it sizes the
 * grid and the scratch): 0, or 2^31 and more, returns -1; a row longer than max_len is treated like a row
 * with a bad aad span: Seal leaves it unwritten, Open gives it status -1 and writes nothing for it.
 * Argument checks, in order: ctx, alg, n == 0 (returns 0), NULL buffers, aad_len, max_len, then the grid
 * (n ceil(max_len / S) workgroups must stay below 2^31) and the scratch budget below; each failure
 * returns -1 with qrk_last_error() set before any device work.
 *
 * qrk_aead_long_layout (host only) gives out = { S, C, the tail's fan-in, scratch bytes per segment }:
 * a row is cut into segments of S = 256 C bytes, one 256-lane workgroup each, a lane owning C consecutive
 * bytes (S = 65536, C = 256).  Segments are counted from the END of the row, so a row's short segment is
 * its first one.  Each segment leaves a partial MAC (16 bytes of GHASH, or five Poly1305 limbs in 32
 * bytes) in the context's scratch and one 64-lane workgroup per row combines them as a tree over powers
 * of H^(S/16) / r^(S/16), finishes the tag and, on Open, compares it without early exit; a second pass
 * then decrypts the rows that verified and writes zeros over the plaintext span of those that did not, so
 * no plaintext byte of an unauthenticated row is ever written.  Associated data is absorbed serially (it
 * is a message id in the reference); keep it short.
 * Scratch: per row ceil(max_len / S) partials plus one 4-byte verdict word, i.e.
 * n (ceil(max_len / S) out[3] + 4) bytes; beyond the context's scratch budget (48 GiB unless the library
 * was built with another QRK_SCRATCH_GIB) the call returns -1.  The partials are secret-derived (H or r
 * can be solved from one of them and the public ciphertext): they exist only in that scratch, the
 * combining workgroup overwrites its row's whole partial span with zeros once it has consumed it (a
 * call whose launch failed wipes the span itself), and qrk_ctx_cleanse covers them like the rest of the
 * scratch.  No round key, H, r or s reaches global memory or a kernel argument.
 *
 * When to use which (measured on one MI355X, n = 1, tools/aead_long_bench.py, medians in ms; "-": the
 * one-lane call takes more than a second there and is not timed):
 *      bytes   GCM seal lane/long   GCM open lane/long   ChaCha seal lane/long   ChaCha open lane/long
 *      4 KiB      2.17 / 0.34          2.20 / 0.35           0.71 / 0.053            0.72 / 0.058
 *     16 KiB      8.95 / 0.34          9.20 / 0.34           2.80 / 0.051            2.81 / 0.056
 *     64 KiB      35.5 / 0.34          35.3 / 0.35           11.1 / 0.052            11.1 / 0.058
 *    256 KiB     137.6 / 0.34         138.0 / 0.35           43.9 / 0.053            44.1 / 0.059
 *      1 MiB     572.8 / 0.44         571.3 / 0.41          178.5 / 0.060           180.1 / 0.064
 *      4 MiB         - / 0.34             - / 0.35          702.2 / 0.089           738.5 / 0.145
 *     16 MiB         - / 0.38             - / 0.38              - / 0.072               - / 0.071
 *     64 MiB         - / 0.85             - / 0.83              - / 0.18                - / 0.20
 * 64 rows of 4 KiB: GCM 2.46 / 0.35 (seal), ChaCha20-Poly1305 1.12 / 0.055: the long pair wins there too.
 * qrkem.symmetric routes a call to the long pair when the longest row is known to the host and is at
 * least long_min_bytes = 4096, the smallest size measured: the long pair was faster at every measured size
 * (a one-lane GCM call costs about 0.55 ms per KiB; the long calls start at 0.34 ms, most of it the 64 KiB AES
 * table filled by the 64 lanes of the combining workgroup).  Batches of more than 64 rows, the largest
 * batch measured, stay on the one-lane pair (long_max_rows). */
int qrk_aead_long_layout(const char *alg, size_t out[4]);
int qrk_aead_seal_long_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *keys, const uint8_t *nonces,
                             const uint8_t *pt, const uint64_t *pt_off, const uint8_t *aad,
                             const uint64_t *aad_off, size_t aad_len, size_t max_len, uint8_t *sealed,
                             void *stream);
int qrk_aead_open_long_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *keys, const uint8_t *sealed,
                             const uint64_t *sealed_off, const uint8_t *aad, const uint64_t *aad_off,
                             size_t aad_len, size_t max_len, uint8_t *pt, int32_t *status, void *stream);
/* (The test hooks of the long calls, qrk_dbg_ghash_long_batch, qrk_dbg_poly1305_long_batch and
 * qrk_dbg_aead_long_residue, are declared in csrc/qrkem_debug.h.) */

/* ML-DSA signature verification (FIPS 204 final, "pure" ML-DSA: Verify, Algorithm 3), the step the
 * reference runs on every handshake and chat message (signatures.py:167 from messaging.py:721, 933,
 * 1174, 1480).  alg: "ML-DSA-44", "ML-DSA-65" or "ML-DSA-87"; any other name returns -1 with
 * qrk_last_error() set.  ML-DSA KeyGen and Sign are qrk_mldsa_keypair_batch and qrk_mldsa_sign_batch
 * below (the OQS_SIG registry of Part 1 stays empty); the hash-based names have qrk_sig_keypair_batch
 * and qrk_sig_sign_batch, which refuse an ML-DSA name.
 * The same two calls verify hash-based signatures, the SHA2 "f" parameter sets, in two flavours:
 * "SPHINCS+-SHA2-128f-simple", "SPHINCS+-SHA2-192f-simple", "SPHINCS+-SHA2-256f-simple" (the round-3.1
 * submission as liboqs ships it, what the reference's SPHINCSSignature asks for, signatures.py:208-212)
 * and "SLH-DSA-SHA2-128f", "SLH-DSA-SHA2-192f", "SLH-DSA-SHA2-256f" (FIPS 205 pure SLH-DSA, Algorithm 24).
 * The flavours differ in the message framing (FIPS 205: 0 || len(ctx) || ctx || M; round 3.1: M) and in
 * the bit order of the FORS indices, and do not verify each other's signatures.  Parity with liboqs and
 * the FIPS 205 KATs is unpinned, as for ML-DSA.
 * out[0..2] = public key, secret key, signature bytes; -1 for an unknown name. */
int qrk_sig_sizes(const char *alg, size_t out[3]);
/* n verifications.  Device pointers: pk [n][pk bytes], sig [n][sig bytes], messages ragged (bytes +
 * uint64[n+1] offsets, as qrk_aead_*), ctx_str / ctx_len one context string for all rows (NULL / 0 =
 * empty, what liboqs's OQS_SIG_sign uses; ctx_len > 255 returns -1).
 * status (required, int32[n]): 0 valid, -1 otherwise; every row is written exactly once.  A row of
 * 2^31 bytes or more gets -1.  Stream-ordered on `stream`; uses the context's scratch (k l KiB + about
 * 1.3 KB per row, grown on demand; qrk_ctx_set_chunk bounds the rows per launch).
 * SLH-DSA / SPHINCS+ names: the same contract; the scratch is the H_msg digest and a flag word per row
 * (38 / 46 / 53 bytes).  A context string exists only under the "SLH-DSA-" names (ctx_len > 255 returns
 * -1); under a "SPHINCS+-" name any ctx_len != 0 returns -1 before any device work. */
int qrk_sig_verify_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *pk, const uint8_t *msg,
                         const uint64_t *msg_off, const uint8_t *sig, const uint8_t *ctx_str, size_t ctx_len,
                         int32_t *status, void *stream);

/* SLH-DSA-SHA2 / SPHINCS+-SHA2-simple "f" key generation and signing: the other half of the reference's
 * SPHINCSSignature (signatures.py:238-292; sign is called on every key-exchange message and chat message,
 * messaging.py:620, 864, 1090).  alg: the six hash-based names of qrk_sig_sizes.  An ML-DSA name returns -1
 * with a message naming it and qrk_mldsa_keypair_batch / qrk_mldsa_sign_batch, any other name -1 "unsupported signature
 * algorithm".  Checked before any device work, in this order: null context, name, ctx_len > 255, a context
 * under a "SPHINCS+-" name; then n == 0 returns 0.  Device pointers, stream-ordered on `stream`.  Output is
 * byte-exact FIPS 205 Algorithm 18 / 19 (and the round-3.1 submission's) for the given seeds and opt_rand.
 * Rows per launch follow qrk_ctx_set_chunk (at most 65536); the context's scratch grows on demand by 950 /
 * 1462 / 1813 bytes per row (128f / 192f / 256f) and holds public values only: the H_msg digest, a flag
 * word, the hash states after PK.seed, the k FORS roots and the d XMSS roots.  SK.seed and SK.prf are read
 * from `sk` (KeyGen: from the sk being written) and never copied anywhere else.
 *
 * KeyGen: seeds [n][3 n_bytes] = SK.seed || SK.prf || PK.seed per row (n_bytes = 16 / 24 / 32; FIPS 205
 * Algorithm 18, the caller draws them); pk [n][pk bytes] = PK.seed || PK.root, sk [n][sk bytes] = seeds || PK.root. */
int qrk_sig_keypair_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *seeds, uint8_t *pk, uint8_t *sk,
                          void *stream);
/* Sign: sk [n][sk bytes]; messages ragged and ctx_str / ctx_len as qrk_sig_verify_batch; opt_rand NULL =
 * the deterministic variant (opt_rand = PK.seed), else [n][n_bytes] fresh random bytes per row (hedged);
 * sig [n][sig bytes].  status (required, int32[n]): 0, or -1 with an all-zero signature row for a row of 2^31
 * bytes or more, a row whose offsets decrease, or a secret key whose PK.root is not the root its SK.seed
 * and PK.seed give (a corrupt key); every row is written exactly once. */
int qrk_sig_sign_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *sk, const uint8_t *msg,
                       const uint64_t *msg_off, const uint8_t *opt_rand, const uint8_t *ctx_str, size_t ctx_len,
                       uint8_t *sig, int32_t *status, void *stream);

/* ML-DSA key generation and signing (FIPS 204 final, "pure" ML-DSA: KeyGen_internal, Algorithm 6, and Sign,
 * Algorithm 2 over Sign_internal, Algorithm 7): the other half of the reference's MLDSASignature, its default
 * signature (signatures.py generate_keypair / sign; sign is called on every key-exchange and chat message,
 * messaging.py:620, 864, 1090).  alg: "ML-DSA-44", "ML-DSA-65" or "ML-DSA-87".  A hash-based name returns -1 with
 * a message naming it and qrk_sig_keypair_batch / qrk_sig_sign_batch, any other name -1 "unsupported signature
 * algorithm".  Checked before any device work, in this order: null context, name, ctx_len > 255; then n == 0
 * returns 0; then null buffers.  Device pointers, stream-ordered on `stream`.  Output is byte-exact FIPS 204 for
 * the given xi and rnd.  Rows per launch follow qrk_ctx_set_chunk; the context's scratch grows on demand by
 * 16452 / 30788 / 57412 bytes per row (ML-DSA-44 / 65 / 87) and holds public values only: A_hat = ExpandA(rho)
 * (k l KiB), mu and a flag word.  xi, rho', K, rho'', s1, s2, t0 and the masks y are read from `xi` and `sk` into
 * registers and on-chip memory, which is zeroed before a workgroup exits, and are never copied anywhere else.
 *
 * KeyGen: xi [n][32], the caller draws them; pk [n][pk bytes], sk [n][sk bytes] (the sizes of qrk_sig_sizes). */
int qrk_mldsa_keypair_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *xi, uint8_t *pk, uint8_t *sk,
                            void *stream);
/* Sign: sk [n][sk bytes]; messages ragged and ctx_str / ctx_len as qrk_sig_verify_batch; rnd NULL = the
 * deterministic variant (32 zero bytes), else [n][32] fresh random bytes per row (hedged); sig [n][sig bytes].
 * status (required, int32[n]): 0, or -1 with an all-zero signature row for a row of 2^31 bytes or more, a row
 * whose offsets decrease, a secret key with an s1 / s2 coefficient outside [-eta, eta], or a row whose rejection
 * loop ran 814 iterations (the cap FIPS 204 Appendix C allows; about 2^-200 for an honest key) without an
 * accepted signature; every row is written exactly once. */
int qrk_mldsa_sign_batch(qrk_ctx *ctx, const char *alg, size_t n, const uint8_t *sk, const uint8_t *msg,
                         const uint64_t *msg_off, const uint8_t *rnd, const uint8_t *ctx_str, size_t ctx_len,
                         uint8_t *sig, int32_t *status, void *stream);

/* ML-DSA key sets: many rows under few keys.  A node verifies what each peer sends against that peer's one key
 * and signs everything with its own (messaging.py:600-620, 721, 864, 933, 1090, 1174, 1480, 1622); the calls above
 * redo per row what depends on the key alone (ExpandA, tr, the NTTs of t1 or of s1, s2, t0).  A key set holds g
 * keys expanded once, and the keyed calls take an index into it per row.
 *
 * Load: pk [g][pk bytes] or sk [g][sk bytes], device pointers; *out receives the handle.  The expansion is
 * stream-ordered on `stream`: calls that use the set on another stream must be ordered behind it by the caller,
 * and `pk` / `sk` may be released once that stream has passed the load.  Checked before any device work, in this
 * order: null context, name (anything but the three ML-DSA names: -1 "unsupported signature algorithm"), g == 0,
 * null pointers, g beyond what the context's scratch budget rule allows for one allocation.  A set holds
 * 20544 / 36928 / 65600 (public) or 28804 / 48260 / 81028 (secret) bytes of device memory per key for
 * ML-DSA-44 / 65 / 87.  A secret set holds K and the NTTs of s1, s2 and t0 of its keys: next to the caller's sk
 * rows and the signatures it is the only place in device memory with secret-derived bytes.
 * qrk_mldsa_keyset_free synchronises the device, zeroes the whole allocation and then frees it (NULL: no-op);
 * free a set before the device is reset.  qrk_ctx_cleanse does not touch key sets.
 * qrk_mldsa_keyset_info: out = { g, parameter set (0, 1, 2 = ML-DSA-44, 65, 87), 1 if secret, device bytes held }. */
typedef struct qrk_mldsa_keyset qrk_mldsa_keyset;
int qrk_mldsa_pubkeys_load(qrk_ctx *ctx, const char *alg, size_t g, const uint8_t *pk, qrk_mldsa_keyset **out,
                           void *stream);
int qrk_mldsa_seckeys_load(qrk_ctx *ctx, const char *alg, size_t g, const uint8_t *sk, qrk_mldsa_keyset **out,
                           void *stream);
int qrk_mldsa_keyset_info(const qrk_mldsa_keyset *ks, size_t out[4]);
void qrk_mldsa_keyset_free(qrk_mldsa_keyset *ks);
/* Verify / Sign under a key set: row i uses key key_index[i] (uint32 [n], a device pointer; NULL means "every
 * row uses key 0" and is accepted only when g == 1); every other argument as in qrk_sig_verify_batch /
 * qrk_mldsa_sign_batch, and so are the results: byte for byte what those calls return for the same keys.  An
 * index >= g is checked on the device before anything is addressed with it and makes the row a refused one:
 * status -1 (and an all-zero signature when signing).  A row that names a secret key with an s1 / s2 coefficient
 * outside [-eta, eta] is refused in the same way.  Checked before any device work, in this order: null context;
 * a null or foreign key set (loaded on another device than the context's, or a public set passed to the signing
 * call / a secret set to the verifying one), with a message that says which; ctx_len > 255; then n == 0 returns
 * 0; then null buffers.  The context's scratch grows by 1092 / 1092 / 1348 bytes per verified row and 68 bytes per
 * signed row (public values only). */
int qrk_mldsa_verify_keyed_batch(qrk_ctx *ctx, const qrk_mldsa_keyset *ks, size_t n, const uint32_t *key_index,
                                 const uint8_t *msg, const uint64_t *msg_off, const uint8_t *sig,
                                 const uint8_t *ctx_str, size_t ctx_len, int32_t *status, void *stream);
int qrk_mldsa_sign_keyed_batch(qrk_ctx *ctx, const qrk_mldsa_keyset *ks, size_t n, const uint32_t *key_index,
                               const uint8_t *msg, const uint64_t *msg_off, const uint8_t *rnd,
                               const uint8_t *ctx_str, size_t ctx_len, uint8_t *sig, int32_t *status, void *stream);

/* ML-KEM key sets: many rows under few keys.  A service with a long-lived KEM key decapsulates everything sent to
 * that key, and a node encapsulates to one peer key many times; qrk_kem_encaps_batch / qrk_kem_decaps_batch redo
 * per row what depends on the key alone (SampleNTT for the whole matrix A_hat, H(ek), Encaps' modulus check).  A
 * key set holds g keys expanded once, and the keyed calls take an index into it per row.
 *
 * Load: pk [g][pk bytes] or sk [g][sk bytes], device pointers; *out receives the handle.  The expansion is
 * stream-ordered on `stream`: calls that use the set on another stream must be ordered behind it by the caller,
 * and `pk` / `sk` may be released once that stream has passed the load.  Checked before any device work, in this
 * order: null context, name (anything but the three ML-KEM names: -1, a FrodoKEM or HQC name with "key sets are
 * ML-KEM only", any other with "unsupported KEM"), g == 0, null pointers, g beyond what the context's scratch
 * budget rule allows for one allocation (and 2^32 - 1).  An ek that fails the FIPS 203 modulus check loads all the
 * same and is marked: rows that name it return what qrk_kem_encaps_batch returns for it, status -1 included.
 * A set holds 2372 / 4676 / 7748 (public: A_hat, ek, H(ek), the mark) or 3168 / 5856 / 9312 (secret: A_hat, dk)
 * bytes of device memory per key for ML-KEM-512 / 768 / 1024, plus at most 1 KiB of alignment per set.  A secret
 * set holds the dk bytes of its keys: next to the caller's sk rows it is the only long-lived place in device
 * memory with secret-derived bytes.  qrk_mlkem_keyset_free synchronises the device, zeroes the whole allocation
 * and then frees it (NULL: no-op); free a set before the device is reset.  qrk_ctx_cleanse does not touch key sets.
 * qrk_mlkem_keyset_info: out = { g, parameter set (0, 1, 2 = ML-KEM-512, 768, 1024), 1 if secret, device bytes held }. */
typedef struct qrk_mlkem_keyset qrk_mlkem_keyset;
int qrk_mlkem_pubkeys_load(qrk_ctx *ctx, const char *alg, size_t g, const uint8_t *pk, qrk_mlkem_keyset **out,
                           void *stream);
int qrk_mlkem_seckeys_load(qrk_ctx *ctx, const char *alg, size_t g, const uint8_t *sk, qrk_mlkem_keyset **out,
                           void *stream);
int qrk_mlkem_keyset_info(const qrk_mlkem_keyset *ks, size_t out[4]);
void qrk_mlkem_keyset_free(qrk_mlkem_keyset *ks);
/* Encaps / Decaps under a key set: row i uses key key_index[i] (uint32 [n], a device pointer; NULL means "every
 * row uses key 0" and is accepted only when g == 1); every other argument as in qrk_kem_encaps_batch /
 * qrk_kem_decaps_batch_status (coins NULL: the OS CSPRNG; status NULL: not reported), and so are the results: byte
 * for byte what those calls return for the same keys and coins.  An index >= g is checked on the device before
 * anything is addressed with it and makes the row a refused one: status -1 and an all-zero ct / ss row; its
 * neighbours are untouched.  No step's work depends on whether a ciphertext is valid or a row refused.  Checked
 * before any device work, in this order: null context; a null or foreign key set (loaded on another device than
 * the context's, or a public set passed to Decaps / a secret set to Encaps), with a message that says which; then
 * n == 0 returns 0; then null buffers.  Rows run in chunks of the context's chunk; the scratch grows by 1088 /
 * 1472 / 1856 bytes per row (ML-KEM-512 / 768 / 1024: PRF words, seeds, m', K', Kbar -- no matrix), and the four
 * secret records are zeroed behind every chunk. */
int qrk_mlkem_encaps_keyed_batch(qrk_ctx *ctx, const qrk_mlkem_keyset *ks, size_t n, const uint32_t *key_index,
                                 uint8_t *ct, uint8_t *ss, const uint8_t *coins, int32_t *status, void *stream);
int qrk_mlkem_decaps_keyed_batch(qrk_ctx *ctx, const qrk_mlkem_keyset *ks, size_t n, const uint32_t *key_index,
                                 uint8_t *ss, const uint8_t *ct, int32_t *status, void *stream);

/* FrodoKEM key sets: the same contract for the six FrodoKEM names (640 / 976 / 1344, SHAKE and AES), where the key
 * alone decides most of a row's cost: qrk_kem_encaps_batch / qrk_kem_decaps_batch regenerate the N x N matrix A from
 * seedA (FrodoKEM-640: 5,120 Keccak permutations, or 51,200 AES blocks) and hash the whole public key for every row.
 * A key set generates A once per key, and the keyed calls compute S'A for all rows that share a key as one integer
 * matrix product against the stored A.
 *
 * Load, free and info are qrk_mlkem_pubkeys_load .. qrk_mlkem_keyset_free word for word, with these differences.  The
 * name check accepts the six FrodoKEM names (an ML-KEM or HQC name: -1 with "these key sets are FrodoKEM only", any
 * other with "unsupported KEM").  Nothing about a key is checked at load (FrodoKEM has no key validity check).  A
 * set holds, per key, A as two planes of int8 limbs (A = 256 hi + lo, 2 N^2 bytes), B unpacked to 16-bit words
 * (16 N) and pkh (32); a secret set adds S^T (16 N) and s (32), which are secret.  That is 829,472 / 1,920,800 /
 * 3,634,208 bytes per public key and 839,744 / 1,936,448 / 3,655,744 per secret key for FrodoKEM-640 / 976 / 1344,
 * plus at most 1.5 KiB of alignment and slack per set: 64 FrodoKEM-1344 keys are 233 MB.  A load whose allocation
 * fails is refused with a message that names the size; nothing is left allocated.
 * qrk_frodo_keyset_info: out = { g, parameter set (0 .. 5 = 640-SHAKE, 640-AES, 976-SHAKE, 976-AES, 1344-SHAKE,
 * 1344-AES), 1 if secret, device bytes held }.
 *
 * Encaps / Decaps under a set are qrk_mlkem_encaps_keyed_batch / qrk_mlkem_decaps_keyed_batch word for word: the same
 * arguments (coins: mu, len_mu bytes per row), the same checks in the same order, refused rows (index >= g: status
 * -1, an all-zero ct / ss row, and the row takes no part in the matrix product) and results byte for byte those of
 * qrk_kem_encaps_batch / qrk_kem_decaps_batch for the same keys and coins.  status is 0 for every other row (Decaps
 * rejects implicitly).  Rows are grouped by key on the device (key_index is public); results do not depend on the
 * order of rows or on how keys interleave.  The scratch grows by 46.5 / 71.1 / 97.7 KB per row (64 N + 8 NP + 420
 * bytes, NP = N rounded up to 128; the per-row calls take 150 / 323 / 552 KB) plus 16 bytes per key, and the secret
 * records (seedSE, k, mu', the hashed key) are zeroed behind every chunk. */
typedef struct qrk_frodo_keyset qrk_frodo_keyset;
int qrk_frodo_pubkeys_load(qrk_ctx *ctx, const char *alg, size_t g, const uint8_t *pk, qrk_frodo_keyset **out,
                           void *stream);
int qrk_frodo_seckeys_load(qrk_ctx *ctx, const char *alg, size_t g, const uint8_t *sk, qrk_frodo_keyset **out,
                           void *stream);
int qrk_frodo_keyset_info(const qrk_frodo_keyset *ks, size_t out[4]);
void qrk_frodo_keyset_free(qrk_frodo_keyset *ks);
int qrk_frodo_encaps_keyed_batch(qrk_ctx *ctx, const qrk_frodo_keyset *ks, size_t n, const uint32_t *key_index,
                                 uint8_t *ct, uint8_t *ss, const uint8_t *coins, int32_t *status, void *stream);
int qrk_frodo_decaps_keyed_batch(qrk_ctx *ctx, const qrk_frodo_keyset *ks, size_t n, const uint32_t *key_index,
                                 uint8_t *ss, const uint8_t *ct, int32_t *status, void *stream);

/* Wire format: standard base64 (RFC 4648 section 4, '=' padding), the encoding the reference
 * puts every KEM payload in before JSON framing (messaging.py:607 public key, :852-853
 * ciphertext and responder key; decoded at :829 with base64.b64decode).  Device pointers,
 * contiguous records.  Encode: in [n][in_len] -> out [n][4*ceil(in_len/3)] ASCII (no NUL).
 * Decode (strict): in [n][4*ceil(out_len/3)] -> out [n][out_len]; status (nullable, int32[n])
 * = -1 for a record with a byte outside the alphabet or misplaced / missing padding, else 0.
 * (Python's b64decode without validate=True would silently skip such bytes; a malformed KEM
 * field is rejected here instead.) */
int qrk_base64_encode_batch(qrk_ctx *ctx, size_t n, const uint8_t *in, size_t in_len, uint8_t *out, void *stream);
int qrk_base64_decode_batch(qrk_ctx *ctx, size_t n, const uint8_t *in, size_t out_len, uint8_t *out,
                            int32_t *status, void *stream);

/* Per-kernel HIP-event timing on the launch stream (for bench.py's roofline).
 * qrk_ctx_profile(ctx, 1) resets and enables; qrk_ctx_profile_collect()
 * synchronises the recorded events and returns the number of distinct kernel
 * names; qrk_ctx_profile_get() reads (name, total ms, launches) for entry i. */
int qrk_ctx_profile(qrk_ctx *ctx, int enable);
int qrk_ctx_profile_collect(qrk_ctx *ctx);
int qrk_ctx_profile_get(qrk_ctx *ctx, int i, const char **name, double *total_ms, uint64_t *launches);

const char *qrk_last_error(void);
int qrk_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* QRKEM_H */
