// The AEAD calls of the batched API (include/qrkem.h): one lane per message (aead.hip) and one row across many
// workgroups (aead_long.hip), with the MAC and residue hooks of both (qrkem_debug.h).
#include "abi_ctx.h"

using namespace qrk;

// "AES-256-GCM" / "ChaCha20-Poly1305": the reference's SymmetricAlgorithm.name strings (symmetric.py:72, 170)
static int resolve_aead(const char* alg, AeadAlg* out) {
  if (alg && !strcmp(alg, "AES-256-GCM")) return *out = AeadAlg::AES_256_GCM, 0;
  if (alg && !strcmp(alg, "ChaCha20-Poly1305")) return *out = AeadAlg::CHACHA20_POLY1305, 0;
  return fail(std::string("unsupported AEAD: ") + (alg ? alg : "(null)"));
}

// The argument checks the four AEAD calls share, in the order qrkem.h documents (`bufs`: no required pointer is
// null; aad may be NULL only with no offsets and no length).  -1: failed, 1: n == 0, 0: go, `which` set.
static int aead_args(qrk_ctx* ctx, const char* alg, size_t n, bool bufs, const uint8_t* aad, const uint64_t* aad_off,
                     size_t aad_len, AeadAlg* which) {
  if (!ctx) return fail("null context");
  if (resolve_aead(alg, which)) return -1;
  if (n == 0) return 1;
  if (!bufs || (!aad && (aad_off || aad_len))) return fail("null buffer");
  if (aad_len >> 31) return fail("AEAD row lengths are 32-bit: aad_len must be below 2^31");
  return 0;
}

extern "C" {

int qrk_aead_seal_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* nonces,
                        const uint8_t* pt, const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off,
                        size_t aad_len, uint8_t* sealed, void* stream) {
  AeadAlg which;
  const bool bufs = keys && pt && pt_off && sealed;
  if (const int r = aead_args(ctx, alg, n, bufs, aad, aad_off, aad_len, &which)) return r < 0 ? -1 : 0;
  hipStream_t st = (hipStream_t)stream;
  // nonces == NULL: n fresh 96-bit nonces from the OS CSPRNG (os.urandom(12), symmetric.py:110, 208),
  // staged and wiped like OS-drawn coins (run_batch).  The staging belongs to the context, so the call
  // is ordered behind the context's previous one and recorded as its last use.
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  CoinWipe nonce_wipe{ctx, st};
  if (!nonces) {
    nonces = stage_os_random(ctx, n * 12, st, nonce_wipe);
    if (!nonces) return -1;
  }
  hipError_t e = aead_seal(which, n, keys, nonces, pt, pt_off, aad, aad_off, aad_len, sealed, st);
  return hip_done("aead_seal", e);
}

int qrk_aead_open_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* sealed,
                        const uint64_t* sealed_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                        uint8_t* pt, int32_t* status, void* stream) {
  AeadAlg which;
  const bool bufs = keys && sealed && sealed_off && pt && status;
  if (const int r = aead_args(ctx, alg, n, bufs, aad, aad_off, aad_len, &which)) return r < 0 ? -1 : 0;
  CallScope scope;  // not ordered against the context's last use: Open touches no context buffer
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = aead_open(which, n, keys, sealed, sealed_off, aad, aad_off, aad_len, pt, status, (hipStream_t)stream);
  return hip_done("aead_open", e);
}

// test hooks (qrkem_debug.h): Poly1305 and GHASH on chosen keys
int qrk_dbg_poly1305_batch(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, uint8_t* tag,
                           void* stream) {
  if (n && (!key32 || !msg || !msg_off || !tag)) return fail("null buffer");
  launch_begin();  // no context, so no scope
  hipError_t e = dbg_poly1305(n, key32, msg, msg_off, tag, (hipStream_t)stream);
  return hip_done("dbg_poly1305", e);
}
int qrk_dbg_ghash_batch(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, uint8_t* out,
                        void* stream) {
  if (n && (!h || !data || !data_off || !out)) return fail("null buffer");
  launch_begin();
  hipError_t e = dbg_ghash(n, h, data, data_off, out, (hipStream_t)stream);
  return hip_done("dbg_ghash", e);
}

// ------------------------------------------------------------------ AEAD, one row across many workgroups (aead_long.hip)
int qrk_aead_long_layout(const char* alg, size_t out[4]) {
  AeadAlg which;
  if (resolve_aead(alg, &which)) return -1;
  if (!out) return fail("null argument");
  aead_long_layout(which, out);
  return 0;
}

// The checks the long calls add to those of qrk_aead_seal_batch / qrk_aead_open_batch, all before any device work:
// the bound itself, the grid, and the scratch (segment partials + a verdict word per row) against the budget that
// caps every family's scratch (scratch_cap: QRK_SCRATCH_GIB).
static int aead_long_args(AeadAlg which, size_t n, size_t max_len) {
  if (max_len == 0 || max_len >> 31) return fail("max_len must be at least 1 and below 2^31");
  size_t lay[4];
  aead_long_layout(which, lay);
  const size_t segs = (max_len + lay[0] - 1) / lay[0], budget = (size_t)QRK_SCRATCH_GIB << 30;
  if (n > (((size_t)1 << 31) - 1) / segs)
    return fail("n rows of ceil(max_len / S) segments must stay below 2^31 workgroups: split the batch");
  if (aead_long_scratch_bytes(which, n, max_len) > budget)
    return fail("the segment partials of n rows of max_len bytes exceed the scratch budget (" +
                std::to_string(QRK_SCRATCH_GIB) + " GiB): split the batch");
  return 0;
}
// ... and the scratch itself, once the call is open
static int aead_long_scratch(qrk_ctx* ctx, AeadAlg which, size_t n, size_t max_len, hipStream_t st) {
  if (grow_device(ctx, &ctx->scratch, &ctx->scratch_bytes, aead_long_scratch_bytes(which, n, max_len), st)) return -1;
  ctx->aead_long_part = aead_long_part_bytes(which, n, max_len);
  return 0;
}

int qrk_aead_seal_long_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* nonces,
                             const uint8_t* pt, const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off,
                             size_t aad_len, size_t max_len, uint8_t* sealed, void* stream) {
  AeadAlg which;
  const bool bufs = keys && pt && pt_off && sealed;
  if (const int r = aead_args(ctx, alg, n, bufs, aad, aad_off, aad_len, &which)) return r < 0 ? -1 : 0;
  if (aead_long_args(which, n, max_len)) return -1;
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  if (aead_long_scratch(ctx, which, n, max_len, st)) return -1;
  CoinWipe nonce_wipe{ctx, st};
  if (!nonces) {
    nonces = stage_os_random(ctx, n * 12, st, nonce_wipe);
    if (!nonces) return -1;
  }
  hipError_t e = aead_seal_long(which, n, keys, nonces, pt, pt_off, aad, aad_off, aad_len, max_len, sealed, ctx->scratch, st);
  return hip_done("aead_seal_long", e);
}

int qrk_aead_open_long_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* sealed,
                             const uint64_t* sealed_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                             size_t max_len, uint8_t* pt, int32_t* status, void* stream) {
  AeadAlg which;
  const bool bufs = keys && sealed && sealed_off && pt && status;
  if (const int r = aead_args(ctx, alg, n, bufs, aad, aad_off, aad_len, &which)) return r < 0 ? -1 : 0;
  if (aead_long_args(which, n, max_len)) return -1;
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;  // ordered: unlike qrk_aead_open_batch this call uses the context's scratch
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  if (aead_long_scratch(ctx, which, n, max_len, st)) return -1;
  hipError_t e = aead_open_long(which, n, keys, sealed, sealed_off, aad, aad_off, aad_len, max_len, pt, status,
                                ctx->scratch, st);
  return hip_done("aead_open_long", e);
}

// test hooks (qrkem_debug.h): the long calls' segment and tail MAC machinery on chosen keys, and what it left behind
static int dbg_mac_long(qrk_ctx* ctx, AeadAlg which, size_t n, const uint8_t* key, const uint8_t* data,
                        const uint64_t* data_off, size_t max_len, uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  if (n == 0) return 0;
  if (!key || !data || !data_off || !out) return fail("null buffer");
  if (aead_long_args(which, n, max_len)) return -1;
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  if (aead_long_scratch(ctx, which, n, max_len, st)) return -1;
  hipError_t e = which == AeadAlg::AES_256_GCM ? dbg_ghash_long(n, key, data, data_off, max_len, out, ctx->scratch, st)
                                               : dbg_poly1305_long(n, key, data, data_off, max_len, out, ctx->scratch, st);
  return hip_done("dbg_mac_long", e);
}
int qrk_dbg_ghash_long_batch(qrk_ctx* ctx, size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off,
                             size_t max_len, uint8_t* out, void* stream) {
  return dbg_mac_long(ctx, AeadAlg::AES_256_GCM, n, h, data, data_off, max_len, out, stream);
}
int qrk_dbg_poly1305_long_batch(qrk_ctx* ctx, size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off,
                                size_t max_len, uint8_t* tag, void* stream) {
  return dbg_mac_long(ctx, AeadAlg::CHACHA20_POLY1305, n, key32, msg, msg_off, max_len, tag, stream);
}
int qrk_dbg_aead_long_residue(qrk_ctx* ctx, uint64_t* out) {
  CallScope scope;
  if (open_inspect(scope, ctx, out)) return -1;
  *out = 0;
  const size_t bytes = std::min(ctx->aead_long_part, ctx->scratch_bytes);
  if (!bytes) return 0;
  return read_residue(
      ctx->scratch, bytes, [](uint64_t acc, uint8_t x) { return acc | x; }, "hipMemcpy(long AEAD residue)", out);
}

}  // extern "C"
