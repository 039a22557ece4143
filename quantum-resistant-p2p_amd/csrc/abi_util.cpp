// The small calls of the batched API (include/qrkem.h) that belong to no family: the benchmark's input
// generators, row digests, HKDF-SHA256 and base64.
#include "abi_ctx.h"

using namespace qrk;

extern "C" {

int qrk_bench_coins(qrk_ctx* ctx, size_t n, size_t len, uint64_t seed, uint64_t first, uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  CallScope scope;  // no lock, no timer: bench.py's input generator, like qrk_tamper below
  if (scope.open(ctx, (hipStream_t)stream, 0)) return -1;
  hipError_t e = bench_coins(n, len, seed, first, out, (hipStream_t)stream);
  return hip_done("bench_coins", e);
}

int qrk_tamper(qrk_ctx* ctx, size_t n, size_t ctlen, uint64_t seed, int mode, uint8_t* ct, void* stream) {
  if (!ctx) return fail("null context");
  // no lock (touches nothing of the context's); no timer: bench.py calls this inside its profiled,
  // timed step, and timing it would change the reported profile
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, 0)) return -1;
  hipError_t e = tamper_ciphertexts(n, ctlen, seed, mode, ct, (hipStream_t)stream);
  return hip_done("tamper", e);
}

int qrk_digest_rows(qrk_ctx* ctx, size_t n, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len,
                    uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  if (n && (!a || !out || (b_len && !b))) return fail("null buffer");
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = digest_rows(n, a, a_len, b_len ? b : nullptr, b_len, out, (hipStream_t)stream);
  return hip_done("digest_rows", e);
}

int qrk_hkdf_sha256_batch(qrk_ctx* ctx, size_t n, const uint8_t* ikm, size_t ikm_len, const uint8_t* salt,
                          size_t salt_len, const uint8_t* info, const uint64_t* info_off, size_t info_len,
                          uint8_t* okm, size_t okm_len, void* stream) {
  if (!ctx) return fail("null context");
  if (okm_len == 0 || okm_len > 255 * 32) return fail("HKDF-SHA256 output length must be 1..8160 bytes");
  if (salt_len && !salt) return fail("salt_len > 0 with a NULL salt");
  if (n && (!ikm || !okm || (!info && (info_off || info_len)))) return fail("null buffer");
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = hkdf_sha256(n, ikm, ikm_len, ikm_len, salt, salt_len, info, info_off, info_len, okm_len, okm,
                             okm_len, (hipStream_t)stream);
  return hip_done("hkdf_sha256", e);
}

int qrk_base64_encode_batch(qrk_ctx* ctx, size_t n, const uint8_t* in, size_t in_len, uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  if (n && in_len && (!in || !out)) return fail("null buffer");
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = base64_encode(n, in, in_len, out, (hipStream_t)stream);
  return hip_done("base64_encode", e);
}

int qrk_base64_decode_batch(qrk_ctx* ctx, size_t n, const uint8_t* in, size_t out_len, uint8_t* out, int32_t* status,
                            void* stream) {
  if (!ctx) return fail("null context");
  if (n && out_len && (!in || !out)) return fail("null buffer");
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = hipSuccess;
  if (status && n) e = hipMemsetAsync(status, 0, n * sizeof(int32_t), (hipStream_t)stream);
  if (e == hipSuccess) e = base64_decode(n, in, out_len, out, status, (hipStream_t)stream);
  return hip_done("base64_decode", e);
}

}  // extern "C"
