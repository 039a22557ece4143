// The signature calls of the batched API (include/qrkem.h): ML-DSA and SLH-DSA / SPHINCS+ verification, key
// generation and signing, ML-DSA key sets, and their trace hooks (qrkem_debug.h).
#include "abi_ctx.h"

using namespace qrk;

extern "C" {

// ------------------------------------------------------------------ signatures (mldsa.hip, slhdsa.hip, slhdsa_sign.hip)
// One family lookup for every entry point: ML-DSA first, then SLH-DSA / SPHINCS+.
enum { SIG_ANY = -1, SIG_MLDSA, SIG_SLHDSA };
struct SigAlg {
  int family = SIG_ANY;  // SIG_ANY: no family has the name
  int which = -1;
  SigSizes sz{};
};
static SigAlg sig_find(const char* alg) {
  SigAlg a;
  if ((a.which = mldsa_find(alg)) >= 0)
    a.family = SIG_MLDSA, a.sz = mldsa_sizes(a.which);
  else if ((a.which = slhdsa_find(alg)) >= 0)
    a.family = SIG_SLHDSA, a.sz = slhdsa_sizes(a.which);
  return a;
}
static int sig_unsupported(const char* alg) {
  return fail(std::string("unsupported signature algorithm: ") + (alg ? alg : "(null)"));
}

int qrk_sig_sizes(const char* alg, size_t out[3]) {
  const SigAlg a = sig_find(alg);
  if (a.family == SIG_ANY || !out) return sig_unsupported(alg);
  out[0] = a.sz.pk, out[1] = a.sz.sk, out[2] = a.sz.sig;
  return 0;
}

// The argument checks of every signature call in the order qrkem.h documents (a trace hook or a qrk_mldsa_* call
// takes its own `family` only; of the signing calls the generic pair takes no ML-DSA name and the ML-DSA pair no
// hash-based one, each naming the other; `bufs`: no required pointer is null).  -1: failed, 1: n == 0, 0: go, `a` set.
static int sig_args(qrk_ctx* ctx, const char* alg, int family, bool signing, size_t ctx_len, size_t n, bool bufs,
                    SigAlg& a) {
  if (!ctx) return fail("null context");
  a = sig_find(alg);
  if (signing && family == SIG_MLDSA && a.family == SIG_SLHDSA)
    return fail(std::string(alg) + ": a hash-based parameter set: its KeyGen and Sign are qrk_sig_keypair_batch / "
                                   "qrk_sig_sign_batch");
  if (a.family == SIG_ANY || (family != SIG_ANY && family != a.family)) return sig_unsupported(alg);
  if (signing && family == SIG_ANY && a.family == SIG_MLDSA)
    return fail(std::string(alg) + ": the generic signing calls have no ML-DSA KeyGen or Sign (they are "
                                   "qrk_mldsa_keypair_batch / qrk_mldsa_sign_batch)");
  if (ctx_len > 255) return fail(a.family == SIG_MLDSA ? "ML-DSA context strings are at most 255 bytes"
                                                       : "SLH-DSA context strings are at most 255 bytes");
  if (a.family == SIG_SLHDSA && ctx_len && !slhdsa_is_fips(a.which))
    return fail(std::string(alg) + " is the round-3.1 submission, which has no context string (ctx_len must be 0; "
                                   "the SLH-DSA-SHA2-* names take one)");
  if (n == 0) return 1;
  return bufs ? 0 : fail("null buffer");
}

// Verification, one call site per family behind the public call and that family's trace hook.  Chunks are capped
// like the KEM families' (ML-DSA's scratch: k l KiB + 1.3 KB per row; SLH-DSA's: 38 to 53 bytes) and at 2^20 rows.
struct VerifyIo {  // the arguments of qrk_sig_verify_batch that a chunk's launcher sees
  const uint8_t *pk, *msg;
  const uint64_t* msg_off;
  const uint8_t *sig, *ctx_str;
  size_t ctx_len;
  int32_t* status;
  bool set() const { return pk && msg && msg_off && sig && status && (ctx_str || !ctx_len); }
};
static size_t verify_cap(size_t per_row) { return std::min((size_t)1 << 20, scratch_cap(per_row)); }

static int mldsa_verify_rows(qrk_ctx* ctx, const SigAlg& a, size_t n, const VerifyIo& v, const MldsaTrace& trace,
                             hipStream_t st) {
  return run_rows(ctx, st, n, verify_cap(mldsa_scratch_bytes(a.which, 1)), mldsa_scratch_bytes, a.which, "mldsa_verify",
                  [&](size_t off, size_t m) {
                    return mldsa_verify(a.which, m, v.pk + off * a.sz.pk, v.msg, v.msg_off + off, v.sig + off * a.sz.sig,
                                        v.ctx_str, v.ctx_len, v.status + off, mldsa_trace_at(a.which, trace, off),
                                        ctx->scratch, st);
                  });
}
static int slhdsa_verify_rows(qrk_ctx* ctx, const SigAlg& a, size_t n, const VerifyIo& v, const SlhdsaTrace& trace,
                              hipStream_t st) {
  return run_rows(ctx, st, n, verify_cap(slhdsa_scratch_bytes(a.which, 1)), slhdsa_scratch_bytes, a.which,
                  "slhdsa_verify", [&](size_t off, size_t m) {
                    return slhdsa_verify(a.which, m, v.pk + off * a.sz.pk, v.msg, v.msg_off + off, v.sig + off * a.sz.sig,
                                         v.ctx_str, v.ctx_len, v.status + off, slhdsa_trace_at(a.which, trace, off),
                                         ctx->scratch, st);
                  });
}

int qrk_sig_verify_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* pk, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                         int32_t* status, void* stream) {
  const VerifyIo v{pk, msg, msg_off, sig, ctx_str, ctx_len, status};
  SigAlg a;
  if (const int r = sig_args(ctx, alg, SIG_ANY, false, ctx_len, n, v.set(), a)) return r < 0 ? -1 : 0;
  return a.family == SIG_MLDSA ? mldsa_verify_rows(ctx, a, n, v, MldsaTrace{}, (hipStream_t)stream)
                               : slhdsa_verify_rows(ctx, a, n, v, SlhdsaTrace{}, (hipStream_t)stream);
}

// Key generation and signing (slhdsa_sign.hip): at most SLHDSA_SIGN_MAX_ROWS rows per launch, what one grid takes.
int qrk_sig_keypair_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* seeds, uint8_t* pk, uint8_t* sk,
                          void* stream) {
  SigAlg a;
  if (const int r = sig_args(ctx, alg, SIG_ANY, true, 0, n, seeds && pk && sk, a)) return r < 0 ? -1 : 0;
  hipStream_t st = (hipStream_t)stream;
  return run_rows(ctx, st, n, SLHDSA_SIGN_MAX_ROWS, slhdsa_sign_scratch_bytes, a.which, "slhdsa_keypair",
                  [&](size_t off, size_t m) {
                    return slhdsa_keypair(a.which, m, seeds + off * 3 * a.sz.n, pk + off * a.sz.pk, sk + off * a.sz.sk,
                                          ctx->scratch, st);
                  });
}

int qrk_sig_sign_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* msg,
                       const uint64_t* msg_off, const uint8_t* opt_rand, const uint8_t* ctx_str, size_t ctx_len,
                       uint8_t* sig, int32_t* status, void* stream) {
  SigAlg a;
  const bool bufs = sk && msg && msg_off && sig && status && (ctx_str || !ctx_len);
  if (const int r = sig_args(ctx, alg, SIG_ANY, true, ctx_len, n, bufs, a)) return r < 0 ? -1 : 0;
  hipStream_t st = (hipStream_t)stream;
  return run_rows(ctx, st, n, SLHDSA_SIGN_MAX_ROWS, slhdsa_sign_scratch_bytes, a.which, "slhdsa_sign",
                  [&](size_t off, size_t m) {
                    return slhdsa_sign(a.which, m, sk + off * a.sz.sk, msg, msg_off + off,
                                       opt_rand ? opt_rand + off * a.sz.n : nullptr, ctx_str, ctx_len, sig + off * a.sz.sig,
                                       status + off, ctx->scratch, st);
                  });
}

// ML-DSA key generation and signing (mldsa_sign.hip).  Chunks are capped like verification's: the scratch is
// A_hat, k l KiB per row, plus 68 bytes.
int qrk_mldsa_keypair_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* xi, uint8_t* pk, uint8_t* sk,
                            void* stream) {
  SigAlg a;
  if (const int r = sig_args(ctx, alg, SIG_MLDSA, true, 0, n, xi && pk && sk, a)) return r < 0 ? -1 : 0;
  hipStream_t st = (hipStream_t)stream;
  return run_rows(ctx, st, n, verify_cap(mldsa_sign_scratch_bytes(a.which, 1)), mldsa_sign_scratch_bytes, a.which,
                  "mldsa_keypair", [&](size_t off, size_t m) {
                    return mldsa_keypair(a.which, m, xi + off * 32, pk + off * a.sz.pk, sk + off * a.sz.sk, ctx->scratch,
                                         st);
                  });
}

// qrk_mldsa_sign_batch and its traced twin qrk_dbg_mldsa_sign_trace (iters != NULL): one body
static int mldsa_sign_call(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* msg,
                           const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len,
                           uint8_t* sig, int32_t* status, uint32_t max_iters, bool traced, uint8_t* mu, uint32_t* iters,
                           hipStream_t st) {
  SigAlg a;
  const bool bufs = sk && msg && msg_off && sig && status && (ctx_str || !ctx_len) && (!traced || (mu && iters));
  if (const int r = sig_args(ctx, alg, SIG_MLDSA, true, ctx_len, n, bufs, a)) return r < 0 ? -1 : 0;
  return run_rows(ctx, st, n, verify_cap(mldsa_sign_scratch_bytes(a.which, 1)), mldsa_sign_scratch_bytes, a.which,
                  "mldsa_sign", [&](size_t off, size_t m) {
                    return mldsa_sign(a.which, m, sk + off * a.sz.sk, msg, msg_off + off, rnd ? rnd + off * 32 : nullptr,
                                      ctx_str, ctx_len, sig + off * a.sz.sig, status + off, max_iters,
                                      traced ? mu + off * 64 : nullptr, traced ? iters + off : nullptr, ctx->scratch, st);
                  });
}

int qrk_mldsa_sign_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len,
                         uint8_t* sig, int32_t* status, void* stream) {
  return mldsa_sign_call(ctx, alg, n, sk, msg, msg_off, rnd, ctx_str, ctx_len, sig, status, MLDSA_SIGN_MAX_ITERS, false,
                         nullptr, nullptr, (hipStream_t)stream);
}

// test hook (qrkem_debug.h): the call above with the loop's cap as an argument and the trace outputs
int qrk_dbg_mldsa_sign_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* msg,
                             const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str, size_t ctx_len,
                             uint8_t* sig, int32_t* status, uint32_t max_iters, uint8_t* mu, uint32_t* iters,
                             void* stream) {
  return mldsa_sign_call(ctx, alg, n, sk, msg, msg_off, rnd, ctx_str, ctx_len, sig, status, max_iters, true, mu, iters,
                         (hipStream_t)stream);
}

// test hook (qrkem_debug.h): qrk_sig_verify_batch for an ML-DSA name, with the trace outputs
int qrk_dbg_mldsa_verify_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* pk, const uint8_t* msg,
                               const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                               int32_t* status, uint8_t* mu, uint8_t* ctilde, uint8_t* w1, uint32_t* flags,
                               void* stream) {
  if (n && (!mu || !ctilde || !w1 || !flags)) return fail("null trace buffer");
  const VerifyIo v{pk, msg, msg_off, sig, ctx_str, ctx_len, status};
  SigAlg a;
  if (const int r = sig_args(ctx, alg, SIG_MLDSA, false, ctx_len, n, v.set(), a)) return r < 0 ? -1 : 0;
  return mldsa_verify_rows(ctx, a, n, v, MldsaTrace{mu, ctilde, w1, flags}, (hipStream_t)stream);
}

// ------------------------------------------------------------------ ML-DSA key sets (mldsa_keyed.hip)
// g keys expanded once into one device allocation of their own (not the context's scratch: a set outlives calls
// and contexts).  A secret set holds K and the NTTs of s1, s2, t0: qrk_mldsa_keyset_free zeroes it before freeing.
struct qrk_mldsa_keyset {
  int device = 0;
  int which = 0;
  bool secret = false;
  size_t g = 0;
  void* mem = nullptr;
  size_t bytes = 0;
  MldsaKeys view;
};

static int keyset_load(qrk_ctx* ctx, const char* alg, bool secret, size_t g, const uint8_t* keys,
                       qrk_mldsa_keyset** out, hipStream_t st) {
  if (!ctx) return fail("null context");
  const int which = mldsa_find(alg);
  if (which < 0) return sig_unsupported(alg);
  if (g == 0) return fail("a key set holds at least one key (g == 0)");
  if (!keys || !out) return fail("null buffer");
  const size_t per_key = mldsa_keyset_bytes(which, secret, 1);
  if (g > verify_cap(per_key))
    return fail(std::string(alg) + ": a key set of " + std::to_string(g) + " keys exceeds the scratch budget (at most " +
                std::to_string(verify_cap(per_key)) + " keys of " + std::to_string(per_key) + " bytes)");
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::TIMER)) return -1;
  qrk_mldsa_keyset* ks = new qrk_mldsa_keyset;
  ks->device = ctx->device, ks->which = which, ks->secret = secret, ks->g = g;
  ks->bytes = mldsa_keyset_bytes(which, secret, g);
  hipError_t e = hipMalloc(&ks->mem, ks->bytes);
  if (e != hipSuccess) {
    delete ks;
    return hip_fail("hipMalloc(key set)", e);
  }
  ks->view = mldsa_keyset_view(which, secret, g, ks->mem);
  e = mldsa_keyset_expand(which, secret, g, keys, ks->mem, st);
  if (e != hipSuccess) {
    qrk_mldsa_keyset_free(ks);
    return hip_fail("mldsa_keyset_expand", e);
  }
  *out = ks;
  return 0;
}

int qrk_mldsa_pubkeys_load(qrk_ctx* ctx, const char* alg, size_t g, const uint8_t* pk, qrk_mldsa_keyset** out,
                           void* stream) {
  return keyset_load(ctx, alg, false, g, pk, out, (hipStream_t)stream);
}

int qrk_mldsa_seckeys_load(qrk_ctx* ctx, const char* alg, size_t g, const uint8_t* sk, qrk_mldsa_keyset** out,
                           void* stream) {
  return keyset_load(ctx, alg, true, g, sk, out, (hipStream_t)stream);
}

int qrk_mldsa_keyset_info(const qrk_mldsa_keyset* ks, size_t out[4]) {
  if (!ks || !out) return fail(ks ? "null buffer" : "null key set");
  out[0] = ks->g, out[1] = (size_t)ks->which, out[2] = ks->secret ? 1 : 0, out[3] = ks->bytes;
  return 0;
}

void qrk_mldsa_keyset_free(qrk_mldsa_keyset* ks) {
  if (!ks) return;
  if (ks->mem) {
    DeviceGuard guard;
    if (guard.set(ks->device) == 0) {
      (void)hipDeviceSynchronize();  // no launch that reads the set is still running
      (void)hipMemset(ks->mem, 0, ks->bytes);
      (void)hipDeviceSynchronize();
      (void)hipFree(ks->mem);
    }
  }
  delete ks;
}

// The argument checks of the two keyed calls and their trace hooks, in the order qrkem.h documents.  `bufs`: no
// required pointer is null.  -1: failed, 1: n == 0, 0: go.  ctx is not dereferenced before ks is known to be set.
static int keyed_args(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, bool signing, const uint32_t* key_index, size_t ctx_len,
                      size_t n, bool bufs) {
  if (!ctx) return fail("null context");
  if (!ks) return fail("null key set");
  if (ks->device != ctx->device)
    return fail("foreign key set: it was loaded on device " + std::to_string(ks->device) + ", the context is on device " +
                std::to_string(ctx->device));
  if (signing && !ks->secret)
    return fail("foreign key set: a public key set cannot sign (load the secret keys with qrk_mldsa_seckeys_load)");
  if (!signing && ks->secret)
    return fail("foreign key set: a secret key set cannot verify (load the public keys with qrk_mldsa_pubkeys_load)");
  if (ctx_len > 255) return fail("ML-DSA context strings are at most 255 bytes");
  if (n == 0) return 1;
  if (!bufs) return fail("null buffer");
  if (!key_index && ks->g != 1)
    return fail("null buffer: key_index may be NULL only for a key set of one key");
  return 0;
}

// qrk_mldsa_verify_keyed_batch and its traced twin: one body
static int mldsa_verify_keyed_call(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                   const uint8_t* msg, const uint64_t* msg_off, const uint8_t* sig,
                                   const uint8_t* ctx_str, size_t ctx_len, int32_t* status, const MldsaTrace& trace,
                                   hipStream_t st) {
  const bool bufs = msg && msg_off && sig && status && (ctx_str || !ctx_len);
  if (const int r = keyed_args(ctx, ks, false, key_index, ctx_len, n, bufs)) return r < 0 ? -1 : 0;
  const SigSizes sz = mldsa_sizes(ks->which);
  return run_rows(ctx, st, n, verify_cap(mldsa_keyed_scratch_bytes(ks->which, 1)), mldsa_keyed_scratch_bytes, ks->which,
                  "mldsa_verify_keyed", [&](size_t off, size_t m) {
                    return mldsa_verify_keyed(ks->which, ks->view, m, key_index ? key_index + off : nullptr, msg,
                                              msg_off + off, sig + off * sz.sig, ctx_str, ctx_len, status + off,
                                              mldsa_trace_at(ks->which, trace, off), ctx->scratch, st);
                  });
}

int qrk_mldsa_verify_keyed_batch(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                 const uint8_t* msg, const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str,
                                 size_t ctx_len, int32_t* status, void* stream) {
  return mldsa_verify_keyed_call(ctx, ks, n, key_index, msg, msg_off, sig, ctx_str, ctx_len, status, MldsaTrace{},
                                 (hipStream_t)stream);
}

// test hook (qrkem_debug.h): the call above with the trace outputs
int qrk_dbg_mldsa_verify_keyed_trace(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                     const uint8_t* msg, const uint64_t* msg_off, const uint8_t* sig,
                                     const uint8_t* ctx_str, size_t ctx_len, int32_t* status, uint8_t* mu,
                                     uint8_t* ctilde, uint8_t* w1, uint32_t* flags, void* stream) {
  if (n && (!mu || !ctilde || !w1 || !flags)) return fail("null trace buffer");
  return mldsa_verify_keyed_call(ctx, ks, n, key_index, msg, msg_off, sig, ctx_str, ctx_len, status,
                                 MldsaTrace{mu, ctilde, w1, flags}, (hipStream_t)stream);
}

// qrk_mldsa_sign_keyed_batch and its traced twin qrk_dbg_mldsa_sign_keyed_trace (iters != NULL): one body
static int mldsa_sign_keyed_call(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                 const uint8_t* msg, const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str,
                                 size_t ctx_len, uint8_t* sig, int32_t* status, uint32_t max_iters, bool traced,
                                 uint8_t* mu, uint32_t* iters, hipStream_t st) {
  const bool bufs = msg && msg_off && sig && status && (ctx_str || !ctx_len) && (!traced || (mu && iters));
  if (const int r = keyed_args(ctx, ks, true, key_index, ctx_len, n, bufs)) return r < 0 ? -1 : 0;
  const SigSizes sz = mldsa_sizes(ks->which);
  return run_rows(ctx, st, n, verify_cap(mldsa_keyed_sign_scratch_bytes(ks->which, 1)), mldsa_keyed_sign_scratch_bytes,
                  ks->which, "mldsa_sign_keyed", [&](size_t off, size_t m) {
                    return mldsa_sign_keyed(ks->which, ks->view, m, key_index ? key_index + off : nullptr, msg,
                                            msg_off + off, rnd ? rnd + off * 32 : nullptr, ctx_str, ctx_len,
                                            sig + off * sz.sig, status + off, max_iters,
                                            traced ? mu + off * 64 : nullptr, traced ? iters + off : nullptr,
                                            ctx->scratch, st);
                  });
}

int qrk_mldsa_sign_keyed_batch(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                               const uint8_t* msg, const uint64_t* msg_off, const uint8_t* rnd, const uint8_t* ctx_str,
                               size_t ctx_len, uint8_t* sig, int32_t* status, void* stream) {
  return mldsa_sign_keyed_call(ctx, ks, n, key_index, msg, msg_off, rnd, ctx_str, ctx_len, sig, status,
                               MLDSA_SIGN_MAX_ITERS, false, nullptr, nullptr, (hipStream_t)stream);
}

// test hook (qrkem_debug.h): the call above with the loop's cap as an argument and the trace outputs
int qrk_dbg_mldsa_sign_keyed_trace(qrk_ctx* ctx, const qrk_mldsa_keyset* ks, size_t n, const uint32_t* key_index,
                                   const uint8_t* msg, const uint64_t* msg_off, const uint8_t* rnd,
                                   const uint8_t* ctx_str, size_t ctx_len, uint8_t* sig, int32_t* status,
                                   uint32_t max_iters, uint8_t* mu, uint32_t* iters, void* stream) {
  return mldsa_sign_keyed_call(ctx, ks, n, key_index, msg, msg_off, rnd, ctx_str, ctx_len, sig, status, max_iters, true,
                               mu, iters, (hipStream_t)stream);
}

// test and tool hook (qrkem_debug.h): which form of the keyed signing core later launches take
int qrk_dbg_mldsa_keyed_sign_mode(int mode) {
  g_mldsa_keyed_sign_mode.store(mode == 1 || mode == 2 ? mode : MLDSA_KEYED_SIGN_DEFAULT, std::memory_order_relaxed);
  return g_mldsa_keyed_sign_mode.load(std::memory_order_relaxed);
}

// test hook (qrkem_debug.h): qrk_sig_verify_batch for an SLH-DSA / SPHINCS+ name, with the trace outputs
int qrk_dbg_slhdsa_verify_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* pk, const uint8_t* msg,
                                const uint64_t* msg_off, const uint8_t* sig, const uint8_t* ctx_str, size_t ctx_len,
                                int32_t* status, uint8_t* digest, uint8_t* fors_pk, uint8_t* roots, uint32_t* flags,
                                void* stream) {
  if (n && (!digest || !fors_pk || !roots || !flags)) return fail("null trace buffer");
  const VerifyIo v{pk, msg, msg_off, sig, ctx_str, ctx_len, status};
  SigAlg a;
  if (const int r = sig_args(ctx, alg, SIG_SLHDSA, false, ctx_len, n, v.set(), a)) return r < 0 ? -1 : 0;
  return slhdsa_verify_rows(ctx, a, n, v, SlhdsaTrace{digest, fors_pk, roots, flags}, (hipStream_t)stream);
}

}  // extern "C"
