// C ABI of libqrkem.so, Part 2b: FrodoKEM key sets (declared in include/qrkem.h; kernels in frodo_keyed.cuh).  The
// contract of the ML-KEM key sets (abi_kem_keyed.cpp) wherever it applies: g keys expanded once into a device
// allocation of their own, and Encaps / Decaps of n rows that name their key by index, chunked like qrk_kem_*_batch.
#include "abi_ctx.h"

using namespace qrk;

struct qrk_frodo_keyset {
  int device = 0;
  const AlgInfo* alg = nullptr;
  bool secret = false;
  size_t g = 0;
  void* mem = nullptr;
  size_t bytes = 0;
  FrodoKeys view;
};

// the six FrodoKEM names; any other name is refused, an ML-KEM or HQC one by name
static const AlgInfo* keyed_alg(const char* alg) {
  const AlgInfo* a = find_alg(alg);
  if (a && a->family == Family::FRODO && a->enabled) return a;
  if (a)
    fail(std::string("these key sets are FrodoKEM only: ") + alg +
         (a->family == Family::MLKEM ? " has its own (qrk_mlkem_pubkeys_load / qrk_mlkem_seckeys_load)"
                                     : " has none (use qrk_kem_encaps_batch / qrk_kem_decaps_batch)"));
  else
    fail(std::string("unsupported KEM: ") + (alg ? alg : "(null)"));
  return nullptr;
}

static size_t set_index(const AlgInfo& a) { return (a.k == 640 ? 0 : a.k == 976 ? 2 : 4) + (a.aes ? 1 : 0); }

static size_t keyed_chunk(const qrk_ctx* ctx, const AlgInfo& a) {
  return std::min(ctx->chunk, scratch_cap(frodo_keyed_scratch_bytes(a, 1024, 1) / 1024 + 1));
}

static int keyset_load(qrk_ctx* ctx, const char* alg, bool secret, size_t g, const uint8_t* keys,
                       qrk_frodo_keyset** out, hipStream_t st) {
  if (!ctx) return fail("null context");
  const AlgInfo* a = keyed_alg(alg);
  if (!a) return -1;
  if (g == 0) return fail("a key set holds at least one key (g == 0)");
  if (!keys || !out) return fail("null buffer");
  const size_t per_key = frodo_keyset_bytes(*a, secret, 64) / 64;
  const size_t cap = std::min<size_t>(scratch_cap(per_key), 0xFFFFFFFFu);
  if (g > cap)
    return fail(std::string(alg) + ": a key set of " + std::to_string(g) + " keys exceeds the scratch budget (at most " +
                std::to_string(cap) + " keys of " + std::to_string(per_key) + " bytes)");
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::TIMER)) return -1;
  qrk_frodo_keyset* ks = new qrk_frodo_keyset;
  ks->device = ctx->device, ks->alg = a, ks->secret = secret, ks->g = g;
  ks->bytes = frodo_keyset_bytes(*a, secret, g);
  hipError_t e = hipMalloc(&ks->mem, ks->bytes);
  if (e != hipSuccess) {
    delete ks;
    (void)hipGetLastError();
    return fail(std::string(alg) + ": cannot allocate a key set of " + std::to_string(g) + " keys (" +
                std::to_string(frodo_keyset_bytes(*a, secret, g)) + " bytes): " + hipGetErrorString(e));
  }
  ks->view = frodo_keyset_view(*a, secret, g, ks->mem);
  e = frodo_keyset_expand(*a, secret, g, keys, ks->mem, st);
  if (e != hipSuccess) {
    qrk_frodo_keyset_free(ks);
    return hip_fail("frodo_keyset_expand", e);
  }
  *out = ks;
  return 0;
}

// The argument checks of the keyed calls, in the order qrkem.h documents.  -1: failed, 1: n == 0, 0: go.
// ctx is not dereferenced before ks is known to be set.
static int keyed_args(qrk_ctx* ctx, const qrk_frodo_keyset* ks, bool decaps, const uint32_t* key_index, size_t n,
                      bool bufs) {
  if (!ctx) return fail("null context");
  if (!ks) return fail("null key set");
  if (ks->device != ctx->device)
    return fail("foreign key set: it was loaded on device " + std::to_string(ks->device) + ", the context is on device " +
                std::to_string(ctx->device));
  if (decaps && !ks->secret)
    return fail("foreign key set: a public key set cannot decapsulate (load the secret keys with qrk_frodo_seckeys_load)");
  if (!decaps && ks->secret)
    return fail("foreign key set: a secret key set cannot encapsulate (load the public keys with qrk_frodo_pubkeys_load)");
  if (n == 0) return 1;
  if (!bufs) return fail("null buffer");
  if (!key_index && ks->g != 1) return fail("null buffer: key_index may be NULL only for a key set of one key");
  return 0;
}

// n > 0 rows in equal chunks of at most the context's chunk; the records of a chunk are zeroed behind it
template <class Launch>
static int keyed_rows(qrk_ctx* ctx, const qrk_frodo_keyset* ks, hipStream_t st, size_t n, const uint8_t** os_coins,
                      const char* what, Launch launch) {
  const AlgInfo& a = *ks->alg;
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  const size_t chunk = chunk_plan(n, keyed_chunk(ctx, a));
  if (grow_device(ctx, &ctx->scratch, &ctx->scratch_bytes, frodo_keyed_scratch_bytes(a, chunk, ks->g), st)) return -1;
  // OS coins are Encaps messages: both staged copies are wiped on every exit path (declared after the scope, so
  // the device wipe is queued before the call's end event)
  CoinWipe coin_wipe{ctx, st};
  if (os_coins) {
    *os_coins = stage_os_random(ctx, n * a.enc_coins, st, coin_wipe);
    if (!*os_coins) return -1;
  }
  Streams S;
  S.main = st;
  S.serial = ctx->streams == 1;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = std::min(chunk, n - off);
    launch_begin();
    hipError_t e = launch(off, m, S);
    if (e != hipSuccess) return hip_fail(what, e);
    e = frodo_keyed_cleanse(a, m, ks->g, ctx->scratch, st);
    if (e != hipSuccess) return hip_fail("hipMemsetAsync(cleanse)", e);
  }
  return 0;
}

extern "C" {

int qrk_frodo_pubkeys_load(qrk_ctx* ctx, const char* alg, size_t g, const uint8_t* pk, qrk_frodo_keyset** out,
                           void* stream) {
  return keyset_load(ctx, alg, false, g, pk, out, (hipStream_t)stream);
}

int qrk_frodo_seckeys_load(qrk_ctx* ctx, const char* alg, size_t g, const uint8_t* sk, qrk_frodo_keyset** out,
                           void* stream) {
  return keyset_load(ctx, alg, true, g, sk, out, (hipStream_t)stream);
}

int qrk_frodo_keyset_info(const qrk_frodo_keyset* ks, size_t out[4]) {
  if (!ks || !out) return fail(ks ? "null buffer" : "null key set");
  out[0] = ks->g, out[1] = set_index(*ks->alg), out[2] = ks->secret ? 1 : 0, out[3] = ks->bytes;
  return 0;
}

void qrk_frodo_keyset_free(qrk_frodo_keyset* ks) {
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

int qrk_frodo_encaps_keyed_batch(qrk_ctx* ctx, const qrk_frodo_keyset* ks, size_t n, const uint32_t* key_index,
                                 uint8_t* ct, uint8_t* ss, const uint8_t* coins, int32_t* status, void* stream) {
  if (const int r = keyed_args(ctx, ks, false, key_index, n, ct && ss)) return r < 0 ? -1 : 0;
  const AlgInfo& a = *ks->alg;
  return keyed_rows(ctx, ks, (hipStream_t)stream, n, coins ? nullptr : &coins, "frodo_encaps_keyed",
                    [&](size_t off, size_t m, const Streams& S) {
                      return frodo_encaps_keyed(a, ks->view, m, key_index ? key_index + off : nullptr, ct + off * a.ct,
                                                ss + off * a.ss, coins + off * a.enc_coins,
                                                status ? status + off : nullptr, ctx->scratch, S);
                    });
}

int qrk_frodo_decaps_keyed_batch(qrk_ctx* ctx, const qrk_frodo_keyset* ks, size_t n, const uint32_t* key_index,
                                 uint8_t* ss, const uint8_t* ct, int32_t* status, void* stream) {
  if (const int r = keyed_args(ctx, ks, true, key_index, n, ss && ct)) return r < 0 ? -1 : 0;
  const AlgInfo& a = *ks->alg;
  return keyed_rows(ctx, ks, (hipStream_t)stream, n, nullptr, "frodo_decaps_keyed",
                    [&](size_t off, size_t m, const Streams& S) {
                      return frodo_decaps_keyed(a, ks->view, m, key_index ? key_index + off : nullptr, ss + off * a.ss,
                                                ct + off * a.ct, status ? status + off : nullptr, ctx->scratch, S);
                    });
}

}  // extern "C"
