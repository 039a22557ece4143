// The context of the batched API (include/qrkem.h, Part 2): its lifetime, its settings, its profile, and the
// definitions behind abi_ctx.h.  The API areas are in abi_kem.cpp, abi_aead.cpp, abi_sig.cpp and abi_util.cpp.
#include "abi_ctx.h"

#include <sys/random.h>

namespace qrk {

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}
int hip_fail(const char* what, hipError_t e) {
  return fail(std::string(what) + ": " + hipGetErrorString(e));
}

// ------------------------------------------------------------------ kernel timing
thread_local KernelTimer* g_timer = nullptr;
thread_local hipError_t g_launch_err{hipSuccess};
std::atomic<int> g_dbg_fail_launch{0};

// Calls that use a context's scratch are ordered one after another whatever stream each runs
// on: the new call's stream waits, on the device, on the event the previous call recorded at its
// end.  (A device-pointer call on the caller's stream followed by a host-pointer call on the
// context's own I/O stream would otherwise let the second overwrite scratch the first is still
// reading.)  This is the only cross-stream dependency of the library: every kernel of one call
// runs on that call's stream, so a device-pointer call never blocks the host.
int ctx_order(qrk_ctx* ctx, hipStream_t st) {
  if (!ctx->ev_last) {
    hipError_t e = hipEventCreateWithFlags(&ctx->ev_last, hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail("hipEventCreate(last use)", e);
  }
  if (ctx->last_valid && ctx->last_stream != st) {  // same stream: already in order
    hipError_t e = hipStreamWaitEvent(st, ctx->ev_last, 0);
    if (e != hipSuccess) return hip_fail("hipStreamWaitEvent(last use)", e);
  }
  return 0;
}
// Host-side wait for the previous call's device work (before freeing or refilling buffers it reads).
void ctx_quiesce(qrk_ctx* ctx) {
  if (ctx->last_valid) (void)hipEventSynchronize(ctx->ev_last);
}

int grow_device(qrk_ctx* ctx, void** p, size_t* have, size_t need, hipStream_t st) {
  if (*have >= need) return 0;
  if (*p) {
    ctx_quiesce(ctx);
    (void)hipStreamSynchronize(st);
    (void)hipMemset(*p, 0, *have);  // the old buffer may hold secret intermediates
    (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
  }
  hipError_t e = hipMalloc(p, need);
  if (e != hipSuccess) return hip_fail("hipMalloc", e);
  *have = need;
  return 0;
}

int grow_pinned(uint8_t** p, size_t* have, size_t need) {
  if (*have >= need) return 0;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *have = 0;
  hipError_t e = hipHostMalloc((void**)p, need, hipHostMallocDefault);
  if (e != hipSuccess) return hip_fail("hipHostMalloc", e);
  *have = need;
  return 0;
}

int os_random(uint8_t* out, size_t n) {
  while (n) {
    ssize_t r = getrandom(out, n, 0);
    if (r < 0) return fail("getrandom failed");
    out += r;
    n -= (size_t)r;
  }
  return 0;
}

// The opening of a hook that reads a context's buffers back: the previous call's device work complete
int open_inspect(CallScope& scope, qrk_ctx* ctx, bool args_ok) {
  if (!ctx || !args_ok) return fail("null argument");
  if (scope.open(ctx, nullptr, CallScope::LOCK)) return -1;
  ctx_quiesce(ctx);
  return 0;
}

// `bytes` from the OS CSPRNG in the context's device staging (NULL: failed), for a call on `st`
// that holds `wipe`.  The one host wait of the device-pointer API: the pinned copy is wiped as soon
// as it has reached the device, so the call returns after the upload (which the stream orders behind
// its earlier work), not after the kernels.
const uint8_t* stage_os_random(qrk_ctx* ctx, size_t bytes, hipStream_t st, CoinWipe& wipe) {
  if (grow_pinned(&ctx->hstage, &ctx->hstage_bytes, bytes)) return nullptr;
  if (grow_device(ctx, (void**)&ctx->dstage, &ctx->dstage_bytes, bytes, st)) return nullptr;
  hipError_t e = ctx->ev_up ? hipSuccess : hipEventCreateWithFlags(&ctx->ev_up, hipEventDisableTiming);
  if (e != hipSuccess) return hip_fail("hipEventCreate(upload)", e), nullptr;
  if (os_random(ctx->hstage, bytes)) return nullptr;
  wipe.bytes = bytes;
  e = hipMemcpyAsync(ctx->dstage, ctx->hstage, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev_up, st);
  if (e == hipSuccess) e = hipEventSynchronize(ctx->ev_up);
  OQS_MEM_cleanse(ctx->hstage, bytes);
  if (e != hipSuccess) return hip_fail("hipMemcpyAsync(OS random bytes)", e), nullptr;
  return ctx->dstage;
}

int read_residue(const void* src, size_t bytes, ResidueFold fold, const char* what, uint64_t* acc) {
  std::vector<uint8_t> tmp(bytes);
  const hipError_t e = hipMemcpy(tmp.data(), src, bytes, hipMemcpyDeviceToHost);
  for (uint8_t x : tmp) *acc = fold(*acc, x);
  // the copy may hold expanded key material (PRF / CBD output, FrodoKEM S, HQC x, y): wipe it
  // before the heap gets it back
  OQS_MEM_cleanse(tmp.data(), tmp.size());
  return hip_done(what, e);
}

}  // namespace qrk

using namespace qrk;

extern "C" {

int qrk_ctx_create(qrk_ctx** out, int device) {
  if (!out) return fail("null out");
  *out = nullptr;
  DeviceGuard device_guard;
  if (device_guard.set(device)) return -1;
  qrk_ctx* c = new qrk_ctx();
  c->device = device;
  *out = c;
  return 0;
}

// Every buffer of the context that can hold keys or secret intermediates (device scratch, handshake
// scratch, device and pinned host staging) set to `byte` over its full current size.  Synchronous.
// The one list of those buffers: cleanse_all (byte 0) and the test hook qrk_dbg_ctx_fill walk it.
// What a call relies on from one call to the next is not in it: the ML-KEM CtxState words, hflag,
// preloaded key sets (they own their memory), and the sizes, aead_long_part among them.  The ML-KEM kept
// region (public data) is in it, and is invalid from here: no later Decaps reads what this wrote there.
static hipError_t fill_all(qrk_ctx* ctx, int byte) {
  ctx_quiesce(ctx);
  void* keep = nullptr;
  size_t keep_bytes = 0;
  ctx->mlkem.keep_invalidate(&keep, &keep_bytes);
  void* const dev[] = {ctx->scratch, ctx->hs_scratch, ctx->dio, ctx->dstage, keep};
  const size_t dev_bytes[] = {ctx->scratch_bytes, ctx->hs_scratch_bytes, ctx->dio_bytes, ctx->dstage_bytes, keep_bytes};
  uint8_t* const pinned[] = {ctx->hio, ctx->hstage};
  const size_t pinned_bytes[] = {ctx->hio_bytes, ctx->hstage_bytes};
  hipError_t first = hipSuccess;
  for (int i = 0; i < 5; ++i) {
    if (!dev[i]) continue;
    const hipError_t e = hipMemset(dev[i], byte, dev_bytes[i]);
    if (first == hipSuccess) first = e;
  }
  const hipError_t e = hipDeviceSynchronize();
  if (first == hipSuccess) first = e;
  for (int i = 0; i < 2; ++i) {
    if (!pinned[i]) continue;
    if (byte == 0) {
      OQS_MEM_cleanse(pinned[i], pinned_bytes[i]);
    } else {
      memset(pinned[i], byte, pinned_bytes[i]);
    }
  }
  return first;
}
static void cleanse_all(qrk_ctx* ctx) { (void)fill_all(ctx, 0); }

int qrk_ctx_cleanse(qrk_ctx* ctx) {
  if (!ctx) return fail("null context");
  CallScope scope;
  if (scope.open(ctx, nullptr, CallScope::LOCK)) return -1;
  cleanse_all(ctx);
  return 0;
}

void qrk_ctx_destroy(qrk_ctx* ctx) {
  if (!ctx) return;
  DeviceGuard device_guard;
  if (device_guard.set(ctx->device) == 0) {
    (void)hipDeviceSynchronize();
    cleanse_all(ctx);
  }
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->hs_scratch) (void)hipFree(ctx->hs_scratch);
  if (ctx->dio) (void)hipFree(ctx->dio);
  if (ctx->hio) (void)hipHostFree(ctx->hio);
  if (ctx->hflag) (void)hipHostFree(ctx->hflag);
  if (ctx->io_stream) (void)hipStreamDestroy(ctx->io_stream);
  if (ctx->dstage) (void)hipFree(ctx->dstage);
  if (ctx->hstage) (void)hipHostFree(ctx->hstage);
  ctx->mlkem.free();
  if (ctx->ev_up) (void)hipEventDestroy(ctx->ev_up);
  if (ctx->ev_last) (void)hipEventDestroy(ctx->ev_last);
  delete ctx;
}

int qrk_ctx_set_streams(qrk_ctx* ctx, int streams) {
  if (!ctx || streams < 0 || streams > 1) return fail("streams must be 0 (auto) or 1 (serial)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->streams = streams;
  return 0;
}

int qrk_ctx_set_chunk(qrk_ctx* ctx, size_t chunk) {
  if (!ctx || chunk == 0) return fail("bad chunk");
  std::lock_guard<std::mutex> lk(ctx->mu);  // chunk_for reads it under the lock
  ctx->chunk = round64(chunk);
  return 0;
}

size_t qrk_ctx_scratch_bytes(const qrk_ctx* ctx) { return ctx ? ctx->scratch_bytes : 0; }

int qrk_ctx_staging_residue(qrk_ctx* ctx, uint64_t out[3]) {
  CallScope scope;
  if (open_inspect(scope, ctx, out)) return -1;
  out[0] = out[1] = out[2] = 0;
  for (size_t i = 0; i < ctx->hstage_bytes; ++i) out[0] += ctx->hstage[i] != 0;
  const void* src[2] = {ctx->dstage, ctx->scratch};
  const size_t len[2] = {ctx->dstage_bytes, std::min<size_t>(ctx->scratch_bytes, (size_t)64 << 20)};
  for (int b = 0; b < 2; ++b) {
    if (!len[b]) continue;
    if (read_residue(src[b], len[b], count_nonzero, "hipMemcpy(staging residue)", &out[1 + b])) return -1;
  }
  return 0;
}

// ---- test hooks: declared and documented in qrkem_debug.h, not in qrkem.h
int qrk_dbg_kg_late(int role) {
  g_kg_dbg_late.store(role, std::memory_order_relaxed);
  return 0;
}

int qrk_dbg_fail_launch(int on) {
  g_dbg_fail_launch.store(on, std::memory_order_relaxed);
  return 0;
}

int qrk_dbg_ctx_fill(qrk_ctx* ctx, int byte) {
  CallScope scope;
  if (open_inspect(scope, ctx, byte >= 0 && byte <= 255)) return -1;
  return hip_done("hipMemset(context fill)", fill_all(ctx, byte));
}

int qrk_dbg_fail_after_flip(int on) {
  g_dbg_fail_after_flip.store(on, std::memory_order_relaxed);
  return 0;
}

int qrk_ctx_profile(qrk_ctx* ctx, int enable) {
  if (!ctx) return fail("null context");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->timer.reset();
  ctx->profile.clear();
  ctx->profiling = enable != 0;
  return 0;
}

int qrk_ctx_profile_collect(qrk_ctx* ctx) {
  if (!ctx) return fail("null context");
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (auto& r : ctx->timer.recs) {
    hipError_t e = hipEventSynchronize(r.b);
    if (e != hipSuccess) return hip_fail("hipEventSynchronize", e);
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e != hipSuccess) return hip_fail("hipEventElapsedTime", e);
    auto it = std::find_if(ctx->profile.begin(), ctx->profile.end(),
                           [&](const auto& p) { return p.first == r.name; });
    if (it == ctx->profile.end()) {
      ctx->profile.push_back({r.name, {ms, 1}});
    } else {
      it->second.first += ms;
      it->second.second += 1;
    }
  }
  ctx->timer.reset();
  return (int)ctx->profile.size();
}

int qrk_ctx_profile_get(qrk_ctx* ctx, int i, const char** name, double* total_ms, uint64_t* launches) {
  if (!ctx || i < 0 || i >= (int)ctx->profile.size()) return fail("profile index out of range");
  *name = ctx->profile[i].first.c_str();
  *total_ms = ctx->profile[i].second.first;
  *launches = ctx->profile[i].second.second;
  return 0;
}

const char* qrk_last_error(void) { return g_err.c_str(); }

int qrk_device_count(void) {
  int c = 0;
  return hipGetDeviceCount(&c) == hipSuccess ? c : 0;
}

}  // extern "C"
