// What every abi_*.cpp shares: the context, the error channel and the opening of an ABI call.  Internal: included
// by the abi_*.cpp files only.  Definitions that are not inline here are in abi_ctx.cpp; what one file alone uses
// stays static in that file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qrkem.h"
#include "qrkem_debug.h"
#include "qrkem_internal.h"

namespace qrk {

// ------------------------------------------------------------------ errors (the thread's qrk_last_error string)
int fail(const std::string& msg);  // -1
int hip_fail(const char* what, hipError_t e);
inline int hip_done(const char* what, hipError_t e) { return e == hipSuccess ? 0 : hip_fail(what, e); }

// ------------------------------------------------------------------ kernel timing
// Pairs of HIP events recorded on the launch stream around every kernel; read
// back (after a synchronise) as per-kernel-name totals.
struct EventTimer : KernelTimer {
  struct Rec {
    const char* name;
    hipEvent_t a, b;
  };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t pending = nullptr;
  hipEvent_t take() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    // timing only: no system-scope release (an L2 writeback + invalidate per event, which cost
    // 5 % of an ML-KEM-768 2^20 bench step with one event pair per launch)
    hipEvent_t e;
    (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    return e;
  }
  void before(const char*, hipStream_t st) override {
    pending = take();
    (void)hipEventRecord(pending, st);
  }
  void after(const char* name, hipStream_t st) override {
    hipEvent_t b = take();
    (void)hipEventRecord(b, st);
    recs.push_back({name, pending, b});
    pending = nullptr;
  }
  void reset() {
    for (auto& r : recs) pool.push_back(r.a), pool.push_back(r.b);
    recs.clear();
  }
  ~EventTimer() override {
    reset();
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

}  // namespace qrk

// ------------------------------------------------------------------ context
struct qrk_ctx {
  int device = 0;
  size_t chunk = 1 << 20;
  bool profiling = false;
  qrk::EventTimer timer;
  std::vector<std::pair<std::string, std::pair<double, uint64_t>>> profile;  // name -> (ms, launches)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  size_t aead_long_part = 0;  // bytes at the start of the scratch that the last long AEAD call's segment partials took
  uint8_t* dstage = nullptr;  // device staging for host-pointer calls and generated coins
  size_t dstage_bytes = 0;
  uint8_t* hstage = nullptr;  // pinned host staging
  size_t hstage_bytes = 0;
  uint8_t* hs_scratch = nullptr;  // handshake driver: ephemeral sk / ss of one chunk
  size_t hs_scratch_bytes = 0;
  uint8_t* dio = nullptr;         // host-pointer calls: packed device inputs | outputs
  size_t dio_bytes = 0;
  uint8_t* hio = nullptr;         // ... and their pinned host mirror
  size_t hio_bytes = 0;
  uint8_t* hio_dev = nullptr;     // device mapping of hio (zero-copy small calls)
  uint32_t* hflag = nullptr;      // single-shot completion flag (fine-grained pinned) ...
  uint32_t* hflag_dev = nullptr;  // ... its device address
  qrk::mlkem::CtxState mlkem;     // what ML-KEM alone keeps between calls (qrkem_internal.h)
  uint32_t ticket = 0;            // what the last single-shot call asked its kernel to store in hflag[0]
  hipStream_t io_stream = nullptr;
  int streams = 0;            // 0: multi-role launches, 1: serial (one kernel per launch)
  hipEvent_t ev_last = nullptr;  // recorded at the end of the last call that used the scratch
  hipStream_t last_stream = nullptr;  // ... on this stream
  bool last_valid = false;
  hipEvent_t ev_up = nullptr;    // end of the OS-coin upload (run_batch)
  mutable std::mutex mu;
};

namespace qrk {

// Orders a call on `st` behind the context's last use (the rule is beside the definition, abi_ctx.cpp) ...
int ctx_order(qrk_ctx* ctx, hipStream_t st);
// ... and the host-side wait for that last use
void ctx_quiesce(qrk_ctx* ctx);
// Records the end of this call on `st` on every exit path, including early error returns.
struct LastUse {
  qrk_ctx* ctx = nullptr;  // null: not armed
  hipStream_t st = nullptr;
  ~LastUse() {
    if (ctx && hipEventRecord(ctx->ev_last, st) == hipSuccess) {
      ctx->last_valid = true;
      ctx->last_stream = st;
    }
  }
};

// Makes `device` current for the scope of one ABI call and restores the caller's current
// device on exit, so a call on a context of GPU 3 never leaves the calling thread (and the
// torch allocations that follow) switched to GPU 3.
struct DeviceGuard {
  int prev = -1;
  int set(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) return fail("no HIP device available (libqrkem has no CPU path)");
    if (device < 0 || device >= count) return fail("invalid device index");
    if (prev < 0 && hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev == device) return 0;
    e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail("hipSetDevice", e);
    return 0;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Context buffers grow, never shrink; a device buffer is zeroed before it is freed.
int grow_device(qrk_ctx* ctx, void** p, size_t* have, size_t need, hipStream_t st);
int grow_pinned(uint8_t** p, size_t* have, size_t need);
int os_random(uint8_t* out, size_t n);

// FrodoKEM scratch is 0.14-0.53 MB per handshake, HQC's 9-24 KB: their chunks are capped so
// scratch stays near QRK_SCRATCH_GIB (48 GiB of the 288 GB HBM by default: a 2^16 FrodoKEM batch in
// one chunk, so the lane-per-handshake sponge kernels get a whole wave per SIMD)
#ifndef QRK_SCRATCH_GIB
#define QRK_SCRATCH_GIB 48
#endif
inline size_t scratch_cap(size_t per_row) {
  return std::max<size_t>(4096, ((size_t)QRK_SCRATCH_GIB << 30) / per_row / 64 * 64);
}

// Equal chunks (multiples of 64) of at most `cap` handshakes rather than full chunks plus a small tail.
inline size_t chunk_plan(size_t n, size_t cap) {
  const size_t nchunks = (n + cap - 1) / cap;
  return std::min(cap, round64((n + nchunks - 1) / nchunks));
}

// Routes QRK_LAUNCH timing to a timer (or to none) from set() to the end of the scope (nests).
struct TimerScope {
  KernelTimer* prev = g_timer;
  void set(KernelTimer* t) { g_timer = t; }
  ~TimerScope() { g_timer = prev; }
};

// The opening of every ABI call that launches, after its argument checks: the context lock, the
// context's device current, the call ordered behind the context's last use and recorded as the new
// one, kernel timing routed to the context's timer, the launch-error channel cleared -- in this
// order, undone in reverse on every exit path.  An entry point names the parts it takes:
//   LOCK   it is the outermost call on the context (run_batch runs under its caller's lock)
//   ORDER  it reads or writes a buffer the context owns (scratch, staging)
//   TIMER  its kernels count in the context's profile (qrk_ctx_profile)
// and every one gets launch_begin(), so its launchers' return value is its answer.
struct CallScope {
  enum : unsigned { LOCK = 1, ORDER = 2, TIMER = 4 };
  std::unique_lock<std::mutex> lk;
  DeviceGuard device_guard;
  LastUse last_use;
  TimerScope timer_scope;
  int open(qrk_ctx* ctx, hipStream_t st, unsigned parts) {
    if (parts & LOCK) lk = std::unique_lock<std::mutex>(ctx->mu);
    if (device_guard.set(ctx->device)) return -1;
    if (parts & ORDER) {
      if (ctx_order(ctx, st)) return -1;
      last_use.ctx = ctx, last_use.st = st;
    }
    if (parts & TIMER) timer_scope.set(ctx->profiling ? &ctx->timer : nullptr);
    launch_begin();
    return 0;
  }
};
// ... and of a hook that reads a context's buffers back: the previous call's device work complete
int open_inspect(CallScope& scope, qrk_ctx* ctx, bool args_ok);

// Zeroes the device staging copy of OS-drawn bytes when the call returns (coins are
// the KeyGen seeds / Encaps messages, i.e. enough to rebuild the keys), stream-ordered after the
// kernels that read it.  The pinned host copy is wiped as soon as its upload has completed.
struct CoinWipe {
  qrk_ctx* ctx;
  hipStream_t st;
  size_t bytes = 0;
  ~CoinWipe() {
    if (bytes) (void)hipMemsetAsync(ctx->dstage, 0, bytes, st);
  }
};
// `bytes` from the OS CSPRNG in the context's device staging (NULL: failed), for a call on `st` that holds `wipe`
const uint8_t* stage_os_random(qrk_ctx* ctx, size_t bytes, hipStream_t st, CoinWipe& wipe);

// The row driver of the signature calls (outermost: it takes the lock): n > 0 rows through a launcher that uses the
// context's scratch (public values only: no cleanse), in equal chunks of at most min(qrk_ctx_set_chunk, cap) rows.
// launch(off, m) runs rows [off, off + m); the first failing chunk's status is the call's error, named `what`.
template <class Launch>
int run_rows(qrk_ctx* ctx, hipStream_t st, size_t n, size_t cap, size_t (*scratch_bytes)(int, size_t), int which,
             const char* what, Launch launch) {
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  const size_t chunk = chunk_plan(n, std::min(ctx->chunk, cap));
  if (grow_device(ctx, &ctx->scratch, &ctx->scratch_bytes, scratch_bytes(which, chunk), st)) return -1;
  for (size_t off = 0; off < n; off += chunk) {
    launch_begin();
    const hipError_t e = launch(off, std::min(chunk, n - off));
    if (e != hipSuccess) return hip_fail(what, e);
  }
  return 0;
}

// A hook's read-back of what a call left behind: *acc = fold(*acc, x) over a host copy of the `bytes` bytes at
// the device pointer `src`.  The copy may hold key material, so it is cleansed before the heap gets it back;
// the copy's own failure is the hook's error, named `what`.
typedef uint64_t (*ResidueFold)(uint64_t acc, uint8_t x);
inline uint64_t count_nonzero(uint64_t acc, uint8_t x) { return acc + (x != 0); }
int read_residue(const void* src, size_t bytes, ResidueFold fold, const char* what, uint64_t* acc);

}  // namespace qrk
