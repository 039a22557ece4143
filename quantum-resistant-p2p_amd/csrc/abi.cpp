// C ABI of libqrkem.so (declared in include/qrkem.h).
//
// Part 1 mirrors the liboqs entry points bound by the reference's ctypes
// wrapper (quantum_resistant_p2p/vendor/oqs.py:192-198, 271, 318, 348, 372,
// 386-390, 397, 406-411); each single-shot call is a batch of one on the GPU.
// Part 2 is the batched device API.  There is no CPU fallback: with no HIP
// device every KEM call returns OQS_ERROR and qrk_last_error() says why.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qrkem.h"
#include "qrkem_debug.h"
#include "qrkem_internal.h"

// -DQRK_HOST_TRACE=1 (tools/build_variant.sh builds only): steady-clock stamps at the phases of a
// single-shot call, read by qrk_dbg_host_trace (tools/host_trace.py)
#ifndef QRK_HOST_TRACE
#define QRK_HOST_TRACE 0
#endif
#if QRK_HOST_TRACE
static long long g_host_trace[16];
#define HT(i) (g_host_trace[i] = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count())
int qrk_dbg_host_trace(long long* out) {
  memcpy(out, g_host_trace, sizeof(g_host_trace));
  return 0;
}
#else
#define HT(i) ((void)0)
#endif

namespace qrk {

// ------------------------------------------------------------------ algorithm table
static AlgInfo ALGS[] = {
    // name, family, level, k/n, pk, sk, ct, ss, kp coins, enc coins, aes, enabled
    {"ML-KEM-512", Family::MLKEM, 1, 2, 800, 1632, 768, 32, 64, 32, false, true},
    {"ML-KEM-768", Family::MLKEM, 3, 3, 1184, 2400, 1088, 32, 64, 32, false, true},
    {"ML-KEM-1024", Family::MLKEM, 5, 4, 1568, 3168, 1568, 32, 64, 32, false, true},
    {"FrodoKEM-640-AES", Family::FRODO, 1, 640, 9616, 19888, 9720, 16, 48, 16, true, true},
    {"FrodoKEM-640-SHAKE", Family::FRODO, 1, 640, 9616, 19888, 9720, 16, 48, 16, false, true},
    {"FrodoKEM-976-AES", Family::FRODO, 3, 976, 15632, 31296, 15744, 24, 64, 24, true, true},
    {"FrodoKEM-976-SHAKE", Family::FRODO, 3, 976, 15632, 31296, 15744, 24, 64, 24, false, true},
    {"FrodoKEM-1344-AES", Family::FRODO, 5, 1344, 21520, 43088, 21632, 32, 80, 32, true, true},
    {"FrodoKEM-1344-SHAKE", Family::FRODO, 5, 1344, 21520, 43088, 21632, 32, 80, 32, false, true},
    {"HQC-128", Family::HQC, 1, 128, 2249, 2305, 4433, 64, 96, 32, false, true},
    {"HQC-192", Family::HQC, 3, 192, 4522, 4586, 8978, 64, 104, 40, false, true},
    {"HQC-256", Family::HQC, 5, 256, 7245, 7317, 14421, 64, 112, 48, false, true},
};
static const int NALG = (int)(sizeof(ALGS) / sizeof(ALGS[0]));

const AlgInfo* find_alg(const char* name) {
  if (!name) return nullptr;
  for (int i = 0; i < NALG; ++i)
    if (!strcmp(ALGS[i].name, name)) return &ALGS[i];
  return nullptr;
}

// Everything the driver needs to know about a family, indexed by Family.  A launcher whose
// `sets_status` flag is false never touches `status`: run_batch zeroes it before the launch.
struct FamilyOps {
  size_t (*scratch_bytes)(const AlgInfo&, size_t chunk);
  hipError_t (*cleanse)(const AlgInfo&, size_t n, void* scratch, hipStream_t);
  hipError_t (*keypair)(const AlgInfo&, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                        const Streams&);
  hipError_t (*encaps)(const AlgInfo&, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                       int32_t* status, void* scratch, const Streams&);
  hipError_t (*decaps)(const AlgInfo&, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, int32_t* status,
                       void* scratch, const Streams&);
  bool encaps_sets_status, decaps_sets_status;  // the kernels write every status word themselves
  const char* alg_version;
};
static const FamilyOps FAMILIES[] = {
    // ML-KEM decapsulation rejects implicitly; FrodoKEM and HQC encapsulation have no public-key check
    {mlkem_scratch_bytes, mlkem_cleanse, mlkem_keypair, mlkem_encaps, mlkem_decaps, true, false,
     "FIPS203 (qrkem gfx950)"},
    {frodo_scratch_bytes, frodo_cleanse, frodo_keypair, frodo_encaps, frodo_decaps, false, false,
     "FrodoKEM round 3 (qrkem gfx950)"},
    {hqc_scratch_bytes, hqc_cleanse, hqc_keypair, hqc_encaps, hqc_decaps, false, true,
     "HQC 2023-04-30 (qrkem gfx950)"},
};
static_assert((int)Family::MLKEM == 0 && (int)Family::FRODO == 1 && (int)Family::HQC == 2, "FAMILIES order");
static const FamilyOps& ops_of(const AlgInfo& a) { return FAMILIES[(int)a.family]; }

}  // namespace qrk

using namespace qrk;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}
static int hip_fail(const char* what, hipError_t e) {
  return fail(std::string(what) + ": " + hipGetErrorString(e));
}

// ------------------------------------------------------------------ kernel timing
namespace qrk {
thread_local KernelTimer* g_timer = nullptr;
thread_local hipError_t g_launch_err{hipSuccess};
std::atomic<int> g_dbg_fail_launch{0};
}

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

// ------------------------------------------------------------------ context
struct qrk_ctx {
  int device = 0;
  size_t chunk = 1 << 20;
  bool profiling = false;
  EventTimer timer;
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
  mlkem::CtxState mlkem;          // what ML-KEM alone keeps between calls (qrkem_internal.h)
  uint32_t ticket = 0;            // what the last single-shot call asked its kernel to store in hflag[0]
  hipStream_t io_stream = nullptr;
  int streams = 0;            // 0: multi-role launches, 1: serial (one kernel per launch)
  hipEvent_t ev_last = nullptr;  // recorded at the end of the last call that used the scratch
  hipStream_t last_stream = nullptr;  // ... on this stream
  bool last_valid = false;
  hipEvent_t ev_up = nullptr;    // end of the OS-coin upload (run_batch)
  mutable std::mutex mu;
};

// Calls that use a context's scratch are ordered one after another whatever stream each runs
// on: the new call's stream waits, on the device, on the event the previous call recorded at its
// end.  (A device-pointer call on the caller's stream followed by a host-pointer call on the
// context's own I/O stream would otherwise let the second overwrite scratch the first is still
// reading.)  This is the only cross-stream dependency of the library: every kernel of one call
// runs on that call's stream, so a device-pointer call never blocks the host.
static int ctx_order(qrk_ctx* ctx, hipStream_t st) {
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
static void ctx_quiesce(qrk_ctx* ctx) {
  if (ctx->last_valid) (void)hipEventSynchronize(ctx->ev_last);
}
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

static int grow_device(qrk_ctx* ctx, void** p, size_t* have, size_t need, hipStream_t st) {
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

static int grow_pinned(uint8_t** p, size_t* have, size_t need) {
  if (*have >= need) return 0;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *have = 0;
  hipError_t e = hipHostMalloc((void**)p, need, hipHostMallocDefault);
  if (e != hipSuccess) return hip_fail("hipHostMalloc", e);
  *have = need;
  return 0;
}


static int os_random(uint8_t* out, size_t n) {
  while (n) {
    ssize_t r = getrandom(out, n, 0);
    if (r < 0) return fail("getrandom failed");
    out += r;
    n -= (size_t)r;
  }
  return 0;
}

static const AlgInfo* resolve(const char* alg) {
  const AlgInfo* a = find_alg(alg);
  if (a && a->enabled) return a;
  fail(std::string(a ? "KEM not enabled in this build: " : "unsupported KEM: ") + (alg ? alg : "(null)"));
  return nullptr;
}

// What one caller asks of one run_batch call beyond the batch itself.  Each option takes effect
// only where run_batch says so; the public device-pointer entry points pass none.
struct CallOpts {
  bool flag = false;                  // single-shot: the kernel stores ctx->ticket in the completion flag ...
  const uint8_t* host_in1 = nullptr;  // ... and may take the public input's host copy as a by-value argument
  bool kg_err = false;                // ML-KEM KeyGen: hand the launch the error word, hflag[1]
  uint64_t* xof_keep = nullptr;       // Streams::xof_keep (KeyGen) / xof_given (Decaps): the handshake
  const uint64_t* xof_given = nullptr;  // driver's A_hat hand-over
  uint8_t* frodo_mu = nullptr;        // FrodoKEM Decaps (tests): mu' [n][32], copied out before each chunk's cleanse
};

// FrodoKEM scratch is 0.14-0.53 MB per handshake, HQC's 9-24 KB: their chunks are capped so
// scratch stays near QRK_SCRATCH_GIB (48 GiB of the 288 GB HBM by default: a 2^16 FrodoKEM batch in
// one chunk, so the lane-per-handshake sponge kernels get a whole wave per SIMD)
#ifndef QRK_SCRATCH_GIB
#define QRK_SCRATCH_GIB 48
#endif
static size_t scratch_cap(size_t per_row) {
  return std::max<size_t>(4096, ((size_t)QRK_SCRATCH_GIB << 30) / per_row / 64 * 64);
}
static size_t chunk_for(const qrk_ctx* ctx, const AlgInfo& a) {
  if (a.family == Family::MLKEM) return ctx->chunk;
  return std::min(ctx->chunk, scratch_cap(ops_of(a).scratch_bytes(a, 1024) / 1024 + 1));
}

// Equal chunks (multiples of 64) of at most `cap` handshakes rather than full chunks plus a small tail.
static size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }
static size_t chunk_plan(size_t n, size_t cap) {
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
static int open_inspect(CallScope& scope, qrk_ctx* ctx, bool args_ok) {
  if (!ctx || !args_ok) return fail("null argument");
  if (scope.open(ctx, nullptr, CallScope::LOCK)) return -1;
  ctx_quiesce(ctx);
  return 0;
}

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
// `bytes` from the OS CSPRNG in the context's device staging (NULL: failed), for a call on `st`
// that holds `wipe`.  The one host wait of the device-pointer API: the pinned copy is wiped as soon
// as it has reached the device, so the call returns after the upload (which the stream orders behind
// its earlier work), not after the kernels.
static const uint8_t* stage_os_random(qrk_ctx* ctx, size_t bytes, hipStream_t st, CoinWipe& wipe) {
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

// Core batched driver over device pointers, chunked.
static int run_batch(qrk_ctx* ctx, const AlgInfo& a, Op op, size_t n, uint8_t* o1, uint8_t* o2, const uint8_t* i1,
                     const uint8_t* i2, int32_t* status, hipStream_t st, const CallOpts& opts) {
  if (n == 0) return 0;
  const FamilyOps& f = ops_of(a);
  CallScope scope;  // the caller holds the lock
  if (scope.open(ctx, st, CallScope::ORDER | CallScope::TIMER)) return -1;
  const size_t chunk = chunk_plan(n, chunk_for(ctx, a));
  if (grow_device(ctx, &ctx->scratch, &ctx->scratch_bytes, f.scratch_bytes(a, chunk), st)) return -1;
  // coins: NULL -> OS CSPRNG, uploaded to device staging
  const uint8_t* coins = (op == Op::KEYPAIR) ? i1 : (op == Op::ENCAPS ? i2 : nullptr);
  const size_t clen = (op == Op::KEYPAIR) ? a.kp_coins : a.enc_coins;
  // OS coins are KeyGen seeds / Encaps messages: wipe both staged copies on every exit path
  // (declared after the scope, so the device wipe is queued before the call's end event)
  CoinWipe coin_wipe{ctx, st};
  if (op != Op::DECAPS && coins == nullptr) {
    coins = stage_os_random(ctx, n * clen, st, coin_wipe);
    if (!coins) return -1;
  }
  Streams S;
  S.main = st;
  // streams == 1: the documented serial schedule (one kernel per launch: per-kernel timings in
  // isolation, qrkem.h); otherwise independent kernels of one operation share launches
  S.serial = ctx->streams == 1;
  if (opts.flag) {
    S.done = ctx->hflag_dev;
    S.ticket = ctx->ticket;
    S.host_in1 = opts.host_in1;
  }
  if (a.family == Family::MLKEM) {
    if (opts.kg_err) S.kg_err = ctx->hflag_dev + 1;
    S.xof_keep = opts.xof_keep;
    S.xof_given = opts.xof_given;
    const char* what = nullptr;
    const hipError_t e = ctx->mlkem.prepare(S, op, n, chunk, ctx->scratch, ctx->scratch_bytes, &what);
    if (e != hipSuccess) return hip_fail(what, e);
  }
  HT(3);
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = std::min(chunk, n - off);
    hipError_t e = hipSuccess;
    launch_begin();
    int32_t* const stat = status ? status + off : nullptr;
    switch (op) {
      case Op::KEYPAIR:
        e = f.keypair(a, m, o1 + off * a.pk, o2 + off * a.sk, coins + off * clen, ctx->scratch, S);
        break;
      case Op::ENCAPS:
        if (stat && !f.encaps_sets_status) e = hipMemsetAsync(stat, 0, m * sizeof(int32_t), st);
        if (e == hipSuccess)
          e = f.encaps(a, m, o1 + off * a.ct, o2 + off * a.ss, i1 + off * a.pk, coins + off * clen, stat, ctx->scratch,
                       S);
        break;
      case Op::DECAPS:
        if (stat && !f.decaps_sets_status) e = hipMemsetAsync(stat, 0, m * sizeof(int32_t), st);
        if (e == hipSuccess) e = f.decaps(a, m, o1 + off * a.ss, i1 + off * a.ct, i2 + off * a.sk, stat, ctx->scratch, S);
        if (e == hipSuccess && opts.frodo_mu) e = frodo_trace_mu(a, m, ctx->scratch, opts.frodo_mu + off * 32, st);
        break;
    }
    HT(4);
    if (e != hipSuccess) {
      ctx->mlkem.chunk_failed(S);  // whatever the family: S carries no ML-KEM counters for the others
      return hip_fail("kernel launch", e);
    }
    // key material of this chunk (seeds, m', K', Kbar, ...) does not outlive the call
    e = f.cleanse(a, m, ctx->scratch, st);
    if (e != hipSuccess) return hip_fail("hipMemsetAsync(cleanse)", e);
  }
  return 0;
}

// The row driver of the signature calls (outermost: it takes the lock): n > 0 rows through a launcher that uses the
// context's scratch (public values only: no cleanse), in equal chunks of at most min(qrk_ctx_set_chunk, cap) rows.
// launch(off, m) runs rows [off, off + m); the first failing chunk's status is the call's error, named `what`.
template <class Launch>
static int run_rows(qrk_ctx* ctx, hipStream_t st, size_t n, size_t cap, size_t (*scratch_bytes)(int, size_t), int which,
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

// The single-shot completion flag: one word of fine-grained (coherent) pinned memory.
static int flag_ready(qrk_ctx* ctx) {
  if (ctx->hflag_dev) return 0;
  hipError_t e = hipHostMalloc((void**)&ctx->hflag, 64, hipHostMallocCoherent);
  if (e != hipSuccess) return hip_fail("hipHostMalloc(flag)", e);
  *ctx->hflag = 0;
  void* d = nullptr;
  e = hipHostGetDevicePointer(&d, ctx->hflag, 0);
  if (e != hipSuccess) return hip_fail("hipHostGetDevicePointer(flag)", e);
  ctx->hflag_dev = (uint32_t*)d;
  return 0;
}

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Packed I/O of a host-pointer call of n handshakes: the inputs (i1 | i2, one H2D copy), then the
// outputs (o1 | o2 | status, one D2H copy), every slot rounded up to 256 bytes.  l_*: bytes per
// handshake (0: no such buffer); o_*: byte offset of the slot (i1 is at 0, the outputs at o_o1).
struct IoLayout {
  size_t n, l_i1, l_i2, l_o1, l_o2, l_st;
  size_t o_i2, o_o1, o_o2, o_st, total;
  IoLayout(const AlgInfo& a, Op op, size_t n_, bool coins, bool status) : n(n_) {
    switch (op) {
      case Op::KEYPAIR: l_i1 = coins ? a.kp_coins : 0, l_i2 = 0, l_o1 = a.pk, l_o2 = a.sk; break;
      case Op::ENCAPS: l_i1 = a.pk, l_i2 = coins ? a.enc_coins : 0, l_o1 = a.ct, l_o2 = a.ss; break;
      default: l_i1 = a.ct, l_i2 = a.sk, l_o1 = a.ss, l_o2 = 0; break;
    }
    l_st = status ? sizeof(int32_t) : 0;
    o_i2 = al256(n * l_i1), o_o1 = o_i2 + al256(n * l_i2), o_o2 = o_o1 + al256(n * l_o1);
    o_st = o_o2 + al256(n * l_o2), total = o_st + al256(n * l_st);
  }
};

// Zero-copy host call (see run_batch_host): the layout L (coins and status slots always present)
// lives in the pinned mirror, which the kernel addresses through its device mapping.
static int run_small_host(qrk_ctx* ctx, const AlgInfo& a, Op op, const IoLayout& L, uint8_t* o1, uint8_t* o2,
                          const uint8_t* i1, const uint8_t* i2, int32_t* status) {
  const size_t n = L.n;
  hipStream_t st = ctx->io_stream;
  if (ctx->hio_bytes < L.total) {
    ctx_quiesce(ctx);
    if (ctx->hio) OQS_MEM_cleanse(ctx->hio, ctx->hio_bytes);
    if (grow_pinned(&ctx->hio, &ctx->hio_bytes, L.total)) return -1;
    ctx->hio_dev = nullptr;
  }
  if (!ctx->hio_dev) {
    void* d = nullptr;
    hipError_t e = hipHostGetDevicePointer(&d, ctx->hio, 0);
    if (e != hipSuccess) return hip_fail("hipHostGetDevicePointer", e);
    ctx->hio_dev = (uint8_t*)d;
  }
  uint8_t* h = ctx->hio;
  // inputs (coins the caller did not supply come from the OS CSPRNG)
  if (L.l_i1) {
    if (i1) memcpy(h, i1, n * L.l_i1);
    else if (os_random(h, n * L.l_i1)) return -1;
  }
  if (L.l_i2) {
    if (i2) memcpy(h + L.o_i2, i2, n * L.l_i2);
    else if (os_random(h + L.o_i2, n * L.l_i2)) return -1;
  }
  memset(h + L.o_st, 0, n * L.l_st);
  HT(2);
  uint8_t* d = ctx->hio_dev;
  CallOpts opts;
  // n == 1: the kernel stores a ticket in fine-grained pinned memory once its outputs are visible,
  // and the host spins on it (about 4 us sooner than hipStreamSynchronize wakes up)
  opts.flag = n == 1 && flag_ready(ctx) == 0;
  // ML-KEM KeyGen: the pipelined kernel's error word, hflag[1] (the flag's 64-byte line)
  opts.kg_err = op == Op::KEYPAIR && n <= mlkem_kg_multi_max() && flag_ready(ctx) == 0;
  if (opts.kg_err) __atomic_store_n(ctx->hflag + 1, 0u, __ATOMIC_RELEASE);
  if (opts.flag) {
    ctx->ticket = ctx->ticket + 1 ? ctx->ticket + 1 : 1;
    // the public input (Encaps pk, Decaps c) may travel as a kernel argument; KeyGen's coins never
    opts.host_in1 = (op != Op::KEYPAIR && L.l_i1) ? h : nullptr;
  }
  // ML-KEM decapsulation reports no status (implicit rejection): only encapsulation writes it
  int rc = run_batch(ctx, a, op, n, d + L.o_o1, L.l_o2 ? d + L.o_o2 : nullptr, L.l_i1 ? d : nullptr,
                     L.l_i2 ? d + L.o_i2 : nullptr, (status && op == Op::ENCAPS) ? (int32_t*)(d + L.o_st) : nullptr, st,
                     opts);
  HT(5);
  hipError_t e = hipSuccess;
  if (!rc && opts.flag) {
    // bounded spin; a kernel that never stores the ticket (a launch or execution error) falls
    // back to the stream synchronise, which reports it
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (unsigned k = 0;; ++k) {
      if (__atomic_load_n(ctx->hflag, __ATOMIC_ACQUIRE) == ctx->ticket) {
        seen = true;
        break;
      }
      if ((k & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
    }
    HT(6);
    if (!seen) e = hipStreamSynchronize(st);
  } else if (!rc) {
    e = hipStreamSynchronize(st);
  }
  if (!rc && e != hipSuccess) rc = hip_fail("kernel execution", e);
  // the collector stores the error word before the ticket (or the kernel's end, which the stream
  // synchronise waited for)
  if (!rc && opts.kg_err && __atomic_load_n(ctx->hflag + 1, __ATOMIC_ACQUIRE) != 0)
    rc = fail("ML-KEM KeyGen: keygen hand-off timeout (a bounded cross-workgroup wait expired)");
  if (!rc) {
    memcpy(o1, h + L.o_o1, n * L.l_o1);
    if (L.l_o2) memcpy(o2, h + L.o_o2, n * L.l_o2);
    if (status) memcpy(status, h + L.o_st, n * L.l_st);
  }
  if (rc) {
    (void)hipStreamSynchronize(st);  // nothing may still read or write the mirror
    ctx->mlkem.keygen_failed(opts.kg_err, ctx->scratch, ctx->scratch_bytes, st);
  }
  OQS_MEM_cleanse(h, L.total);  // coins, secret keys and shared secrets do not outlive the call
  HT(7);
  return rc;
}

// Host-pointer wrapper: stage inputs, run, copy outputs back, synchronise.  The context
// keeps a device I/O buffer, a pinned host mirror and its own stream, so a call is one
// packed H2D copy, the kernels, one packed D2H copy and one synchronise (the reference's
// one-handshake-per-call pattern, oqs.py:318, 348, 372, pays no allocation per call).
static int run_batch_host(qrk_ctx* ctx, const AlgInfo& a, Op op, size_t n, uint8_t* o1, uint8_t* o2,
                          const uint8_t* i1, const uint8_t* i2, int32_t* status) {
  if (n == 0) return 0;
  DeviceGuard device_guard;
  if (device_guard.set(ctx->device)) return -1;
  // Small ML-KEM batches (one launch per operation, the reference's single-shot calls) run
  // zero-copy: the kernel reads its inputs from and writes its outputs to the pinned mirror, and
  // coins are drawn straight into it, so a call is one launch and one synchronise.
  const bool zc = a.family == Family::MLKEM && n <= mlkem_small_max();
  // coins the caller left out get no slot here (run_batch draws them); zero-copy calls reserve
  // the coin and status slots unconditionally
  const IoLayout L(a, op, n, zc || (op == Op::KEYPAIR ? i1 : i2), zc || status);
  if (!ctx->io_stream) {
    hipError_t e = hipStreamCreateWithFlags(&ctx->io_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail("hipStreamCreate(io)", e);
  }
  hipStream_t st = ctx->io_stream;
  if (zc) return run_small_host(ctx, a, op, L, o1, o2, i1, i2, status);
  if (grow_device(ctx, (void**)&ctx->dio, &ctx->dio_bytes, L.total, st)) return -1;
  if (ctx->hio_bytes < L.total) ctx->hio_dev = nullptr;  // reallocated below
  if (grow_pinned(&ctx->hio, &ctx->hio_bytes, L.total)) return -1;
  uint8_t *d = ctx->dio, *h = ctx->hio;
  if (L.l_i1) memcpy(h, i1, n * L.l_i1);
  if (L.l_i2) memcpy(h + L.o_i2, i2, n * L.l_i2);
  hipError_t e = L.o_o1 ? hipMemcpyAsync(d, h, L.o_o1, hipMemcpyHostToDevice, st) : hipSuccess;
  if (e != hipSuccess) return hip_fail("hipMemcpyAsync(H2D)", e);
  int rc = run_batch(ctx, a, op, n, d + L.o_o1, L.l_o2 ? d + L.o_o2 : nullptr, L.l_i1 ? d : nullptr,
                     L.l_i2 ? d + L.o_i2 : nullptr, status ? (int32_t*)(d + L.o_st) : nullptr, st, {});
  if (rc) return rc;
  e = hipMemcpyAsync(h + L.o_o1, d + L.o_o1, L.total - L.o_o1, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail("kernel execution / D2H", e);
  memcpy(o1, h + L.o_o1, n * L.l_o1);
  if (L.l_o2) memcpy(o2, h + L.o_o2, n * L.l_o2);
  if (status) memcpy(status, h + L.o_st, n * L.l_st);
  // the staged copies of secrets do not outlive the call: coins (KeyGen's i1, Encaps' i2) or sk
  // (Decaps' i2) in, sk or ss (o2; Decaps' o1) out
  struct Span {
    size_t off, len;
  };
  const Span sec[2] = {op == Op::KEYPAIR ? Span{0, n * L.l_i1} : Span{L.o_i2, n * L.l_i2},
                       op == Op::DECAPS ? Span{L.o_o1, n * L.l_o1} : Span{L.o_o2, n * L.l_o2}};
  for (const Span& z : sec) {
    if (!z.len) continue;
    OQS_MEM_cleanse(h + z.off, z.len);
    (void)hipMemsetAsync(d + z.off, 0, z.len, st);
  }
  return 0;
}

// ------------------------------------------------------------------ default context (single-shot API)
static std::mutex g_default_mu;
static qrk_ctx* g_default = nullptr;

static qrk_ctx* default_ctx() {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (!g_default) {
    g_default = new qrk_ctx();
    const char* dev = getenv("QRK_DEVICE");
    g_default->device = dev ? atoi(dev) : 0;
    g_default->chunk = 1 << 12;
  }
  return g_default;
}

static OQS_STATUS single(const AlgInfo& a, Op op, uint8_t* o1, uint8_t* o2, const uint8_t* i1, const uint8_t* i2) {
  HT(0);
  qrk_ctx* ctx = default_ctx();
  std::lock_guard<std::mutex> lk(ctx->mu);
  int32_t status = 0;
  HT(1);
  int rc = run_batch_host(ctx, a, op, 1, o1, o2, i1, i2, op == Op::KEYPAIR ? nullptr : &status);
  HT(9);
  // ML-KEM encaps: the FIPS 203 modulus check; HQC decaps: liboqs returns OQS_ERROR when the
  // re-encryption check fails (the shared secret K(sigma || ct) is still written)
  if (rc == 0 && status != 0)
    rc = fail(op == Op::ENCAPS ? "encapsulation key failed the FIPS 203 modulus check"
                               : "ciphertext rejected by the re-encryption check");
  return rc == 0 ? OQS_SUCCESS : OQS_ERROR;
}

// per-algorithm callbacks stored in OQS_KEM (liboqs semantics: no kem argument)
template <int I>
static OQS_STATUS cb_keypair(uint8_t* pk, uint8_t* sk) {
  return single(ALGS[I], Op::KEYPAIR, pk, sk, nullptr, nullptr);
}
template <int I>
static OQS_STATUS cb_encaps(uint8_t* ct, uint8_t* ss, const uint8_t* pk) {
  return single(ALGS[I], Op::ENCAPS, ct, ss, pk, nullptr);
}
template <int I>
static OQS_STATUS cb_decaps(uint8_t* ss, const uint8_t* ct, const uint8_t* sk) {
  return single(ALGS[I], Op::DECAPS, ss, nullptr, ct, sk);
}

template <int I>
static void fill_cbs(OQS_KEM* k, int idx) {
  if constexpr (I < (int)(sizeof(ALGS) / sizeof(ALGS[0]))) {
    if (idx == I) {
      k->keypair = cb_keypair<I>;
      k->encaps = cb_encaps<I>;
      k->decaps = cb_decaps<I>;
      return;
    }
    fill_cbs<I + 1>(k, idx);
  }
}

extern "C" {

// ------------------------------------------------------------------ Part 1: liboqs subset
void OQS_init(void) {}

const char* OQS_version(void) { return "0.12.0-qrkem-gfx950"; }

size_t OQS_KEM_alg_count(void) { return (size_t)NALG; }

const char* OQS_KEM_alg_identifier(size_t i) { return i < (size_t)NALG ? ALGS[i].name : nullptr; }

int OQS_KEM_alg_is_enabled(const char* method_name) {
  const AlgInfo* a = find_alg(method_name);
  return a && a->enabled ? 1 : 0;
}

OQS_KEM* OQS_KEM_new(const char* method_name) {
  const AlgInfo* a = find_alg(method_name);
  if (!a || !a->enabled) return nullptr;
  OQS_KEM* k = (OQS_KEM*)calloc(1, sizeof(OQS_KEM));
  if (!k) return nullptr;
  k->method_name = a->name;
  k->alg_version = ops_of(*a).alg_version;
  k->claimed_nist_level = (uint8_t)a->level;
  k->ind_cca = true;
  k->length_public_key = a->pk;
  k->length_secret_key = a->sk;
  k->length_ciphertext = a->ct;
  k->length_shared_secret = a->ss;
  fill_cbs<0>(k, (int)(a - ALGS));
  return k;
}

static const AlgInfo* alg_of(const OQS_KEM* kem) {
  if (!kem) {
    fail("null OQS_KEM");
    return nullptr;
  }
  return resolve(kem->method_name);
}

OQS_STATUS OQS_KEM_keypair(const OQS_KEM* kem, uint8_t* pk, uint8_t* sk) {
  const AlgInfo* a = alg_of(kem);
  return a ? single(*a, Op::KEYPAIR, pk, sk, nullptr, nullptr) : OQS_ERROR;
}
OQS_STATUS OQS_KEM_keypair_derand(const OQS_KEM* kem, uint8_t* pk, uint8_t* sk, const uint8_t* seed) {
  const AlgInfo* a = alg_of(kem);
  if (!a || !seed) return OQS_ERROR;
  return single(*a, Op::KEYPAIR, pk, sk, seed, nullptr);
}
OQS_STATUS OQS_KEM_encaps(const OQS_KEM* kem, uint8_t* ct, uint8_t* ss, const uint8_t* pk) {
  const AlgInfo* a = alg_of(kem);
  return a ? single(*a, Op::ENCAPS, ct, ss, pk, nullptr) : OQS_ERROR;
}
OQS_STATUS OQS_KEM_encaps_derand(const OQS_KEM* kem, uint8_t* ct, uint8_t* ss, const uint8_t* pk,
                                 const uint8_t* seed) {
  const AlgInfo* a = alg_of(kem);
  if (!a || !seed) return OQS_ERROR;
  return single(*a, Op::ENCAPS, ct, ss, pk, seed);
}
OQS_STATUS OQS_KEM_decaps(const OQS_KEM* kem, uint8_t* ss, const uint8_t* ct, const uint8_t* sk) {
  const AlgInfo* a = alg_of(kem);
  return a ? single(*a, Op::DECAPS, ss, nullptr, ct, sk) : OQS_ERROR;
}
void OQS_KEM_free(OQS_KEM* kem) { free(kem); }

// Empty signature registry (see include/qrkem.h: verification is qrk_sig_verify_batch, Part 2)
size_t OQS_SIG_alg_count(void) { return 0; }
const char* OQS_SIG_alg_identifier(size_t) { return nullptr; }
int OQS_SIG_alg_is_enabled(const char*) { return 0; }
OQS_SIG* OQS_SIG_new(const char*) {
  fail("signatures are not implemented by libqrkem");
  return nullptr;
}
OQS_STATUS OQS_SIG_keypair(const OQS_SIG*, uint8_t*, uint8_t*) { return OQS_ERROR; }
OQS_STATUS OQS_SIG_sign(const OQS_SIG*, uint8_t*, size_t*, const uint8_t*, size_t, const uint8_t*) {
  return OQS_ERROR;
}
OQS_STATUS OQS_SIG_verify(const OQS_SIG*, const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*) {
  return OQS_ERROR;
}
void OQS_SIG_free(OQS_SIG*) {}

void OQS_MEM_cleanse(void* ptr, size_t len) {
  if (!ptr) return;
  volatile uint8_t* p = (volatile uint8_t*)ptr;
  while (len--) *p++ = 0;
}

// ------------------------------------------------------------------ Part 2: batched API
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

// Zero every buffer of the context that can hold keys or secret intermediates (device scratch,
// handshake scratch, device and pinned host staging).  Synchronous.
static void cleanse_all(qrk_ctx* ctx) {
  ctx_quiesce(ctx);
  if (ctx->scratch) (void)hipMemset(ctx->scratch, 0, ctx->scratch_bytes);
  if (ctx->hs_scratch) (void)hipMemset(ctx->hs_scratch, 0, ctx->hs_scratch_bytes);
  if (ctx->dio) (void)hipMemset(ctx->dio, 0, ctx->dio_bytes);
  if (ctx->dstage) (void)hipMemset(ctx->dstage, 0, ctx->dstage_bytes);
  (void)hipDeviceSynchronize();
  if (ctx->hio) OQS_MEM_cleanse(ctx->hio, ctx->hio_bytes);
  if (ctx->hstage) OQS_MEM_cleanse(ctx->hstage, ctx->hstage_bytes);
}

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
    std::vector<uint8_t> tmp(len[b]);
    hipError_t e = hipMemcpy(tmp.data(), src[b], len[b], hipMemcpyDeviceToHost);
    for (uint8_t x : tmp) out[1 + b] += x != 0;
    // the copy may hold expanded key material (PRF / CBD output, FrodoKEM S, HQC x, y): wipe it
    // before the heap gets it back
    OQS_MEM_cleanse(tmp.data(), tmp.size());
    if (e != hipSuccess) return hip_fail("hipMemcpy(staging residue)", e);
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

int qrk_dbg_fail_after_flip(int on) {
  g_dbg_fail_after_flip.store(on, std::memory_order_relaxed);
  return 0;
}

int qrk_dbg_fixc_words(qrk_ctx* ctx, uint32_t* out, int* parity) {
  CallScope scope;
  if (open_inspect(scope, ctx, out && parity)) return -1;
  const char* what = nullptr;
  const hipError_t e = ctx->mlkem.fix_words(out, parity, &what);
  return e == hipSuccess ? 0 : hip_fail(what, e);
}

int qrk_dbg_kg_flags_residue(qrk_ctx* ctx, uint64_t* out) {
  CallScope scope;
  if (open_inspect(scope, ctx, out)) return -1;
  const hipError_t e = ctx->mlkem.kg_flags_residue(out);
  return e == hipSuccess ? 0 : hip_fail("hipMemcpy(kg flags)", e);
}

int qrk_dbg_mlkem_records_residue(qrk_ctx* ctx, const char* alg, size_t n, uint64_t* out) {
  CallScope scope;
  if (open_inspect(scope, ctx, out)) return -1;
  const AlgInfo* a = find_alg(alg);
  if (!a || a->family != Family::MLKEM) return fail("not an ML-KEM algorithm");
  size_t off = 0, bytes = 0;
  mlkem_records_span(*a, round64(std::min(n, chunk_for(ctx, *a))), &off, &bytes);
  if (off + bytes > ctx->scratch_bytes) return fail("the context's scratch does not cover that chunk");
  std::vector<uint8_t> tmp(bytes);
  const hipError_t e = hipMemcpy(tmp.data(), (const char*)ctx->scratch + off, bytes, hipMemcpyDeviceToHost);
  *out = 0;
  for (uint8_t x : tmp) *out += x != 0;
  OQS_MEM_cleanse(tmp.data(), tmp.size());
  return e == hipSuccess ? 0 : hip_fail("hipMemcpy(records residue)", e);
}

size_t qrk_ctx_effective_chunk(const qrk_ctx* ctx, const char* alg) {
  const AlgInfo* a = find_alg(alg);
  if (!ctx || !a) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return chunk_for(ctx, *a);
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

int qrk_kem_sizes(const char* alg, size_t out[6]) {
  const AlgInfo* a = find_alg(alg);
  if (!a) return fail(std::string("unsupported KEM: ") + (alg ? alg : "(null)"));
  out[0] = a->pk, out[1] = a->sk, out[2] = a->ct, out[3] = a->ss, out[4] = a->kp_coins, out[5] = a->enc_coins;
  return 0;
}

// The KEM entry points: null check, algorithm, context lock, then the device-pointer driver on the
// caller's stream or (host) the host-pointer wrapper on the context's own.
static int kem_call(qrk_ctx* ctx, const char* alg, bool host, Op op, size_t n, uint8_t* o1, uint8_t* o2,
                    const uint8_t* i1, const uint8_t* i2, int32_t* status, void* stream) {
  if (!ctx) return fail("null context");
  const AlgInfo* a = resolve(alg);
  if (!a) return -1;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (host) return run_batch_host(ctx, *a, op, n, o1, o2, i1, i2, status);
  return run_batch(ctx, *a, op, n, o1, o2, i1, i2, status, (hipStream_t)stream, {});
}
int qrk_kem_keypair_batch(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins,
                          void* stream) {
  return kem_call(ctx, alg, false, Op::KEYPAIR, n, pk, sk, coins, nullptr, nullptr, stream);
}
int qrk_kem_encaps_batch(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk,
                         const uint8_t* coins, int32_t* status, void* stream) {
  return kem_call(ctx, alg, false, Op::ENCAPS, n, ct, ss, pk, coins, status, stream);
}
int qrk_kem_decaps_batch(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk,
                         void* stream) {
  return kem_call(ctx, alg, false, Op::DECAPS, n, ss, nullptr, ct, sk, nullptr, stream);
}
int qrk_kem_decaps_batch_status(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ss, const uint8_t* ct,
                                const uint8_t* sk, int32_t* status, void* stream) {
  return kem_call(ctx, alg, false, Op::DECAPS, n, ss, nullptr, ct, sk, status, stream);
}
int qrk_kem_keypair_batch_host(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* pk, uint8_t* sk,
                               const uint8_t* coins) {
  return kem_call(ctx, alg, true, Op::KEYPAIR, n, pk, sk, coins, nullptr, nullptr, nullptr);
}
int qrk_kem_encaps_batch_host(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk,
                              const uint8_t* coins, int32_t* status) {
  return kem_call(ctx, alg, true, Op::ENCAPS, n, ct, ss, pk, coins, status, nullptr);
}
int qrk_kem_decaps_batch_host(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ss, const uint8_t* ct,
                              const uint8_t* sk) {
  return kem_call(ctx, alg, true, Op::DECAPS, n, ss, nullptr, ct, sk, nullptr, nullptr);
}
int qrk_kem_decaps_batch_status_host(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ss, const uint8_t* ct,
                                     const uint8_t* sk, int32_t* status) {
  return kem_call(ctx, alg, true, Op::DECAPS, n, ss, nullptr, ct, sk, status, nullptr);
}

int qrk_bench_coins(qrk_ctx* ctx, size_t n, size_t len, uint64_t seed, uint64_t first, uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  CallScope scope;  // no lock, no timer: bench.py's input generator, like qrk_tamper below
  if (scope.open(ctx, (hipStream_t)stream, 0)) return -1;
  hipError_t e = bench_coins(n, len, seed, first, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("bench_coins", e);
}

int qrk_tamper(qrk_ctx* ctx, size_t n, size_t ctlen, uint64_t seed, int mode, uint8_t* ct, void* stream) {
  if (!ctx) return fail("null context");
  // no lock (touches nothing of the context's); no timer: bench.py calls this inside its profiled,
  // timed step, and timing it would change the reported profile
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, 0)) return -1;
  hipError_t e = tamper_ciphertexts(n, ctlen, seed, mode, ct, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("tamper", e);
}

int qrk_digest_rows(qrk_ctx* ctx, size_t n, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len,
                    uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  if (n && (!a || !out || (b_len && !b))) return fail("null buffer");
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = digest_rows(n, a, a_len, b_len ? b : nullptr, b_len, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("digest_rows", e);
}

int qrk_hqc_supports(qrk_ctx* ctx, const char* alg, int kind, size_t n, const uint32_t* r, uint32_t* sup,
                     void* stream) {
  if (!ctx) return fail("null context");
  const AlgInfo* a = resolve(alg);
  if (!a) return -1;
  if (a->family != Family::HQC) return fail(std::string("not an HQC parameter set: ") + alg);
  if (kind != 0 && kind != 1) return fail("kind must be 0 (w) or 1 (w_r = w_e)");
  if (n && (!r || !sup)) return fail("null buffer");
  CallScope scope;  // locked but untimed: k_hqc_supports has never counted in a context's profile
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK)) return -1;
  hipError_t e = hqc_supports(*a, kind, n, r, sup, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("hqc_supports", e);
}

// qrk_hqc_code_decode and its traced twin qrk_dbg_hqc_decaps_trace (t_out != NULL): one body, so the
// chunk limit, the argument checks and the failed-launch reporting are the same
static int hqc_code_decode_call(const char* what, qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk,
                                const uint8_t* ct, uint8_t* t_out, bool traced, uint8_t* syms, uint8_t* mprime,
                                void* stream) {
  if (!ctx) return fail("null context");
  const AlgInfo* a = resolve(alg);
  if (!a) return -1;
  if (a->family != Family::HQC) return fail(std::string("not an HQC parameter set: ") + alg);
  if (n == 0) return 0;
  if (!sk || !ct || !syms || !mprime || (traced && !t_out)) return fail("null buffer");
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  if (n > chunk_for(ctx, *a)) return fail(std::string(what) + ": n exceeds the context chunk");
  if (grow_device(ctx, &ctx->scratch, &ctx->scratch_bytes, ops_of(*a).scratch_bytes(*a, round64(n)), st)) return -1;
  hipError_t e = hqc_code_decode(*a, n, sk, ct, t_out, syms, mprime, ctx->scratch, st);
  if (e != hipSuccess) return hip_fail(what, e);
  e = ops_of(*a).cleanse(*a, n, ctx->scratch, st);  // the symbols and m' do not outlive the call
  return e == hipSuccess ? 0 : hip_fail("hipMemsetAsync(cleanse)", e);
}

int qrk_hqc_code_decode(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* ct, uint8_t* syms,
                        uint8_t* mprime, void* stream) {
  return hqc_code_decode_call("hqc_code_decode", ctx, alg, n, sk, ct, nullptr, false, syms, mprime, stream);
}

int qrk_dbg_hqc_decaps_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* ct,
                             uint8_t* t_out, uint8_t* syms, uint8_t* mprime, void* stream) {
  return hqc_code_decode_call("hqc_decaps_trace", ctx, alg, n, sk, ct, t_out, true, syms, mprime, stream);
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
  return e == hipSuccess ? 0 : hip_fail("hkdf_sha256", e);
}

int qrk_handshake_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* coins_kp_i,
                        const uint8_t* coins_kp_r, const uint8_t* coins_enc, const uint8_t* info,
                        const uint64_t* info_off, size_t info_len, size_t key_len, uint8_t* pk_i, uint8_t* pk_r,
                        uint8_t* ct, uint8_t* key_i, uint8_t* key_r, int32_t* agree, void* stream) {
  if (!ctx) return fail("null context");
  const AlgInfo* a = resolve(alg);
  if (!a) return -1;
  if (key_len == 0 || key_len > 255 * 32) return fail("key_len must be 1..8160 bytes");
  if (n == 0) return 0;
  if (!pk_i || !pk_r || !ct || !key_i || !key_r) return fail("null output buffer");
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  // Ephemeral secrets of one chunk live in context scratch and are wiped afterwards
  // (the reference keeps them in Python objects: messaging.py:590-600, 809).
  const size_t chunk = chunk_for(ctx, *a);
  const size_t m0 = std::min(chunk, n);
  const size_t b_sk = al256(m0 * a->sk), b_ss = al256(m0 * a->ss);
  // ML-KEM batched chunks: the initiator's sampled matrix A_hat, kept from its KeyGen (:590) for its
  // Decaps (:1038) -- the same rho, so Decaps skips K^2 SampleNTT entries (27 of a handshake's ~174
  // ML-KEM-768 permutations).  Public data (a function of rho): outside the wiped range.
  const bool keep_a = a->family == Family::MLKEM && m0 > mlkem_small_max();
  const size_t b_mat = keep_a ? al256(mlkem_matrix_bytes(*a, m0)) : 0;
  if (grow_device(ctx, (void**)&ctx->hs_scratch, &ctx->hs_scratch_bytes, 2 * b_sk + 2 * b_ss + b_mat, st)) return -1;
  uint8_t *sk_i = ctx->hs_scratch, *sk_r = sk_i + b_sk, *ss_i = sk_r + b_sk, *ss_r = ss_i + b_ss;
  uint64_t* mat_i = keep_a ? (uint64_t*)(ss_r + b_ss) : nullptr;
  // wipes the ephemeral sk / ss on every exit path, error returns included (runs before the
  // scope records the end of the call)
  struct Wipe {
    void* p;
    size_t bytes;
    hipStream_t st;
    ~Wipe() { (void)hipMemsetAsync(p, 0, bytes, st); }
  } wipe{ctx->hs_scratch, 2 * b_sk + 2 * b_ss, st};
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = std::min(chunk, n - off);
    auto co = [&](const uint8_t* c, size_t len) { return c ? c + off * len : nullptr; };
    // initiate_key_exchange: ephemeral KeyGen (messaging.py:590); A_hat kept for its Decaps
    CallOpts kg_opts, dec_opts;
    dec_opts.xof_given = kg_opts.xof_keep = (keep_a && m > mlkem_small_max()) ? mat_i : nullptr;
    if (run_batch(ctx, *a, Op::KEYPAIR, m, pk_i + off * a->pk, sk_i, co(coins_kp_i, a->kp_coins), nullptr, nullptr, st,
                  kg_opts))
      return -1;
    // _handle_key_exchange_init: responder KeyGen (:809, pk sent back at :853) + Encaps (:830)
    if (run_batch(ctx, *a, Op::KEYPAIR, m, pk_r + off * a->pk, sk_r, co(coins_kp_r, a->kp_coins), nullptr, nullptr,
                  st, {}))
      return -1;
    if (run_batch(ctx, *a, Op::ENCAPS, m, ct + off * a->ct, ss_r, pk_i + off * a->pk, co(coins_enc, a->enc_coins),
                  nullptr, st, {}))
      return -1;
    hipError_t e = hkdf_sha256(m, ss_r, a->ss, a->ss, nullptr, 0, info, info_off ? info_off + off : nullptr,
                               info_len, key_len, key_r + off * key_len, key_len, st);  // :845
    if (e != hipSuccess) return hip_fail("hkdf_sha256", e);
    // _handle_key_exchange_response: Decaps (:1038) + HKDF (:1068)
    if (run_batch(ctx, *a, Op::DECAPS, m, ss_i, nullptr, ct + off * a->ct, sk_i, nullptr, st, dec_opts)) return -1;
    e = hkdf_sha256(m, ss_i, a->ss, a->ss, nullptr, 0, info, info_off ? info_off + off : nullptr, info_len,
                    key_len, key_i + off * key_len, key_len, st);
    if (e != hipSuccess) return hip_fail("hkdf_sha256", e);
    if (agree) {
      e = keys_equal(m, key_i + off * key_len, key_r + off * key_len, key_len, agree + off, st);
      if (e != hipSuccess) return hip_fail("keys_equal", e);
    }
  }
  return 0;
}

// "AES-256-GCM" / "ChaCha20-Poly1305": the reference's SymmetricAlgorithm.name strings (symmetric.py:72, 170)
static int resolve_aead(const char* alg, AeadAlg* out) {
  if (alg && !strcmp(alg, "AES-256-GCM")) return *out = AeadAlg::AES_256_GCM, 0;
  if (alg && !strcmp(alg, "ChaCha20-Poly1305")) return *out = AeadAlg::CHACHA20_POLY1305, 0;
  return fail(std::string("unsupported AEAD: ") + (alg ? alg : "(null)"));
}

int qrk_aead_seal_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* nonces,
                        const uint8_t* pt, const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off,
                        size_t aad_len, uint8_t* sealed, void* stream) {
  if (!ctx) return fail("null context");
  AeadAlg which;
  if (resolve_aead(alg, &which)) return -1;
  if (n == 0) return 0;
  if (!keys || !pt || !pt_off || !sealed || (!aad && (aad_off || aad_len))) return fail("null buffer");
  if (aad_len >> 31) return fail("AEAD row lengths are 32-bit: aad_len must be below 2^31");
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
  return e == hipSuccess ? 0 : hip_fail("aead_seal", e);
}

int qrk_aead_open_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* sealed,
                        const uint64_t* sealed_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                        uint8_t* pt, int32_t* status, void* stream) {
  if (!ctx) return fail("null context");
  AeadAlg which;
  if (resolve_aead(alg, &which)) return -1;
  if (n == 0) return 0;
  if (!keys || !sealed || !sealed_off || !pt || !status || (!aad && (aad_off || aad_len))) return fail("null buffer");
  if (aad_len >> 31) return fail("AEAD row lengths are 32-bit: aad_len must be below 2^31");
  CallScope scope;  // not ordered against the context's last use: Open touches no context buffer
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = aead_open(which, n, keys, sealed, sealed_off, aad, aad_off, aad_len, pt, status, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("aead_open", e);
}

// test hooks (qrkem_debug.h): Poly1305 and GHASH on chosen keys
int qrk_dbg_poly1305_batch(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, uint8_t* tag,
                           void* stream) {
  if (n && (!key32 || !msg || !msg_off || !tag)) return fail("null buffer");
  launch_begin();  // no context, so no scope
  hipError_t e = dbg_poly1305(n, key32, msg, msg_off, tag, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("dbg_poly1305", e);
}
int qrk_dbg_ghash_batch(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, uint8_t* out,
                        void* stream) {
  if (n && (!h || !data || !data_off || !out)) return fail("null buffer");
  launch_begin();
  hipError_t e = dbg_ghash(n, h, data, data_off, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("dbg_ghash", e);
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
  if (!ctx) return fail("null context");
  AeadAlg which;
  if (resolve_aead(alg, &which)) return -1;
  if (n == 0) return 0;
  if (!keys || !pt || !pt_off || !sealed || (!aad && (aad_off || aad_len))) return fail("null buffer");
  if (aad_len >> 31) return fail("AEAD row lengths are 32-bit: aad_len must be below 2^31");
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
  return e == hipSuccess ? 0 : hip_fail("aead_seal_long", e);
}

int qrk_aead_open_long_batch(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* keys, const uint8_t* sealed,
                             const uint64_t* sealed_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                             size_t max_len, uint8_t* pt, int32_t* status, void* stream) {
  if (!ctx) return fail("null context");
  AeadAlg which;
  if (resolve_aead(alg, &which)) return -1;
  if (n == 0) return 0;
  if (!keys || !sealed || !sealed_off || !pt || !status || (!aad && (aad_off || aad_len))) return fail("null buffer");
  if (aad_len >> 31) return fail("AEAD row lengths are 32-bit: aad_len must be below 2^31");
  if (aead_long_args(which, n, max_len)) return -1;
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;  // ordered: unlike qrk_aead_open_batch this call uses the context's scratch
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return -1;
  if (aead_long_scratch(ctx, which, n, max_len, st)) return -1;
  hipError_t e = aead_open_long(which, n, keys, sealed, sealed_off, aad, aad_off, aad_len, max_len, pt, status,
                                ctx->scratch, st);
  return e == hipSuccess ? 0 : hip_fail("aead_open_long", e);
}

// test hooks (qrkem.h): the long calls' segment and tail MAC machinery on chosen keys, and what it left behind
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
  return e == hipSuccess ? 0 : hip_fail("dbg_mac_long", e);
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
  std::vector<uint8_t> tmp(bytes);
  const hipError_t e = hipMemcpy(tmp.data(), ctx->scratch, bytes, hipMemcpyDeviceToHost);
  for (uint8_t x : tmp) *out |= x;
  OQS_MEM_cleanse(tmp.data(), tmp.size());
  return e == hipSuccess ? 0 : hip_fail("hipMemcpy(long AEAD residue)", e);
}

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

// test hook (qrkem_debug.h): qrk_kem_decaps_batch for a FrodoKEM parameter set that also writes mu'
int qrk_dbg_frodo_decaps_trace(qrk_ctx* ctx, const char* alg, size_t n, uint8_t* ss, const uint8_t* ct,
                               const uint8_t* sk, uint8_t* mu_out, void* stream) {
  if (!ctx) return fail("null context");
  const AlgInfo* a = resolve(alg);
  if (!a) return -1;
  if (a->family != Family::FRODO) return fail(std::string("not a FrodoKEM parameter set: ") + alg);
  if (n && (!ss || !ct || !sk || !mu_out)) return fail("null buffer");
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallOpts opts;
  opts.frodo_mu = mu_out;
  return run_batch(ctx, *a, Op::DECAPS, n, ss, nullptr, ct, sk, nullptr, (hipStream_t)stream, opts);
}

int qrk_base64_encode_batch(qrk_ctx* ctx, size_t n, const uint8_t* in, size_t in_len, uint8_t* out, void* stream) {
  if (!ctx) return fail("null context");
  if (n && in_len && (!in || !out)) return fail("null buffer");
  CallScope scope;
  if (scope.open(ctx, (hipStream_t)stream, CallScope::LOCK | CallScope::TIMER)) return -1;
  hipError_t e = base64_encode(n, in, in_len, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail("base64_encode", e);
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
  return e == hipSuccess ? 0 : hip_fail("base64_decode", e);
}

const char* qrk_last_error(void) { return g_err.c_str(); }

int qrk_device_count(void) {
  int c = 0;
  return hipGetDeviceCount(&c) == hipSuccess ? c : 0;
}

}  // extern "C"
