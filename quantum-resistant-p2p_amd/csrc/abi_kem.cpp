// C ABI of libqrkem.so (declared in include/qrkem.h).
//
// Part 1 mirrors the liboqs entry points bound by the reference's ctypes
// wrapper (quantum_resistant_p2p/vendor/oqs.py:192-198, 271, 318, 348, 372,
// 386-390, 397, 406-411); each single-shot call is a batch of one on the GPU.
// Part 2 is the batched device API.  There is no CPU fallback: with no HIP
// device every KEM call returns OQS_ERROR and qrk_last_error() says why.
//
// This file is the KEM surface of both parts: the liboqs subset, the batch driver and its two host-pointer
// paths, the handshake driver, the HQC and FrodoKEM calls, and the hooks that inspect what these leave behind.
// The context and the opening of a call are in abi_ctx.h; AEAD, signatures and the small calls in abi_aead.cpp,
// abi_sig.cpp and abi_util.cpp.  single, run_batch_host, run_small_host and run_batch stay in this one file: they
// are the single-shot latency path.
#include <chrono>

#include "abi_ctx.h"

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
  bool no_keep = false;               // ML-KEM KeyGen: leave the context's kept region as it is (the handshake
                                      // driver's responder keys, which this context never decapsulates under)
  uint8_t* frodo_mu = nullptr;        // FrodoKEM Decaps (tests): mu' [n][32], copied out before each chunk's cleanse
};

static size_t chunk_for(const qrk_ctx* ctx, const AlgInfo& a) {
  if (a.family == Family::MLKEM) return ctx->chunk;
  return std::min(ctx->chunk, scratch_cap(ops_of(a).scratch_bytes(a, 1024) / 1024 + 1));
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
  bool keeps = false;
  if (a.family == Family::MLKEM) {
    if (opts.kg_err) S.kg_err = ctx->hflag_dev + 1;
    const char* what = nullptr;
    const hipError_t e = ctx->mlkem.prepare(S, op, n, chunk, ctx->scratch, ctx->scratch_bytes, &what);
    if (e != hipSuccess) return hip_fail(what, e);
    // KeyGen keeps its sampled matrices for this context's Decaps of the same keys (CtxState, the kept
    // region): invalid from here until every chunk is queued, so a failed KeyGen leaves none
    // (a KeyGen of one-launch chunks alone neither writes the region nor looks at it)
    keeps = op == Op::KEYPAIR && !opts.no_keep && n > mlkem_small_max();
    if (keeps) {
      struct Wait {
        qrk_ctx* ctx;
        hipStream_t st;
      } w{ctx, st};
      ctx->mlkem.keep_begin(a, n, chunk, mlkem_keep_cap_bytes(), [](void* p) {
        ctx_quiesce(((Wait*)p)->ctx);
        (void)hipStreamSynchronize(((Wait*)p)->st);
      }, &w);
    }
  }
  HT(3);
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = std::min(chunk, n - off);
    hipError_t e = hipSuccess;
    launch_begin();
    if (keeps) ctx->mlkem.keep_chunk(S, off / chunk);
    if (a.family == Family::MLKEM && op == Op::DECAPS) ctx->mlkem.kept_chunk(S, a, chunk, off / chunk, m);
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
  if (keeps) ctx->mlkem.keep_commit();
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
  // the outputs of a finished call, from the host mirror `h` of this layout to the caller's buffers
  void copy_out(const uint8_t* h, uint8_t* o1, uint8_t* o2, int32_t* status) const {
    memcpy(o1, h + o_o1, n * l_o1);
    if (l_o2) memcpy(o2, h + o_o2, n * l_o2);
    if (status) memcpy(status, h + o_st, n * l_st);
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
  if (!rc) L.copy_out(h, o1, o2, status);
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
  L.copy_out(h, o1, o2, status);
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

// ------------------------------------------------------------------ Part 2: batched API, the KEM calls
// ---- test hooks (qrkem_debug.h): what the ML-KEM paths keep in, and leave in, a context
int qrk_dbg_fixc_words(qrk_ctx* ctx, uint32_t* out, int* parity) {
  CallScope scope;
  if (open_inspect(scope, ctx, out && parity)) return -1;
  const char* what = nullptr;
  const hipError_t e = ctx->mlkem.fix_words(out, parity, &what);
  return hip_done(what, e);
}

int qrk_dbg_kg_flags_residue(qrk_ctx* ctx, uint64_t* out) {
  CallScope scope;
  if (open_inspect(scope, ctx, out)) return -1;
  const hipError_t e = ctx->mlkem.kg_flags_residue(out);
  return hip_done("hipMemcpy(kg flags)", e);
}

int qrk_dbg_mlkem_records_residue(qrk_ctx* ctx, const char* alg, size_t n, uint64_t* out) {
  CallScope scope;
  if (open_inspect(scope, ctx, out)) return -1;
  const AlgInfo* a = find_alg(alg);
  if (!a || a->family != Family::MLKEM) return fail("not an ML-KEM algorithm");
  size_t off = 0, bytes = 0;
  mlkem_records_span(*a, round64(std::min(n, chunk_for(ctx, *a))), &off, &bytes);
  if (off + bytes > ctx->scratch_bytes) return fail("the context's scratch does not cover that chunk");
  *out = 0;
  return read_residue((const char*)ctx->scratch + off, bytes, count_nonzero, "hipMemcpy(records residue)", out);
}

size_t qrk_ctx_effective_chunk(const qrk_ctx* ctx, const char* alg) {
  const AlgInfo* a = find_alg(alg);
  if (!ctx || !a) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return chunk_for(ctx, *a);
}

int qrk_mlkem_keep_plan(const char* alg, size_t n, size_t chunk, size_t cap_bytes, size_t out[4]) {
  const AlgInfo* a = find_alg(alg);
  if (!a || a->family != Family::MLKEM) return fail("not an ML-KEM algorithm");
  if (!out || chunk == 0) return fail("bad argument");
  const size_t rows = n ? chunk_plan(n, round64(chunk)) : 0;
  const KeepPlan p = mlkem_keep_plan(mlkem_matrix_bytes(*a, 64) / 64, n, rows, mlkem_small_max(),
                                     cap_bytes == (size_t)-1 ? mlkem_keep_cap_bytes() : cap_bytes);
  out[0] = rows, out[1] = p.batched, out[2] = p.kept, out[3] = p.bytes;
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
  return hip_done("hqc_supports", e);
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
  return hip_done("hipMemsetAsync(cleanse)", e);
}

int qrk_hqc_code_decode(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* ct, uint8_t* syms,
                        uint8_t* mprime, void* stream) {
  return hqc_code_decode_call("hqc_code_decode", ctx, alg, n, sk, ct, nullptr, false, syms, mprime, stream);
}

int qrk_dbg_hqc_decaps_trace(qrk_ctx* ctx, const char* alg, size_t n, const uint8_t* sk, const uint8_t* ct,
                             uint8_t* t_out, uint8_t* syms, uint8_t* mprime, void* stream) {
  return hqc_code_decode_call("hqc_decaps_trace", ctx, alg, n, sk, ct, t_out, true, syms, mprime, stream);
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
  // ML-KEM batched chunks: the initiator's sampled matrix A_hat stays in the context's kept region from
  // its KeyGen (:590) for its Decaps (:1038) -- the same rho, so Decaps skips K^2 SampleNTT entries (27 of
  // a handshake's ~174 ML-KEM-768 permutations).  The region's own budget decides whether it is kept; a
  // batch never fails for it.  The responder's KeyGen in between leaves the region alone.
  if (grow_device(ctx, (void**)&ctx->hs_scratch, &ctx->hs_scratch_bytes, 2 * b_sk + 2 * b_ss, st)) return -1;
  uint8_t *sk_i = ctx->hs_scratch, *sk_r = sk_i + b_sk, *ss_i = sk_r + b_sk, *ss_r = ss_i + b_ss;
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
    if (run_batch(ctx, *a, Op::KEYPAIR, m, pk_i + off * a->pk, sk_i, co(coins_kp_i, a->kp_coins), nullptr, nullptr, st,
                  {}))
      return -1;
    // _handle_key_exchange_init: responder KeyGen (:809, pk sent back at :853) + Encaps (:830)
    CallOpts responder;
    responder.no_keep = true;
    if (run_batch(ctx, *a, Op::KEYPAIR, m, pk_r + off * a->pk, sk_r, co(coins_kp_r, a->kp_coins), nullptr, nullptr,
                  st, responder))
      return -1;
    if (run_batch(ctx, *a, Op::ENCAPS, m, ct + off * a->ct, ss_r, pk_i + off * a->pk, co(coins_enc, a->enc_coins),
                  nullptr, st, {}))
      return -1;
    hipError_t e = hkdf_sha256(m, ss_r, a->ss, a->ss, nullptr, 0, info, info_off ? info_off + off : nullptr,
                               info_len, key_len, key_r + off * key_len, key_len, st);  // :845
    if (e != hipSuccess) return hip_fail("hkdf_sha256", e);
    // _handle_key_exchange_response: Decaps (:1038) + HKDF (:1068)
    if (run_batch(ctx, *a, Op::DECAPS, m, ss_i, nullptr, ct + off * a->ct, sk_i, nullptr, st, {})) return -1;
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

// test hook (qrkem_debug.h): the handshake driver's key compare on chosen rows
int qrk_dbg_keys_equal(size_t n, const uint8_t* a, const uint8_t* b, size_t len, int32_t* agree, void* stream) {
  if (n && (!a || !b || !agree)) return fail("null buffer");
  if (len == 0 || len > 255 * 32) return fail("key length must be 1..8160 bytes");
  launch_begin();  // no context, so no scope
  hipError_t e = keys_equal(n, a, b, len, agree, (hipStream_t)stream);
  return hip_done("keys_equal", e);
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

// The two FrodoKEM forward-path hooks: one chunk on the context's scratch, no chunking (n within the context chunk).
// The argument checks of qrk_dbg_frodo_decaps_trace, in its order; then the call's scope and the scratch.
static const AlgInfo* frodo_hook_open(const char* what, CallScope& scope, qrk_ctx* ctx, const char* alg, size_t n,
                                      bool bufs_ok, hipStream_t st) {
  if (!ctx) return fail("null context"), nullptr;
  const AlgInfo* a = resolve(alg);
  if (!a) return nullptr;
  if (a->family != Family::FRODO) return fail(std::string("not a FrodoKEM parameter set: ") + alg), nullptr;
  if (n && !bufs_ok) return fail("null buffer"), nullptr;
  if (scope.open(ctx, st, CallScope::LOCK | CallScope::ORDER | CallScope::TIMER)) return nullptr;
  if (n > chunk_for(ctx, *a)) return fail(std::string(what) + ": n exceeds the context chunk"), nullptr;
  if (n && grow_device(ctx, &ctx->scratch, &ctx->scratch_bytes, ops_of(*a).scratch_bytes(*a, round64(n)), st))
    return nullptr;
  return a;
}

// test hook (qrkem_debug.h): k_fr_sample alone on a caller-chosen stream of 16-bit words
int qrk_dbg_frodo_sample(qrk_ctx* ctx, const char* alg, int kg, size_t n, const uint16_t* words, int8_t* s8,
                         int16_t* e16, int16_t* epp16, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;
  const AlgInfo* a = frodo_hook_open("frodo_sample", scope, ctx, alg, n, words && s8 && e16 && (kg || epp16), st);
  if (!a) return -1;
  if (n == 0) return 0;
  return hip_done("frodo_sample", frodo_dbg_sample(*a, kg != 0, n, words, s8, e16, epp16, ctx->scratch, st));
}

// Every value of a device array of n int8 / int16 samples within [-max, max]?  rows x pitch int8 with `used`
// leading columns per row: the rest (the pad columns) must be zero.  Synchronous (a host copy): -1 on a copy failure.
static int samples_in_range(const void* dev, size_t rows, size_t pitch, size_t used, bool wide, int max,
                            hipStream_t st) {
  std::vector<int16_t> h16(wide ? rows * pitch : 0);
  std::vector<int8_t> h8(wide ? 0 : rows * pitch);
  hipError_t e = hipStreamSynchronize(st);
  if (e == hipSuccess)
    e = hipMemcpy(wide ? (void*)h16.data() : (void*)h8.data(), dev, rows * pitch * (wide ? 2 : 1), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail("hipMemcpy(samples)", e);
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < pitch; ++c) {
      const int v = wide ? h16[r * pitch + c] : h8[r * pitch + c];
      if (c < used ? (v < -max || v > max) : v != 0) return 1;
    }
  return 0;
}

// test hook (qrkem_debug.h): everything after the sampler, on caller-chosen sample matrices
int qrk_dbg_frodo_from_samples(qrk_ctx* ctx, const char* alg, int kg, size_t n, const int8_t* s8, const int16_t* e16,
                               const int16_t* epp16, const uint8_t* in, const uint8_t* mu, uint8_t* out, uint8_t* sk,
                               void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CallScope scope;
  const bool bufs_ok = s8 && e16 && in && out && (kg ? sk != nullptr : epp16 && mu);
  const AlgInfo* a = frodo_hook_open("frodo_from_samples", scope, ctx, alg, n, bufs_ok, st);
  if (!a) return -1;
  if (n == 0) return 0;
  // the kernels' accumulator bounds and the zero pad of S' hold for the sampler's output only: refuse anything else
  const int max = frodo_sample_max(*a);
  const size_t N = (size_t)a->k;
  int bad = samples_in_range(s8, n * 8, frodo_sample_pitch(*a), N, false, max, st);
  if (bad == 0) bad = samples_in_range(e16, n, 8 * N, 8 * N, true, max, st);
  if (bad == 0 && !kg) bad = samples_in_range(epp16, n, 64, 64, true, max, st);
  if (bad < 0) return -1;
  if (bad) return fail("frodo_from_samples: a sample outside the parameter set's sampler range (or a nonzero pad column)");
  hipError_t e = frodo_dbg_from_samples(*a, kg != 0, n, s8, e16, epp16, in, mu, out, sk, ctx->scratch, st);
  if (e != hipSuccess) return hip_fail("frodo_from_samples", e);
  return hip_done("hipMemsetAsync(cleanse)", ops_of(*a).cleanse(*a, n, ctx->scratch, st));  // kk holds what seeds held
}

}  // extern "C"
