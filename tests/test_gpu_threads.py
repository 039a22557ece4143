"""GPU: a call does not depend on what other host threads do meanwhile, on the same context or on another.

Everything else in the suite calls the library from one thread.  Here up to eight Python threads (one process;
ctypes drops the GIL for every call) run the plans of tests/thread_cases.py at once: on ONE context, on a context
each, through the process-wide default context of the single-shot OQS calls, beside a thread whose calls all fail,
beside a profiled context, and over one key set.  Every output buffer is pre-filled (0xA5, status 7) and compared
with the C oracle, the Python specs or a committed fixture, never with another run of the library.

The harness (run_jobs): daemon threads released together by a Barrier; the first failure sets an Event that every
worker looks at before each step, so nothing more is started after it; the main thread joins with a limit of
T x (the same steps run serially on one thread, measured first in the same test) + 30 s, and a worker still alive
then is a hang: the session ends there.  No retries.  Each test prints its serial time and the number of pairs of
calls from different threads that were inside the library at the same time (thread_cases.overlaps), which must be
above zero: a run that happened to be serial would prove nothing.

Measured on one MI355X (serial time of the plan, overlapping pairs; the seven tests took 3.7 s together, so every
join limit is the 30 s floor):
  test_one_shared_context                       serial 0.24 s, 226 pairs
  test_eight_contexts_eight_families            serial 0.07 s, 56 pairs
  test_default_context_through_oqs              serial 0.10 s, 932 pairs
  test_lazy_contexts_of_shared_wrapper_objects  serial 0.12 s, 181 pairs
  test_errors_stay_with_their_thread            serial 0.02 s, 21 pairs
  test_profiling_is_per_context                 serial 0.02 s, 15 pairs
  test_key_sets_from_four_threads               serial 0.05 s, 10 pairs
"""
import contextlib
import ctypes as ct
import threading
import time
import traceback

import numpy as np
import pytest

import aead_spec
import oracle as orc
import thread_cases as tc

torch = pytest.importorskip("torch")

import test_gpu_mldsa_keyed as tk  # noqa: E402  (their pre-filling call helpers; imported here, not in a worker)
import test_gpu_mldsa_sign as ts  # noqa: E402
import test_gpu_slhdsa as tv  # noqa: E402

pytestmark = pytest.mark.gpu
HUNG = False  # set when a worker missed its join limit: nothing more is sent to the GPU, not even a clean-up

QUIET = {"qrk_last_error", "qrk_kem_sizes", "qrk_sig_sizes"}  # no context, no device: not calls that can overlap


@pytest.fixture(scope="module")
def lib():
    from qrkem._debug import bind
    return bind()


def BatchKEM(alg):
    from qrkem.batch import BatchKEM as cls
    return cls(alg, device=0)


# ------------------------------------------------------------------ the log of calls
class Logged:
    """The library as one worker sees it: every call's [enter, return] goes to the shared log under the worker's
    number (list.append is atomic).  span() does the same for a call made through a wrapper class."""

    def __init__(self, lib, log, thread):
        self._lib, self._log, self._thread = lib, log, thread

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in QUIET:
            return fn

        def call(*args):
            t0 = time.monotonic_ns()
            try:
                return fn(*args)
            finally:
                self._log.append((self._thread, t0, time.monotonic_ns()))
        return call

    @contextlib.contextmanager
    def span(self):
        t0 = time.monotonic_ns()
        try:
            yield
        finally:
            self._log.append((self._thread, t0, time.monotonic_ns()))


# ------------------------------------------------------------------ one step through the C ABI, outputs pre-filled
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()  # on the calling thread's current stream


def host(t):
    return t.cpu().numpy()  # waits for that stream only


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def full(shape, value=tc.FILL, dtype=torch.uint8):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def status_buf(n):
    return full((n,), tc.STATUS_FILL, torch.int32)


def matrix(blobs, width):
    return np.frombuffer(b"".join(blobs), np.uint8).reshape(len(blobs), width).copy()


def packed(blobs):
    """Ragged rows as the ABI takes them: the bytes back to back and n + 1 offsets, both on the device."""
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    return dev(np.frombuffer(b"".join(blobs) or b"\0", np.uint8).copy()), dev(off), off


def kem_step(lib, ctx, s):
    a, n, z, i = s.alg.encode(), s.n, orc.sizes(s.alg), s.inputs
    if s.host:
        out = lambda w: np.full((n, w), tc.FILL, np.uint8)  # noqa: E731

        def p(x):
            assert x.flags["C_CONTIGUOUS"] and x.dtype in (np.uint8, np.int32)
            return x.ctypes.data
        st = np.full(n, tc.STATUS_FILL, np.int32)
        if s.op == "keypair":
            pk, sk, coins = out(z["pk"]), out(z["sk"]), np.ascontiguousarray(i["coins"])
            return lib.qrk_kem_keypair_batch_host(ctx, a, n, p(pk), p(sk), p(coins)), {"pk": pk, "sk": sk}
        if s.op == "encaps":
            c, ss, pk, coins = out(z["ct"]), out(z["ss"]), np.ascontiguousarray(i["pk"]), np.ascontiguousarray(i["coins"])
            rc = lib.qrk_kem_encaps_batch_host(ctx, a, n, p(c), p(ss), p(pk), p(coins), p(st))
            return rc, {"ct": c, "ss": ss, "status": st}
        assert s.op == "decaps", s.op
        ss, c, sk = out(z["ss"]), np.ascontiguousarray(i["ct"]), np.ascontiguousarray(i["sk"])
        rc = lib.qrk_kem_decaps_batch_status_host(ctx, a, n, p(ss), p(c), p(sk), p(st))
        return rc, {"ss": ss, "status": st}
    if s.op == "keypair":
        coins, pk, sk = dev(i["coins"]), full((n, z["pk"])), full((n, z["sk"]))
        rc = lib.qrk_kem_keypair_batch(ctx, a, n, pk.data_ptr(), sk.data_ptr(), coins.data_ptr(), stream())
        return rc, {"pk": host(pk), "sk": host(sk)}
    if s.op == "encaps":
        pk, coins, c, ss, st = dev(i["pk"]), dev(i["coins"]), full((n, z["ct"])), full((n, z["ss"])), status_buf(n)
        rc = lib.qrk_kem_encaps_batch(ctx, a, n, c.data_ptr(), ss.data_ptr(), pk.data_ptr(), coins.data_ptr(),
                                      st.data_ptr(), stream())
        c = host(c)
        return rc, {"ct": c, "ss": host(ss), "status": host(st), "ct0": [c[0].tobytes()]}
    sk, c, ss, st = dev(i["sk"]), dev(i["ct"]), full((n, z["ss"])), status_buf(n)
    got = {}
    if s.op == "decaps_tampered":  # qrk_tamper mode 2 on the device copy, then Decaps of what it left
        rc = lib.qrk_tamper(ctx, n, z["ct"], i["seed"], 2, c.data_ptr(), stream())
        if rc != 0:
            return rc, got
        got["ct_tampered"] = host(c)
    else:
        assert s.op == "decaps", s.op
    rc = lib.qrk_kem_decaps_batch_status(ctx, a, n, ss.data_ptr(), c.data_ptr(), sk.data_ptr(), st.data_ptr(), stream())
    got.update(ss=host(ss), status=host(st))
    return rc, got


def sig_step(lib, ctx, s):
    """The signature steps go through the helpers of the per-family GPU tests, which pre-fill every output and
    assert the call's return value themselves."""
    i = s.inputs
    if s.op == "sig_keygen":
        pk, sk = ts.keygen(lib, ctx, s.alg, i["xi"])
        return 0, {"pk": pk, "sk": sk}
    if s.op == "sig_sign":
        sigs, status = ts.sign(lib, ctx, s.alg, i["sk"], i["msg"])
        return 0, {"sig_sha3": tc.sha3_rows(sigs), "status": status}
    assert s.op == "sig_verify", s.op
    if s.alg == tc.SLHDSA:
        return 0, {"status": tv.run(lib, ctx, s.alg, list(zip(i["pk"], i["msg"], i["sig"])), trace=False)["status"]}
    return 0, {"status": ts.verify(lib, ctx, s.alg, i["pk"], i["msg"], i["sig"])}


def aead_step(lib, ctx, s):
    a, n, i = s.alg.encode(), s.n, s.inputs
    keys = dev(matrix(i["key"], 32))
    aad, aad_off, _ = packed(i["aad"])
    if s.op == "aead_seal":
        nonces = dev(matrix(i["nonce"], 12))
        pt, pt_off, off = packed(i["pt"])
        out = full((int(off[-1]) + 28 * n,))
        rc = lib.qrk_aead_seal_batch(ctx, a, n, keys.data_ptr(), nonces.data_ptr(), pt.data_ptr(), pt_off.data_ptr(),
                                     aad.data_ptr(), aad_off.data_ptr(), 0, out.data_ptr(), stream())
        h = host(out)
        return rc, {"sealed": [h[off[k] + 28 * k:off[k + 1] + 28 * (k + 1)].tobytes() for k in range(n)]}
    sealed, sealed_off, off = packed(i["sealed"])
    out, st = full((max(int(off[-1]) - 28, 1),)), status_buf(n)
    rc = lib.qrk_aead_open_batch(ctx, a, n, keys.data_ptr(), sealed.data_ptr(), sealed_off.data_ptr(), aad.data_ptr(),
                                 aad_off.data_ptr(), 0, out.data_ptr(), st.data_ptr(), stream())
    h = host(out)
    pts = [h[max(off[k] - 28 * k, 0):max(off[k + 1] - 28 * (k + 1), 0)].tobytes() for k in range(n)]
    return rc, {"pt": pts, "status": host(st)}


def small_step(lib, ctx, s):
    n, i = s.n, s.inputs
    if s.op == "hkdf":
        ikm = dev(matrix(i["ikm"], len(i["ikm"][0])))
        salt = dev(np.frombuffer(i["salt"], np.uint8).copy()) if i["salt"] else None
        info = dev(np.frombuffer(i["info"] or b"\0", np.uint8).copy())
        okm = full((n, i["L"]))
        rc = lib.qrk_hkdf_sha256_batch(ctx, n, ikm.data_ptr(), ikm.shape[1], salt.data_ptr() if salt is not None else None,
                                       len(i["salt"]), info.data_ptr(), None, len(i["info"]), okm.data_ptr(), i["L"],
                                       stream())
        return rc, {"okm": host(okm)}
    if s.op == "b64_encode":
        raw = dev(i["raw"])
        out = full((n, 4 * ((raw.shape[1] + 2) // 3)))
        rc = lib.qrk_base64_encode_batch(ctx, n, raw.data_ptr(), raw.shape[1], out.data_ptr(), stream())
        return rc, {"text": host(out)}
    assert s.op == "b64_decode", s.op
    text, out, st = dev(i["text"]), full((n, i["L"])), status_buf(n)
    rc = lib.qrk_base64_decode_batch(ctx, n, text.data_ptr(), i["L"], out.data_ptr(), st.data_ptr(), stream())
    return rc, {"raw": host(out), "status": host(st)}


def keyed_step(lib, ctx, s, sets):
    n, i = s.n, s.inputs
    if s.op == "sign_keyed":
        sigs, status = tk.sign_keyed(lib, ctx, sets["mldsa"], s.alg, i["msg"], i["index"])
        return 0, {"sig_sha3": tc.sha3_rows(sigs), "status": status}
    idx, z = dev(i["index"].view(np.int32)), orc.sizes(s.alg)
    ss, st = full((n, z["ss"])), status_buf(n)
    if s.op == "encaps_keyed":
        coins, c = dev(i["coins"]), full((n, z["ct"]))
        rc = lib.qrk_mlkem_encaps_keyed_batch(ctx, sets["pub"]._handle, n, idx.data_ptr(), c.data_ptr(), ss.data_ptr(),
                                              coins.data_ptr(), st.data_ptr(), stream())
        return rc, {"ct": host(c), "ss": host(ss), "status": host(st)}
    assert s.op == "decaps_keyed", s.op
    c = dev(i["ct"])
    rc = lib.qrk_mlkem_decaps_keyed_batch(ctx, sets["sec"]._handle, n, idx.data_ptr(), ss.data_ptr(), c.data_ptr(),
                                          st.data_ptr(), stream())
    return rc, {"ss": host(ss), "status": host(st)}


def adopt(ctx, obj):
    """Point a wrapper object at `ctx`; it no longer owns (or destroys) a context."""
    obj.close()
    obj._ctx = ctx
    obj.close = lambda: None
    return obj


def fail_step(lib, ctx, s):
    """The calls of thread_cases.error_thread that fail before any device work."""
    if s.op == "fail_unknown_kem":
        z = orc.sizes("ML-KEM-768")
        pk, sk, coins = full((1, z["pk"])), full((1, z["sk"])), full((1, 64), 1)
        return lib.qrk_kem_keypair_batch(ctx, s.alg.encode(), 1, pk.data_ptr(), sk.data_ptr(), coins.data_ptr(), stream()), {}
    if s.op == "fail_unknown_sig":
        pk, sig, msg, off, st = full((1, 1952)), full((1, 3309)), full((8,)), dev(np.array([0, 8], np.int64)), status_buf(1)
        return lib.qrk_sig_verify_batch(ctx, s.alg.encode(), 1, pk.data_ptr(), msg.data_ptr(), off.data_ptr(),
                                        sig.data_ptr(), None, 0, st.data_ptr(), stream()), {}
    assert s.op == "fail_wrong_width", s.op
    eng = adopt(ctx, BatchKEM(s.alg))
    try:
        eng.encaps(dev(s.inputs["pk"]))
        return 0, {"raised": [b"nothing"]}
    except ValueError as exc:
        return 0, {"raised": [type(exc).__name__.encode()]}


def do_step(lib, ctx, s, sets=None):
    """-> the step's outputs, with the call's return value and the calling thread's qrk_last_error() text."""
    if s.op in ("keypair", "encaps", "decaps", "decaps_tampered"):
        rc, got = kem_step(lib, ctx, s)
    elif s.op.startswith("sig_"):
        rc, got = sig_step(lib, ctx, s)
    elif s.op.startswith("aead_"):
        rc, got = aead_step(lib, ctx, s)
    elif s.op.endswith("_keyed"):
        rc, got = keyed_step(lib, ctx, s, sets)
    elif s.op.startswith("fail_"):
        rc, got = fail_step(lib, ctx, s)
    else:
        rc, got = small_step(lib, ctx, s)
    got["rc"], got["error"] = [rc], [lib.qrk_last_error() or b""]
    if rc != 0 and "rc" not in s.want:
        raise RuntimeError(f"{s.where()}: the call returned {rc}: {got['error'][0].decode()}")
    return got


def checked(ctx, s, sets=None, after=None):
    """A job entry: run the step, judge it; `after(step, got)` may add a verdict of its own."""
    def run(lib):
        got = do_step(lib, ctx, s, sets)
        return tc.check(s, got) or (after(s, got) if after else None)
    return run


# ------------------------------------------------------------------ the harness
@contextlib.contextmanager
def contexts(lib, count):
    hs = []
    try:
        for _ in range(count):
            h = ct.c_void_p()
            assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
            hs.append(h)
        yield hs
    finally:
        if not HUNG:
            torch.cuda.synchronize()
            for h in hs:
                lib.qrk_ctx_destroy(h)


def run_serial(lib, jobs):
    """Every entry of every job on this one thread, judged the same way: the time the join limit is sized by, and a
    first run of the same steps that has nothing to do with threads."""
    log = []
    t0 = time.monotonic()
    for k, job in enumerate(jobs):
        for entry in job:
            msg = entry(Logged(lib, log, k))
            assert msg is None, "serial: " + msg
    torch.cuda.synchronize()
    return time.monotonic() - t0


def run_jobs(lib, jobs, serial_s, own_stream=None, name=""):
    """jobs: per worker a list of entries f(lib) -> None or a message.  Returns the log of calls.  own_stream[k]:
    worker k works on a torch.cuda.Stream of its own (default: every worker does)."""
    limit = tc.T * serial_s + 30.0
    print(f"\n{name}: serial {serial_s:.2f} s, join limit {limit:.1f} s, {len(jobs)} threads, "
          f"{sum(map(len, jobs))} steps")
    log, failures = [], [None] * len(jobs)
    stop, barrier = threading.Event(), threading.Barrier(len(jobs))

    def work(k):
        try:
            st = torch.cuda.Stream() if own_stream is None or own_stream[k] else None
            with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
                logged = Logged(lib, log, k)
                barrier.wait(60)
                for entry in jobs[k]:
                    if stop.is_set():
                        return
                    msg = entry(logged)
                    if msg:
                        failures[k] = msg
                        stop.set()
                        return
                torch.cuda.current_stream().synchronize()
        except BaseException as exc:  # noqa: BLE001  (the worker's verdict, whatever it was)
            failures[k] = f"worker {k}: {exc!r}\n{traceback.format_exc()}"
            stop.set()
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,), daemon=True, name=f"{name}-{k}") for k in range(len(jobs))]
    deadline = time.monotonic() + limit
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    alive = [th.name for th in threads if th.is_alive()]
    if alive:
        global HUNG
        HUNG = True
        stop.set()
        # a hang: nothing more may be started on the GPU in this run
        pytest.exit(f"{name}: workers {alive} still running after {limit:.1f} s (serial {serial_s:.2f} s); first "
                    f"failures: {[f for f in failures if f]}", returncode=3)
    first = [f for f in failures if f]
    assert not first, "\n".join(first)
    return log


def report(name, serial_s, log):
    pairs = tc.overlaps(log)
    print(f"{name}: {len(log)} calls, {pairs} overlapping pairs of calls from different threads (serial {serial_s:.2f} s)")
    assert pairs > 0, f"{name}: no two calls from different threads overlapped: the run was serial and proves nothing"
    return pairs


# ------------------------------------------------------------------ 1. one shared context
def test_one_shared_context(lib):
    """Eight threads, one qrk_ctx: 4 rounds each of ML-KEM KeyGen -> Encaps -> Decaps with the thread's own coins at
    n = 1, 16, 17, 300, 1024, 1025, 1100, 64 (keygen_pipe / keygen_multi and their border, the one-launch kernels, the
    batched schedule), odd threads through host pointers, even ones with device tensors on a stream each; every round
    byte-exact against the oracle.  A round's Decaps uses that round's own secret key with other threads' KeyGens on
    the same context in between, so the matrix the context kept from a KeyGen (threads 5 and 6, n > 1024) is as often
    another thread's as not and must never be used for the wrong key.  Thread 4 also decapsulates its ciphertexts
    half-tampered by qrk_tamper mode 2 and expects the oracle's rejection keys."""
    plan = tc.plan("shared")
    with contexts(lib, 2) as (warm, shared):
        serial = run_serial(lib, [[checked(warm, s) for s in steps] for steps in plan])
        jobs = [[checked(shared, s) for s in steps] for steps in plan]
        log = run_jobs(lib, jobs, serial, own_stream=[t % 2 == 0 for t in range(tc.T)], name="shared context")
        report("shared context", serial, log)


# ------------------------------------------------------------------ 2. eight contexts, eight families
def test_eight_contexts_eight_families(lib):
    """A thread and a context each for ML-KEM-512 (300), ML-KEM-1024 (1100), HQC-128 (64), FrodoKEM-640-SHAKE (8),
    ML-DSA-65 (KeyGen, deterministic Sign, Verify of the fixture rows), SLH-DSA-SHA2-128f (Verify), AES-256-GCM +
    ChaCha20-Poly1305 + HKDF (aead.json, RFC 5869) and base64, three rounds each, against what each family is
    already compared with: one family's kernels must not disturb another's results."""
    plan = tc.plan("mixed")
    with contexts(lib, 2 * tc.T) as hs:
        serial = run_serial(lib, [[checked(hs[t], s) for s in steps] for t, steps in enumerate(plan)])
        jobs = [[checked(hs[tc.T + t], s) for s in steps] for t, steps in enumerate(plan)]
        log = run_jobs(lib, jobs, serial, name="eight families")
        report("eight families", serial, log)


# ------------------------------------------------------------------ 3. the default context
OQS_ALGS = ("ML-KEM-512", "ML-KEM-768", "ML-KEM-1024", "HQC-128", "FrodoKEM-640-SHAKE")
OQS_TRIPS = 6


def oqs_trip(alg, seed):
    """One single-shot round trip through qrkem.oqs.KeyEncapsulation.  The coins are the OS's, so the oracle checks
    both sides: its Decaps of the library's (sk, ct) gives the library's secret, and the library's Decaps of the
    oracle's Encaps under the generated pk gives the oracle's secret."""
    def run(lib):
        from qrkem import oqs
        z = orc.sizes(alg)
        with oqs.KeyEncapsulation(alg) as kem:
            with lib.span():
                pk = kem.generate_keypair()
            sk = kem.export_secret_key()
            with lib.span():
                c, ss = kem.encap_secret(pk)
            with lib.span():
                ss2 = kem.decap_secret(c)
            if ss2 != ss:
                return f"{alg}: decap_secret(ct) != ss"
            rows = lambda b: np.frombuffer(b, np.uint8).reshape(1, -1).copy()  # noqa: E731
            if orc.batch_decaps(alg, rows(sk), rows(c), 1)[0].tobytes() != ss:
                return f"{alg}: the oracle's Decaps of (sk, ct) is not the library's ss"
            oc, oss = orc.batch_encaps(alg, rows(pk), orc.bench_coins(1, z["encaps_coins"], seed), 1)
            with lib.span():
                ss3 = kem.decap_secret(oc[0].tobytes())
            if ss3 != oss[0].tobytes():
                return f"{alg}: the library's Decaps of the oracle's Encaps is not the oracle's ss"
        return None
    return run


def test_default_context_through_oqs(lib):
    """Eight threads, six single-shot round trips each through the one process-wide default context, the algorithms
    (three ML-KEM sets, HQC-128, FrodoKEM-640-SHAKE) in an order offset per thread, so its pinned mirror and scratch
    regrow for a larger family while other threads wait on its lock."""
    def jobs(base):
        return [[oqs_trip(OQS_ALGS[(t + j) % len(OQS_ALGS)], base + 16 * t + j) for j in range(OQS_TRIPS)]
                for t in range(tc.T)]
    serial = run_serial(lib, jobs(0x0A5))
    log = run_jobs(lib, jobs(0x1A5), serial, own_stream=[False] * tc.T, name="default context")
    report("default context", serial, log)


def test_lazy_contexts_of_shared_wrapper_objects(lib, monkeypatch):
    """Eight threads whose first act is the first call on one shared AES256GCM and one shared MLDSASignature: the
    objects create their context on first use.  Every message opens (and is what aead_spec seals under the nonce the
    library drew), every fixture signature verifies and a tampered one does not, every thread sees the same context,
    and each object created exactly one."""
    import qrkem
    from qrkem._native import LIB
    _, vrows, vstatus, _ = tc.mldsa_sets()
    created, real = [], LIB.qrk_ctx_create

    def counting(out, device):
        created.append(threading.get_ident())
        return real(out, device)

    def entries(aes, sig, t, seen):
        key, msg = bytes([t + 1]) * 32, b"thread %d says hello" % t + bytes(range(t))
        pk, m, sg = vrows[t % 4]
        bad = vrows[len(vrows) - 1 - t]

        def first(lib):
            with lib.span():
                sealed = aes.encrypt(key, msg, b"aad")
            seen.append(("aes", aes._ctx.value))
            if aead_spec.seal("AES-256-GCM", key, sealed[:12], msg, b"aad") != sealed:
                return f"thread {t}: encrypt is not AES-256-GCM of the message under the returned nonce"
            with lib.span():
                opened = aes.decrypt(key, sealed, b"aad")
            return None if opened == msg else f"thread {t}: decrypt did not return the message"

        def second(lib):
            with lib.span():
                ok = sig.verify(pk, m, sg)
            seen.append(("sig", sig._ctx.value))
            with lib.span():
                refused = sig.verify(*bad)
            return None if ok and not refused else f"thread {t}: verify gave {ok}, and {refused} for a tampered row"
        return [first, second] if t % 2 == 0 else [second, first]

    assert vstatus[:4] == [0] * 4 and vstatus[-tc.T:] == [-1] * tc.T
    aes, sig = qrkem.AES256GCM(), qrkem.MLDSASignature(3)
    serial = run_serial(lib, [entries(aes, sig, t, []) for t in range(tc.T)])
    aes.close(), sig.close()
    monkeypatch.setattr(LIB, "qrk_ctx_create", counting)
    aes, sig, seen = qrkem.AES256GCM(), qrkem.MLDSASignature(3), []
    try:
        log = run_jobs(lib, [entries(aes, sig, t, seen) for t in range(tc.T)], serial, name="lazy contexts")
        assert len(seen) == 2 * tc.T and len(set(seen)) == 2, seen
        assert len(created) == 2, f"{len(created)} contexts were created for two objects"
        report("lazy contexts", serial, log)
    finally:
        monkeypatch.undo()
        aes.close(), sig.close()


# ------------------------------------------------------------------ 4. errors stay with their thread
def test_errors_stay_with_their_thread(lib):
    """Thread A fails cleanly in turn (an unknown KEM name, a device tensor of the wrong width, an ML-KEM ek with a
    field of 3329 -> status -1, an unknown signature name, an AEAD row of 27 bytes -> status -1, an ML-DSA secret key
    with an eta field out of range -> status -1) while B runs good ML-KEM steps on the same context and C on another.
    B and C are byte-exact and never see one of A's messages in qrk_last_error(); A always sees the message of its
    own last failed call.  No hook, nothing that faults: every failure is an argument check or a status."""
    plan = tc.plan("errors")

    def clean(s, got):
        text = got["error"][0].decode()
        return f"{s.where()}: qrk_last_error() is another thread's: {text!r}" if text in tc.ERROR_TEXTS else None

    def jobs(a, c):
        return [[checked(a, s) for s in plan[0]], [checked(a, s, after=clean) for s in plan[1]],
                [checked(c, s, after=clean) for s in plan[2]]]

    with contexts(lib, 4) as hs:
        # the serial run is three threads' work in one thread, where A's messages are that thread's own: B and C are
        # judged for their bytes alone there
        serial = run_serial(lib, [[checked(hs[0], s) for s in steps] for steps in (plan[1], plan[2], plan[0])])
        log = run_jobs(lib, jobs(hs[2], hs[3]), serial, own_stream=[True, False, True], name="errors")
        report("errors", serial, log)


# ------------------------------------------------------------------ 5. profiling is per context
def profile_counts(lib, ctx):
    import qrkem
    n = lib.qrk_ctx_profile_collect(ctx)
    assert n >= 0, qrkem.last_error()
    out = {}
    for k in range(n):
        name, ms, cnt = ct.c_char_p(), ct.c_double(), ct.c_uint64()
        assert lib.qrk_ctx_profile_get(ctx, k, ct.byref(name), ct.byref(ms), ct.byref(cnt)) == 0
        out[name.value.decode()] = cnt.value
    return out


def test_profiling_is_per_context(lib):
    """qrk_ctx_profile on one context while two other threads run unprofiled contexts: the kernel names and launch
    counts collected equal those of the same steps profiled alone on one thread, taken first in this test (names and
    counts only, no times), and the unprofiled contexts collect nothing."""
    shared = tc.plan("shared")
    profiled, others = shared[5][:6] + shared[0][:3], [shared[6][:6], shared[3][:6]]  # n = 1025 and 1; 1100; 300 (host)
    with contexts(lib, 6) as hs:
        assert lib.qrk_ctx_profile(hs[0], 1) == 0
        serial = run_serial(lib, [[checked(hs[0], s) for s in profiled]] +
                            [[checked(hs[1 + k], s) for s in steps] for k, steps in enumerate(others)])
        alone = profile_counts(lib, hs[0])
        assert alone and all(c > 0 for c in alone.values()), alone
        assert lib.qrk_ctx_profile(hs[3], 1) == 0
        jobs = [[checked(hs[3], s) for s in profiled]] + [[checked(hs[4 + k], s) for s in steps] for k, steps in enumerate(others)]
        log = run_jobs(lib, jobs, serial, own_stream=[True, True, False], name="profile")
        together = profile_counts(lib, hs[3])
        print("profile: kernels and launches", together)
        assert together == alone
        assert profile_counts(lib, hs[4]) == {} and profile_counts(lib, hs[5]) == {}
        report("profile", serial, log)


# ------------------------------------------------------------------ 6. key sets
@contextlib.contextmanager
def key_sets(lib, ctx):
    keys = tc.keyed_sets()
    eng = adopt(ctx, BatchKEM("ML-KEM-768"))
    pub, sec = eng.load_public_keys(dev(keys["mlkem_pk"])), eng.load_secret_keys(dev(keys["mlkem_sk"]))
    mldsa = tk.KeySet(lib, ctx, tc.MLDSA, keys["mldsa_sk"], True)
    try:
        yield {"pub": pub, "sec": sec, "mldsa": mldsa}
    finally:
        if not HUNG:
            torch.cuda.synchronize()
            pub.close(), sec.close(), mldsa.free()


def test_key_sets_from_four_threads(lib):
    """One MLKEMKeySet pair (17 keys of tests/golden/mlkem_keyed.json: public and secret) and one secret MLDSAKeySet
    (the distinct keys of mldsa_sign.json's rows), each used by four threads at once through the context it was loaded
    on, every thread with its own row count and index pattern (i mod g, reversed, random, first / last) and a
    stream of its own: keyed Encaps and Decaps (odd rows' ciphertexts flipped) against the oracle under the gathered
    keys, keyed deterministic signing against the fixture's stored SHA3-256.
    include/qrkem.h forbids none of this: its one rule for a set, that a call on another stream be ordered behind the
    load, is met by the wrappers' synchronise after loading; the sets are freed after the join."""
    plan = tc.plan("keyed")
    with contexts(lib, 2) as (warm, shared):
        with key_sets(lib, warm) as sets:
            serial = run_serial(lib, [[checked(warm, s, sets) for s in steps] for steps in plan])
        with key_sets(lib, shared) as sets:
            log = run_jobs(lib, [[checked(shared, s, sets) for s in steps] for steps in plan], serial, name="key sets")
        report("key sets", serial, log)
