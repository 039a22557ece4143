"""Batched ML-DSA key generation and signing latency and throughput on one GPU: one JSON line per parameter set
and batch size.

    python tools/mldsa_sign_bench.py [--rows 1,1024,2048,4096,8192,16384] [--steps 7] [--warmup 2] [--sets NAME,...]
                                     [--out profiles/mldsa/sign_bench.jsonl] [--commit ID]

Every row signs its own 64-byte message under the key of tests/golden/mldsa_sign.json, deterministically (rnd =
32 zero bytes).  The messages differ because the cost of a row is its iteration count: a batch of equal rows
would measure one draw of it.  The data is resident before timing starts; the signatures of the warm-up step are
checked with qrk_sig_verify_batch (all rows) and the first against tests/mldsa_spec.py.  Per set and batch size:
the median ms per step and signatures/s from warm, HIP-event-timed steps (one step = one qrk_mldsa_sign_batch
through MLDSASigner.sign_batch with return_status=True, so no host wait inside the step), the spread; the same
for qrk_mldsa_keypair_batch over as many distinct xi; the per-kernel split of one further signing step from
qrk_ctx_profile; and the batch's mean and largest iteration count from qrk_dbg_mldsa_sign_trace, so that signing
cost reads as iterations x cost per iteration.  rows = 1 is the latency figure (its message is row 0 of every
batch).  The yardstick is tools/mldsa_verify_bench.py run beside it on the same machine
(profiles/mldsa/verify_bench.jsonl): there is no speed gate and no CPU baseline.
"""
from __future__ import annotations

import argparse
import ctypes as ct
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "quantum-resistant-p2p_amd", ROOT / "tests", ROOT / "tests" / "golden"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_mldsa_sign as gold  # noqa: E402
import mldsa_spec as spec  # noqa: E402
import qrkem  # noqa: E402
from qrkem._debug import bind  # noqa: E402

LIB = bind()
LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}
MSG_BYTES = 64


def profile_read(ctx) -> dict:
    out = {}
    for i in range(max(LIB.qrk_ctx_profile_collect(ctx), 0)):
        name, ms, cnt = ct.c_char_p(), ct.c_double(), ct.c_uint64()
        LIB.qrk_ctx_profile_get(ctx, i, ct.byref(name), ct.byref(ms), ct.byref(cnt))
        out[name.value.decode()] = round(ms.value, 4)
    return out


def commit_id() -> str:
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def timed(steps: int, call) -> list:
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def iterations(s, sk, ms, off, n: int):
    """(mean, max) of the iterations the rows of this batch run: one traced call."""
    sig = torch.empty((n, s.signature_size), dtype=torch.uint8, device="cuda")
    status = torch.empty((n,), dtype=torch.int32, device="cuda")
    mu = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    iters = torch.empty((n,), dtype=torch.int32, device="cuda")
    rc = LIB.qrk_dbg_mldsa_sign_trace(s._context(), s.variant.encode(), n, sk.data_ptr(), ms.data_ptr(), off.data_ptr(),
                                      None, None, 0, sig.data_ptr(), status.data_ptr(), 814, mu.data_ptr(),
                                      iters.data_ptr(), s._stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    return round(float(iters.float().mean()), 3), int(iters.max())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,1024,2048,4096,8192,16384")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default=",".join(gold.NAMES))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mldsa" / "sign_bench.jsonl"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    fixture = gold.load()
    commit = a.commit or commit_id()
    rows = [int(x) for x in a.rows.split(",")]
    rng = np.random.default_rng(204)
    all_msgs = rng.integers(0, 256, size=(max(rows), MSG_BYTES), dtype=np.uint8)
    all_xi = rng.integers(0, 256, size=(max(rows), 32), dtype=np.uint8)
    for name in a.sets.split(","):
        f = fixture[name]
        want = spec.sign(f["sk"], all_msgs[0].tobytes())
        s = qrkem.MLDSASigner(LEVEL[name], deterministic=True)
        for n in rows:
            sk = torch.from_numpy(np.frombuffer(f["sk"], np.uint8).copy()).cuda().repeat(n, 1)
            pk = torch.from_numpy(np.frombuffer(f["pk"], np.uint8).copy()).cuda().repeat(n, 1)
            ms = torch.from_numpy(all_msgs[:n].reshape(-1).copy()).cuda()
            xi = torch.from_numpy(all_xi[:n].copy()).cuda()
            off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * MSG_BYTES
            for _ in range(a.warmup):
                sg, st = s.sign_batch(sk, ms, offsets=off, return_status=True)
                s.generate_keypair_batch(n, seeds=xi)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0 and sg[0].cpu().numpy().tobytes() == want, "wrong signature"
            assert int(s.verify_status(pk, ms, sg, offsets=off).abs().sum()) == 0, "a signature does not verify"
            times = timed(a.steps, lambda: s.sign_batch(sk, ms, offsets=off, return_status=True))
            kg_times = timed(a.steps, lambda: s.generate_keypair_batch(n, seeds=xi))
            LIB.qrk_ctx_profile(s._ctx, 1)
            s.sign_batch(sk, ms, offsets=off, return_status=True)
            torch.cuda.synchronize()
            kernels = profile_read(s._ctx)
            LIB.qrk_ctx_profile(s._ctx, 0)
            mean_iters, max_iters = iterations(s, sk, ms, off, n)
            med, kg_med = statistics.median(times), statistics.median(kg_times)
            per_s = lambda t: round(n / (t * 1e-3), 1)
            line = json.dumps({
                "bench": "mldsa_sign", "alg": name, "rows": n, "msg_bytes": MSG_BYTES, "steps": a.steps,
                "warmup": a.warmup, "ms_per_step_median": round(med, 4),
                "ms_per_step_all": [round(t, 4) for t in times], "signatures_per_s": per_s(med),
                "signatures_per_s_min": per_s(max(times)), "signatures_per_s_max": per_s(min(times)),
                "iterations_mean": mean_iters, "iterations_max": max_iters,
                "us_per_iteration_row": round(med * 1e3 / (n * mean_iters), 3),
                "keygen_ms_per_step_median": round(kg_med, 4), "keygen_ms_per_step_all": [round(t, 4) for t in kg_times],
                "keypairs_per_s": per_s(kg_med), "kernel_ms": kernels,
                "scratch_bytes": int(LIB.qrk_ctx_scratch_bytes(s._ctx)), "device": torch.cuda.get_device_name(0),
                "command": "python tools/mldsa_sign_bench.py " + " ".join(sys.argv[1:]), "commit": commit})
            print(line, flush=True)
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
            del sk, pk, ms, xi, off, sg, st
            torch.cuda.empty_cache()
        s.close()


if __name__ == "__main__":
    main()
