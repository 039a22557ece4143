"""Batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple signing latency and throughput on one GPU: one JSON line per
name and batch size.

    python tools/slhdsa_sign_bench.py [--rows 1,256,4096] [--steps 7] [--warmup 2] [--sets NAME,...]
                                      [--out profiles/slhdsa/sign_bench.jsonl] [--commit ID]

Every row signs the 2500-byte message of tests/golden/slhdsa.json under the fixture key, deterministically
(opt_rand = PK.seed), replicated: the kernels share nothing between rows, so each row costs what a distinct one
would; the data is resident before timing starts, the first signature is checked against the stored SHA3-256
and all rows are checked equal.  Per name and batch size: the median ms per step and signatures/s from warm,
HIP-event-timed steps (one step = one qrk_sig_sign_batch through SPHINCSSignature.sign_batch with
return_status=True, so no host wait inside the step), the spread; the per-kernel split of one further step
from qrk_ctx_profile; the SHA-2 compressions one signature costs, counted by the spec's Hasher over the same
signature computed outside the timed region, and the compressions/s the median implies.  rows = 1 is the
latency figure.  The yardstick is tools/slhdsa_verify_bench.py run beside it on the same machine: there is no
speed gate and no CPU baseline.
"""
from __future__ import annotations

import argparse
import ctypes as ct
import hashlib
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

import make_golden_slhdsa as gold  # noqa: E402
import slhdsa_spec as spec  # noqa: E402
import qrkem  # noqa: E402
from qrkem._native import LIB  # noqa: E402

LEVEL = {16: 1, 24: 3, 32: 5}


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


def sign_cost(name: str, sk: bytes, msg: bytes):
    """(c256, c512) of one spec signature: spec.sign with a counting Hasher."""
    made = []
    real = spec.Hasher

    class Counting(real):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

    spec.Hasher = Counting
    try:
        sig = spec.sign(name, sk, msg)
    finally:
        spec.Hasher = real
    return sig, sum(h.c256 for h in made), sum(h.c512 for h in made)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,256,4096")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default=",".join(spec.PARAMS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "slhdsa" / "sign_bench.jsonl"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    fixture = gold.load()
    commit = a.commit or commit_id()
    for name in a.sets.split(","):
        p, f = spec.PARAMS[name], fixture[name]
        msg = f["msgs"][-1]
        want, c256, c512 = sign_cost(name, f["sk"], msg)
        assert hashlib.sha3_256(want).hexdigest() == f["records"][-1]["sig_sha3"]
        s = qrkem.SPHINCSSignature(LEVEL[p.n], fips205=p.fips, signing=True, deterministic=True)
        for n in (int(x) for x in a.rows.split(",")):
            sk = torch.from_numpy(np.frombuffer(f["sk"], np.uint8).copy()).cuda().repeat(n, 1)
            ms = torch.from_numpy(np.frombuffer(msg, np.uint8).copy()).cuda().repeat(n)
            off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * len(msg)
            for _ in range(a.warmup):
                sg, st = s.sign_batch(sk, ms, offsets=off, return_status=True)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0 and sg[0].cpu().numpy().tobytes() == want, "wrong signature"
            assert bool((sg == sg[0]).all()), "rows differ"
            times = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sg, st = s.sign_batch(sk, ms, offsets=off, return_status=True)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            assert int(st.abs().sum()) == 0
            LIB.qrk_ctx_profile(s._ctx, 1)
            s.sign_batch(sk, ms, offsets=off, return_status=True)
            torch.cuda.synchronize()
            kernels = profile_read(s._ctx)
            LIB.qrk_ctx_profile(s._ctx, 0)
            med = statistics.median(times)
            per_s = lambda t: round(n / (t * 1e-3), 1)
            line = json.dumps({
                "bench": "slhdsa_sign", "alg": name, "rows": n, "msg_bytes": len(msg), "steps": a.steps,
                "warmup": a.warmup, "ms_per_step_median": round(med, 4),
                "ms_per_step_all": [round(t, 4) for t in times], "signatures_per_s": per_s(med),
                "signatures_per_s_min": per_s(max(times)), "signatures_per_s_max": per_s(min(times)),
                "kernel_ms": kernels, "sha256_compressions_per_row": c256, "sha512_compressions_per_row": c512,
                "compressions_per_s": round((c256 + c512) * n / (med * 1e-3), 1),
                "scratch_bytes": int(LIB.qrk_ctx_scratch_bytes(s._ctx)), "device": torch.cuda.get_device_name(0),
                "command": "python tools/slhdsa_sign_bench.py " + " ".join(sys.argv[1:]), "commit": commit})
            print(line, flush=True)
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
            del sk, ms, off, sg, st
            torch.cuda.empty_cache()
        s.close()


if __name__ == "__main__":
    main()
