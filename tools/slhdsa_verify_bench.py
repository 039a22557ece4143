"""Batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple verification throughput on one GPU: one JSON line per name.

    python tools/slhdsa_verify_bench.py [--rows 16384] [--steps 7] [--warmup 2] [--sets NAME,...]
                                        [--out profiles/slhdsa/verify_bench.jsonl] [--commit ID]

Every row is the 2500-byte record of tests/golden/slhdsa.json (its key and message, and the spec's
signature over it, replicated: the kernels share nothing between rows, so each row costs what a distinct one
would; the data is resident before timing starts and every row verifies).  Per name: verifications/s from
warm, HIP-event-timed steps (one step = one qrk_sig_verify_batch over all rows, through
SPHINCSSignature.verify_status): the median, and the spread as min and max; the per-kernel split of one
further step from qrk_ctx_profile; the SHA-256 and SHA-512 compressions one verification costs, counted by
the spec's verifier (tests/slhdsa_spec.py, Hasher.c256 / c512) on this very input, and the compressions/s
the median implies.  Lines are appended to --out with the command and the commit.  There is no speed gate
and no CPU baseline: no other SLH-DSA implementation is at hand.
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default=",".join(spec.PARAMS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "slhdsa" / "verify_bench.jsonl"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    fixture = gold.load()
    commit = a.commit or commit_id()
    for name in a.sets.split(","):
        p, f = spec.PARAMS[name], fixture[name]
        msg = f["msgs"][-1]
        sig = spec.sign(name, f["sk"], msg)
        hs = spec.Hasher(p, f["pk"][:p.n])
        assert spec.verify_trace(name, f["pk"], msg, sig, hasher=hs)["flags"] == 0
        n = a.rows
        pk = torch.from_numpy(np.frombuffer(f["pk"], np.uint8).copy()).cuda().repeat(n, 1)
        sg = torch.from_numpy(np.frombuffer(sig, np.uint8).copy()).cuda().repeat(n, 1)
        ms = torch.from_numpy(np.frombuffer(msg, np.uint8).copy()).cuda().repeat(n)
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * len(msg)
        s = qrkem.SPHINCSSignature(LEVEL[p.n], fips205=p.fips)
        for _ in range(a.warmup):
            st = s.verify_status(pk, ms, sg, offsets=off)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0, "a row did not verify"
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = s.verify_status(pk, ms, sg, offsets=off)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        assert int(st.abs().sum()) == 0
        LIB.qrk_ctx_profile(s._ctx, 1)
        s.verify_status(pk, ms, sg, offsets=off)
        torch.cuda.synchronize()
        kernels = profile_read(s._ctx)
        LIB.qrk_ctx_profile(s._ctx, 0)
        med = statistics.median(times)
        per_s = lambda t: round(n / (t * 1e-3), 1)
        line = json.dumps({
            "bench": "slhdsa_verify", "alg": name, "rows": n, "msg_bytes": len(msg), "steps": a.steps,
            "warmup": a.warmup, "ms_per_step_median": round(med, 4), "ms_per_step_all": [round(t, 4) for t in times],
            "verifications_per_s": per_s(med), "verifications_per_s_min": per_s(max(times)),
            "verifications_per_s_max": per_s(min(times)), "kernel_ms": kernels,
            "sha256_compressions_per_row": hs.c256, "sha512_compressions_per_row": hs.c512,
            "compressions_per_s": round((hs.c256 + hs.c512) * n / (med * 1e-3), 1),
            "scratch_bytes": int(LIB.qrk_ctx_scratch_bytes(s._ctx)), "device": torch.cuda.get_device_name(0),
            "command": "python tools/slhdsa_verify_bench.py " + " ".join(sys.argv[1:]), "commit": commit})
        print(line, flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        s.close()
        del pk, sg, ms, off
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
