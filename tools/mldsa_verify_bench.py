"""Batched ML-DSA.Verify throughput on one GPU: one JSON line per parameter set.

    python tools/mldsa_verify_bench.py [--rows 65536] [--steps 5] [--warmup 2] [--sets ML-DSA-44,...]

Every row is the 2500-byte record of tests/golden/mldsa.json (its key, message and signature
replicated: the kernels share nothing between rows, so each row costs what a distinct one would; the
data is resident before timing starts).  Per set: verifications/s from warm, HIP-event-timed steps
(median; one step = one qrk_sig_verify_batch over all rows, through MLDSASignature.verify_status), the
per-kernel split of one further step from qrk_ctx_profile, the Keccak-f[1600] permutations a row costs
and their rate as a fraction of the 45.3 T/s Keccak-loop ceiling measured for this project.
There is no speed gate and no CPU baseline: no other ML-DSA implementation is at hand.
"""
from __future__ import annotations

import argparse
import ctypes as ct
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "quantum-resistant-p2p_amd", ROOT / "tests", ROOT / "tests" / "golden"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_mldsa as gold  # noqa: E402
import mldsa_spec as spec  # noqa: E402
import qrkem  # noqa: E402
from qrkem._native import LIB  # noqa: E402

# permutations/s: 45.3 T VALU lane-instructions/s in the Keccak loop, 4320 per permutation (csrc/keccak.cuh)
KECCAK_CEILING = 45.3e12 / 4320
LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}


def permutations_per_row(p, msg_len: int, ctx_len: int = 0) -> dict:
    blocks = lambda n: n // 136 + 1  # SHAKE256 absorb of n bytes, padding included
    return {"expand_a": p.k * p.l * 5, "tr": blocks(p.pk), "mu": blocks(64 + 2 + ctx_len + msg_len),
            "sample_in_ball": 1, "ctilde": blocks(64 + p.w1)}


def profile_read(ctx) -> dict:
    out = {}
    for i in range(max(LIB.qrk_ctx_profile_collect(ctx), 0)):
        name, ms, cnt = ct.c_char_p(), ct.c_double(), ct.c_uint64()
        LIB.qrk_ctx_profile_get(ctx, i, ct.byref(name), ct.byref(ms), ct.byref(cnt))
        out[name.value.decode()] = round(ms.value, 4)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default=",".join(LEVEL))
    a = ap.parse_args()
    fixture = gold.load()
    for name in a.sets.split(","):
        p, f = spec.PARAMS[name], fixture[name]
        msg, sig = f["msgs"][3], f["sigs"][3]
        n = a.rows
        pk = torch.from_numpy(np.frombuffer(f["pk"], np.uint8).copy()).cuda().repeat(n, 1)
        sg = torch.from_numpy(np.frombuffer(sig, np.uint8).copy()).cuda().repeat(n, 1)
        ms = torch.from_numpy(np.frombuffer(msg, np.uint8).copy()).cuda().repeat(n)
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * len(msg)
        s = qrkem.MLDSASignature(LEVEL[name])
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
        perms = permutations_per_row(p, len(msg))
        total = sum(perms.values())
        expand_rate = perms["expand_a"] * n / (kernels["k_mldsa_expand"] * 1e-3) if kernels.get("k_mldsa_expand") else None
        print(json.dumps({
            "bench": "mldsa_verify", "alg": name, "rows": n, "msg_bytes": len(msg), "steps": a.steps, "warmup": a.warmup,
            "ms_per_step_median": round(med, 4), "ms_per_step_all": [round(t, 4) for t in times],
            "verifications_per_s": round(n / (med * 1e-3), 1), "kernel_ms": kernels,
            "keccak_permutations_per_row": total, "keccak_permutations_split": perms,
            "keccak_fraction_of_ceiling": round(total * n / (med * 1e-3) / KECCAK_CEILING, 4),
            "expand_kernel_fraction_of_ceiling": round(expand_rate / KECCAK_CEILING, 4) if expand_rate else None,
            "scratch_bytes": int(LIB.qrk_ctx_scratch_bytes(s._ctx)), "device": torch.cuda.get_device_name(0)}))
        s.close()
        del pk, sg, ms, off
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
