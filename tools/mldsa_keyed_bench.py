"""ML-DSA key sets against the per-row calls on the same rows, on one GPU: one JSON line per parameter set and case.

    python tools/mldsa_keyed_bench.py [--sets NAME,...] [--cases verify,sign] [--repeats 5] [--steps 5] [--warmup 2]
                                      [--verify-rows 65536] [--sign-rows 16384,1]
                                      [--out profiles/mldsa/keyed_bench.jsonl] [--commit ID]

Verification: --verify-rows rows of 2500-byte messages under g = 1 and g = 64 keys (row i under key i mod g), the
signatures made on the GPU and checked by both calls before timing starts.  Signing: --sign-rows rows of distinct
64-byte messages under one key, deterministic (rnd = 32 zero bytes), for the per-row call and for both forms of the
keyed core (the NTT'd secret vectors held in LDS, or read from the set in every iteration).

The calls under comparison run in one process, interleaved: each of --repeats rounds times --steps warm steps of the
per-row call, then of each keyed variant (HIP events around one call, no host wait inside).  A variant's figure is
the median over the rounds of the round's median step; `spread_ms` is max - min of the per-row round medians, the
noise any difference has to clear.  `kernel_ms` is the per-kernel split of one further step of each call from
qrk_ctx_profile, taken after the timed rounds.  The signing lines carry the batch's mean iteration count
(qrk_dbg_mldsa_sign_trace), since time per signature scales with it.  There is no CPU baseline and no gate: the
per-row call beside it is the yardstick.
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

import qrkem  # noqa: E402
from qrkem._debug import bind  # noqa: E402

LIB = bind()
LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}
VERIFY_MSG_BYTES, SIGN_MSG_BYTES = 2500, 64
SIGN_MODES = {"keyed_lds": 1, "keyed_l2": 2}


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


def interleaved(calls: dict, a) -> dict:
    """name -> {"all": every step in ms, round by round; "medians": one per round}, the variants taking turns."""
    for call in calls.values():
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    out = {name: {"all": [], "medians": []} for name in calls}
    for _ in range(a.repeats):
        for name, call in calls.items():
            t = timed(a.steps, call)
            out[name]["all"] += [round(x, 4) for x in t]
            out[name]["medians"].append(round(statistics.median(t), 4))
    return out


def kernels_of(s, call) -> dict:
    LIB.qrk_ctx_profile(s._ctx, 1)
    call()
    torch.cuda.synchronize()
    k = profile_read(s._ctx)
    LIB.qrk_ctx_profile(s._ctx, 0)
    return k


def emit(a, record: dict) -> None:
    record.update({"repeats": a.repeats, "steps": a.steps, "warmup": a.warmup,
                   "device": torch.cuda.get_device_name(0),
                   "command": "python tools/mldsa_keyed_bench.py " + " ".join(sys.argv[1:]), "commit": a.commit})
    line = json.dumps(record)
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


def summary(t: dict) -> dict:
    out = {}
    for name, v in t.items():
        out[name] = {"ms_per_step_median": round(statistics.median(v["medians"]), 4), "round_medians_ms": v["medians"],
                     "ms_per_step_all": v["all"]}
    return out


def bench_verify(a, name: str, s, rng) -> None:
    n = a.verify_rows
    pk64, sk64 = s.generate_keypair_batch(64, seeds=rng.integers(0, 256, size=(64, 32), dtype=np.uint8))
    ms = torch.from_numpy(rng.integers(0, 256, size=n * VERIFY_MSG_BYTES, dtype=np.uint8)).cuda()
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * VERIFY_MSG_BYTES
    for g in (1, 64):
        index = (torch.arange(n, dtype=torch.int32, device="cuda") % g).contiguous()
        with s.load_secret_keys(sk64[:g].contiguous()) as sec, s.load_public_keys(pk64[:g].contiguous()) as pub:
            sig, st = s.sign_keyed(sec, ms, index, offsets=off, return_status=True)
            assert int(st.abs().sum()) == 0, "a row was not signed"
            pk = pk64[:g][index.long()].contiguous()  # the per-row call's input: every row carries its key
            calls = {"per_row": lambda: s.verify_status(pk, ms, sig, offsets=off),
                     "keyed": lambda: s.verify_keyed_status(pub, ms, sig, index, offsets=off)}
            for call in calls.values():
                assert int(call().abs().sum()) == 0, "a signature does not verify"
            t = summary(interleaved(calls, a))
            kernels = {k: kernels_of(s, call) for k, call in calls.items()}
            rounds = t["per_row"]["round_medians_ms"]
            spread = round(max(rounds) - min(rounds), 4)
            gain = round(t["per_row"]["ms_per_step_median"] - t["keyed"]["ms_per_step_median"], 4)
            expand = kernels["per_row"].get("k_mldsa_expand", 0.0)
            emit(a, {"bench": "mldsa_keyed_verify", "alg": name, "rows": n, "keys": g, "msg_bytes": VERIFY_MSG_BYTES,
                     "per_row": t["per_row"], "keyed": t["keyed"], "spread_ms": spread, "gain_ms": gain,
                     "per_row_expand_ms": expand, "gain_target_ms": round(expand - spread, 4),
                     "target_met": bool(gain >= expand - spread),
                     "speedup": round(t["per_row"]["ms_per_step_median"] / t["keyed"]["ms_per_step_median"], 3),
                     "verifications_per_s_keyed": round(n / (t["keyed"]["ms_per_step_median"] * 1e-3), 1),
                     "kernel_ms": kernels, "keyset_bytes": pub.device_bytes,
                     "scratch_bytes": int(LIB.qrk_ctx_scratch_bytes(s._ctx))})
            del pk, sig, st
        torch.cuda.empty_cache()


def iterations(s, sk, ms, off, n: int) -> float:
    sig = torch.empty((n, s.signature_size), dtype=torch.uint8, device="cuda")
    status = torch.empty((n,), dtype=torch.int32, device="cuda")
    mu = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    iters = torch.empty((n,), dtype=torch.int32, device="cuda")
    rc = LIB.qrk_dbg_mldsa_sign_trace(s._context(), s.variant.encode(), n, sk.data_ptr(), ms.data_ptr(), off.data_ptr(),
                                      None, None, 0, sig.data_ptr(), status.data_ptr(), 814, mu.data_ptr(),
                                      iters.data_ptr(), s._stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    return round(float(iters.float().mean()), 3)


def bench_sign(a, name: str, s, rng) -> None:
    default_mode = LIB.qrk_dbg_mldsa_keyed_sign_mode(0)
    rows = [int(x) for x in a.sign_rows.split(",")]
    _, sk1 = s.generate_keypair_batch(1, seeds=rng.integers(0, 256, size=(1, 32), dtype=np.uint8))
    all_msgs = rng.integers(0, 256, size=(max(rows), SIGN_MSG_BYTES), dtype=np.uint8)
    with s.load_secret_keys(sk1) as sec:
        for n in rows:
            sk = sk1.repeat(n, 1)
            ms = torch.from_numpy(all_msgs[:n].reshape(-1).copy()).cuda()
            off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * SIGN_MSG_BYTES

            def keyed(mode):
                def call():
                    LIB.qrk_dbg_mldsa_keyed_sign_mode(mode)
                    return s.sign_keyed(sec, ms, offsets=off, return_status=True)
                return call
            calls = {"per_row": lambda: s.sign_batch(sk, ms, offsets=off, return_status=True)}
            calls.update({k: keyed(m) for k, m in SIGN_MODES.items()})
            want, st = calls["per_row"]()
            assert int(st.abs().sum()) == 0
            for k in SIGN_MODES:
                got, st = calls[k]()
                assert int(st.abs().sum()) == 0 and torch.equal(got, want), f"{k}: signatures differ from per-row"
            t = summary(interleaved(calls, a))
            kernels = {k: kernels_of(s, call) for k, call in calls.items()}
            rounds = t["per_row"]["round_medians_ms"]
            spread = round(max(rounds) - min(rounds), 4)
            base = t["per_row"]["ms_per_step_median"]
            record = {"bench": "mldsa_keyed_sign", "alg": name, "rows": n, "keys": 1, "msg_bytes": SIGN_MSG_BYTES,
                      "iterations_mean": iterations(s, sk, ms, off, n), "spread_ms": spread,
                      "default_variant": [k for k, m in SIGN_MODES.items() if m == default_mode][0], "per_row": t["per_row"]}
            for k in SIGN_MODES:
                record[k] = t[k]
                record[k]["gain_ms"] = round(base - t[k]["ms_per_step_median"], 4)
                record[k]["not_slower"] = bool(t[k]["ms_per_step_median"] <= base + spread)
                record[k]["signatures_per_s"] = round(n / (t[k]["ms_per_step_median"] * 1e-3), 1)
            record.update({"kernel_ms": kernels, "keyset_bytes": sec.device_bytes,
                           "scratch_bytes": int(LIB.qrk_ctx_scratch_bytes(s._ctx))})
            emit(a, record)
            del sk, ms, off, want, got, st
            torch.cuda.empty_cache()
    LIB.qrk_dbg_mldsa_keyed_sign_mode(0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default=",".join(LEVEL))
    ap.add_argument("--cases", default="verify,sign")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--verify-rows", type=int, default=1 << 16)
    ap.add_argument("--sign-rows", default="16384,1")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mldsa" / "keyed_bench.jsonl"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    a.commit = a.commit or commit_id()
    if not torch.cuda.is_available():
        sys.exit("tools/mldsa_keyed_bench.py needs a GPU: there is nothing to time without one")
    for name in a.sets.split(","):
        s = qrkem.MLDSASigner(LEVEL[name], deterministic=True)
        rng = np.random.default_rng(204)
        if "verify" in a.cases.split(","):
            bench_verify(a, name, s, rng)
        if "sign" in a.cases.split(","):
            bench_sign(a, name, s, rng)
        s.close()


if __name__ == "__main__":
    main()
