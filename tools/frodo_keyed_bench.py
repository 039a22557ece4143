"""FrodoKEM key sets against the per-row calls on the same keys and mu, on one GPU: one JSON line per variant, row
count, set size and operation.

    python tools/frodo_keyed_bench.py [--sets NAME,...] [--rows 4096,chunk] [--keys 1,64] [--repeats 5] [--steps 5]
                                      [--warmup 2] [--out profiles/frodo_keyed/bench.jsonl] [--commit ID]

`chunk` among the row counts is the largest number of rows the per-row call runs as one chunk for that variant
(BatchKEM.effective_chunk: the scratch budget divided by the per-row scratch).  For every case g keys are generated on
the GPU and every row draws its key: key 0 for g = 1, a fixed-seed random draw for g = 64.  The per-row call gets the
gathered pk / sk rows, the keyed call the set and the index; both write into buffers allocated before timing, and
their outputs are compared byte for byte before timing starts.

The calls under comparison run in one process, interleaved: each of --repeats rounds times --steps warm steps of the
per-row call, then of the keyed call (HIP events around one call, no host wait inside).  A call's figure is the mean
over the rounds of the round's mean step, and `round_means_ms` shows every round; `spread_ms` is the larger of the two
calls' max - min over their round means, the noise a difference has to clear, and `faster` says whether the keyed
call's mean step is below the per-row call's by more than that.  `kernel_ms` is the per-kernel split of one further
step of each call from qrk_ctx_profile, taken after the timed rounds, and `sampler_share` the part of the keyed step
in the sampler stream (k_fr_se_stream); `load_ms` is one load of the set and `load_ms_per_key` that over g (not part
of a step, not tuned).  There is no CPU baseline and no gate: the per-row call beside it is the yardstick.
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
sys.path.insert(0, str(ROOT / "quantum-resistant-p2p_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import qrkem  # noqa: E402
from qrkem._native import LIB  # noqa: E402
from qrkem.batch import FrodoBatchKEM  # noqa: E402

ALGS = ("FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE", "FrodoKEM-640-AES", "FrodoKEM-976-AES",
        "FrodoKEM-1344-AES")


def ptr(t):
    return ct.c_void_p(t.data_ptr())


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
    for call in calls.values():
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    out = {name: {"all": [], "means": []} for name in calls}
    for _ in range(a.repeats):
        for name, call in calls.items():
            t = timed(a.steps, call)
            out[name]["all"] += [round(x, 4) for x in t]
            out[name]["means"].append(round(statistics.fmean(t), 4))
    return {name: {"ms_per_step_mean": round(statistics.fmean(v["means"]), 4), "round_means_ms": v["means"],
                   "ms_per_step_all": v["all"]} for name, v in out.items()}


def kernels_of(eng, call) -> dict:
    eng.profile(True)
    call()
    torch.cuda.synchronize()
    k = {name: round(ms, 4) for name, (ms, _) in eng.profile_read().items()}
    eng.profile(False)
    return k


def measured_args() -> list:
    """The command line without --out and its value: where the lines go is no part of what was measured."""
    args, skip = [], False
    for x in sys.argv[1:]:
        if skip or x.startswith("--out="):
            skip = False
        elif x == "--out":
            skip = True
        else:
            args.append(x)
    return args


def emit(a, record: dict) -> None:
    record.update({"repeats": a.repeats, "steps": a.steps, "warmup": a.warmup,
                   "device": torch.cuda.get_device_name(0),
                   "command": "python tools/frodo_keyed_bench.py " + " ".join(measured_args()), "commit": a.commit})
    line = json.dumps(record)
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


def compare(a, eng, op: str, n: int, g: int, index_kind: str, calls: dict, extra: dict) -> None:
    t = interleaved(calls, a)
    kernels = {k: kernels_of(eng, call) for k, call in calls.items()}
    spread = round(max(max(v["round_means_ms"]) - min(v["round_means_ms"]) for v in t.values()), 4)
    base, keyed = t["per_row"]["ms_per_step_mean"], t["keyed"]["ms_per_step_mean"]
    step = sum(kernels["keyed"].values())
    extra = dict(extra, sampler_share=round(kernels["keyed"].get("k_fr_se_stream", 0.0) / step, 3) if step else None)
    record = {"bench": "frodo_keyed_" + op, "alg": eng.alg, "rows": n, "keys": g, "index": index_kind,
              "per_row": t["per_row"], "keyed": t["keyed"], "spread_ms": spread, "gain_ms": round(base - keyed, 4),
              "faster": bool(base - keyed > spread), "speedup": round(base / keyed, 3),
              "rows_per_s_per_row": round(n / (base * 1e-3), 1), "rows_per_s_keyed": round(n / (keyed * 1e-3), 1),
              "kernel_ms": kernels, "scratch_bytes": eng.scratch_bytes}
    record.update(extra)
    emit(a, record)


def load_ms(load) -> tuple:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ks = load()
    e1.record()
    e1.synchronize()
    return ks, round(e0.elapsed_time(e1), 4)


def bench_case(a, alg: str, n: int, g: int, rows_kind: str) -> None:
    eng = FrodoBatchKEM(alg, device=0)
    st = eng._stream()
    pk_g, sk_g = eng.keypair(coins=eng.bench_coins(g, eng.kp_coins, seed=0x4B45 + g))
    coins = eng.bench_coins(n, eng.enc_coins, seed=0x454E + n)
    if g == 1:
        index_kind = "key 0"
        index = torch.zeros(n, dtype=torch.int32, device="cuda")
    else:
        index_kind = "random"
        index = torch.from_numpy(np.random.default_rng(203).integers(0, g, n, dtype=np.int32)).cuda()
    pk = pk_g[index.long()].contiguous()  # the per-row calls' inputs: every row carries its key
    sk = sk_g[index.long()].contiguous()
    out = {k: (eng._empty(n, eng.ct_len), eng._empty(n, eng.ss_len),
               torch.empty((n,), dtype=torch.int32, device="cuda")) for k in ("per_row", "keyed")}
    pub, pub_ms = load_ms(lambda: eng.load_public_keys(pk_g))
    sec, sec_ms = load_ms(lambda: eng.load_secret_keys(sk_g))

    def check(rc):
        assert rc == 0, qrkem.last_error()

    (c0, s0, t0), (c1, s1, t1) = out["per_row"], out["keyed"]
    enc = {"per_row": lambda: check(LIB.qrk_kem_encaps_batch(eng._ctx, eng._name, n, ptr(c0), ptr(s0), ptr(pk),
                                                             ptr(coins), ptr(t0), st)),
           "keyed": lambda: check(LIB.qrk_frodo_encaps_keyed_batch(eng._ctx, pub._handle, n, ptr(index), ptr(c1),
                                                                   ptr(s1), ptr(coins), ptr(t1), st))}
    for call in enc.values():
        call()
    assert torch.equal(c0, c1) and torch.equal(s0, s1) and torch.equal(t0, t1), "Encaps: keyed differs from per-row"
    shape = {"rows_kind": rows_kind, "per_row_chunk": eng.effective_chunk}
    compare(a, eng, "encaps", n, g, index_kind, enc,
            dict(shape, keyset_bytes=pub.device_bytes, load_ms=pub_ms, load_ms_per_key=round(pub_ms / g, 4)))
    dec = {"per_row": lambda: check(LIB.qrk_kem_decaps_batch_status(eng._ctx, eng._name, n, ptr(s0), ptr(c0), ptr(sk),
                                                                    ptr(t0), st)),
           "keyed": lambda: check(LIB.qrk_frodo_decaps_keyed_batch(eng._ctx, sec._handle, n, ptr(index), ptr(s1),
                                                                   ptr(c0), ptr(t1), st))}
    want = s0.clone()
    for call in dec.values():
        call()
    assert torch.equal(s0, want) and torch.equal(s1, want) and torch.equal(t0, t1), "Decaps: keyed differs from per-row"
    compare(a, eng, "decaps", n, g, index_kind, dec,
            dict(shape, keyset_bytes=sec.device_bytes, load_ms=sec_ms, load_ms_per_key=round(sec_ms / g, 4)))
    pub.close()
    sec.close()
    eng.close()
    del pk, sk, out, coins, index
    torch.cuda.empty_cache()


def chunk_rows(alg: str) -> int:
    eng = FrodoBatchKEM(alg, device=0)
    try:
        return eng.effective_chunk
    finally:
        eng.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default=",".join(ALGS))
    ap.add_argument("--rows", default="4096,chunk")
    ap.add_argument("--keys", default="1,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frodo_keyed" / "bench.jsonl"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    a.commit = a.commit or commit_id()
    if not torch.cuda.is_available():
        sys.exit("tools/frodo_keyed_bench.py needs a GPU: there is nothing to time without one")
    for alg in a.sets.split(","):
        for rows in a.rows.split(","):
            n = chunk_rows(alg) if rows == "chunk" else int(rows)
            for g in (int(x) for x in a.keys.split(",")):
                bench_case(a, alg, n, g, "one chunk of the per-row call" if rows == "chunk" else "fixed")


if __name__ == "__main__":
    main()
