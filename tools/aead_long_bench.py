"""The long AEAD calls against the one-lane calls on the same rows, on one GPU: where `long_min_bytes` comes from.

    python tools/aead_long_bench.py [--algs NAME,...] [--repeats 7] [--warmup 2] [--rows 64]
                                    [--out profiles/aead_long/bench.jsonl] [--commit ID]

One process interleaves qrk_aead_seal_batch / qrk_aead_open_batch ("lane": one lane per row) and
qrk_aead_seal_long_batch / qrk_aead_open_long_batch ("long": one row across many workgroups) over device
buffers: both AEADs, Seal and Open, one row of 4 KiB ... 64 MiB in steps of 4, a 13-byte aad.  A point is the
median of --repeats timed calls (HIP events around one call, no host wait inside) after --warmup calls of each,
the two calls taking turns; the outputs are compared byte for byte before anything is timed.  Where one call of
the one-lane path takes more than a second it is not timed at that size or any larger one, and the line says so
(`lane_skipped`).  The 64 MiB lines carry the long call's rate beside a device-to-device copy of the same bytes,
for orientation only: the calls are compute-bound.

The last lines: `threshold`, the smallest measured size from which the long call is faster than the one-lane
call at every larger measured size, for Seal and for Open of every algorithm timed (sizes are powers of two, so
it is one already), which is what qrkem.symmetric.LONG_MIN_BYTES must equal; and per algorithm one line of
--rows rows of that size through both paths, to show whether the routing rule needs a bound on n.  Run it under
one `timeout`.  There is no gate: the one-lane call beside it is the yardstick.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "quantum-resistant-p2p_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from qrkem.handshake import PackedInfos  # noqa: E402
from qrkem.symmetric import BY_NAME, PackedRows, open_rows, open_rows_long, seal_rows, seal_rows_long  # noqa: E402

SIZES = [4 << 10 << (2 * k) for k in range(8)]  # 4 KiB ... 64 MiB
AAD = b"message-id-13"
LANE_LIMIT_MS = 1000.0


def commit_id() -> str:
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def once(call) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(calls: dict, a) -> dict:
    """name -> every timed call in ms, the variants taking turns after the warm-up of each."""
    for call in calls.values():
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    out = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, call in calls.items():
            out[name].append(round(once(call), 4))
    return out


def copy_gbps(nbytes: int, a) -> float:
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(a.warmup):
        dst.copy_(src)
    t = statistics.median(once(lambda: dst.copy_(src)) for _ in range(a.repeats))
    return round(nbytes / (t * 1e-3) / 1e9, 1)


class Case:
    """n rows of `size` bytes under n keys on the device, sealed once by the one-lane call (or, where that is
    skipped, by the long call) so that Open has something to open."""

    def __init__(self, alg: str, n: int, size: int, rng):
        self.alg, self.n, self.size = alg, n, size
        self.c = BY_NAME[alg](device=0)
        self.ctx = self.c._context()
        self.keys = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
        self.nonces = torch.from_numpy(rng.integers(0, 256, size=(n, 12), dtype=np.uint8)).cuda()
        self.rows = PackedRows.from_matrix(torch.from_numpy(rng.integers(0, 256, size=(n, size), dtype=np.uint8)).cuda())
        self.aad = PackedInfos(AAD, n, 0)
        self.sealed = None

    def seal(self, long: bool):
        if long:
            return seal_rows_long(self.ctx, self.alg, 0, self.keys, self.rows, self.aad, self.nonces, self.size)
        return seal_rows(self.ctx, self.alg, 0, self.keys, self.rows, self.aad, self.nonces)

    def open(self, long: bool):
        if long:
            return open_rows_long(self.ctx, self.alg, 0, self.keys, self.sealed, self.aad, self.size)
        return open_rows(self.ctx, self.alg, 0, self.keys, self.sealed, self.aad)

    def measure(self, a, lane: bool) -> dict:
        """{"seal": {...}, "open": {...}}; lane False: only the long call is timed."""
        self.sealed = self.seal(True)
        if lane:
            assert torch.equal(self.seal(False).data, self.sealed.data), "Seal: the two paths differ"
        out = {}
        for op, fn in (("seal", self.seal), ("open", self.open)):
            if op == "open":
                plain, status = self.open(True)
                want = self.rows.data[:self.n * self.size]
                assert int(status.abs().sum()) == 0 and torch.equal(plain.data[:want.numel()], want), "Open (long) failed"
                if lane:
                    plain, status = self.open(False)
                    assert int(status.abs().sum()) == 0 and torch.equal(plain.data[:want.numel()], want), "Open failed"
            calls = {"long": lambda fn=fn: fn(True)}
            if lane:
                calls["lane"] = lambda fn=fn: fn(False)
            t = interleaved(calls, a)
            rec = {"long_ms": round(statistics.median(t["long"]), 4), "long_all_ms": t["long"]}
            if lane:
                rec.update({"lane_ms": round(statistics.median(t["lane"]), 4), "lane_all_ms": t["lane"]})
                rec["speedup"] = round(rec["lane_ms"] / rec["long_ms"], 2)
            out[op] = rec
        return out

    def close(self):
        self.c.close()
        torch.cuda.empty_cache()


def threshold(points: list) -> int:
    """The smallest size from which "long" beats "lane" at every larger measured size, over every algorithm and
    both operations (a size where the one-lane call was skipped for taking over a second counts as beaten)."""
    best = SIZES[-1]
    for size in reversed(SIZES):
        here = [p for p in points if p["bytes"] == size]
        if not all(p["lane_skipped"] or (p["seal"]["long_ms"] < p["seal"]["lane_ms"] and
                                         p["open"]["long_ms"] < p["open"]["lane_ms"]) for p in here):
            break
        best = size
    return best


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--algs", default=",".join(BY_NAME))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "aead_long" / "bench.jsonl"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if a.repeats < 7:
        sys.exit("a point is the median of at least 7 timed calls")
    if not torch.cuda.is_available():
        sys.exit("tools/aead_long_bench.py needs a GPU: there is nothing to time without one")
    common = {"repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "command": "python tools/aead_long_bench.py --repeats %d --warmup %d --rows %d --algs %s"
                         % (a.repeats, a.warmup, a.rows, a.algs), "commit": a.commit or commit_id()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    fh = open(a.out, "w")

    def emit(record: dict) -> None:
        record.update(common)
        line = json.dumps(record)
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    rng = np.random.default_rng(8439)
    algs, points = a.algs.split(","), []
    for alg in algs:
        lane = True
        for size in SIZES:
            case = Case(alg, 1, size, rng)
            if lane:  # one untimed probe call: past a second, this size and every larger one is skipped
                case.sealed = case.seal(True)
                torch.cuda.synchronize()
                probe = max(once(lambda: case.seal(False)), once(lambda: case.open(False)))
                lane = probe <= LANE_LIMIT_MS
            rec = {"bench": "aead_long", "alg": alg, "rows": 1, "bytes": size, "aad_bytes": len(AAD),
                   "lane_skipped": not lane}
            if not lane:
                rec["lane_skipped_why"] = "one call of the one-lane path takes more than %d ms at or below this size" \
                                          % LANE_LIMIT_MS
            rec.update(case.measure(a, lane))
            if size == SIZES[-1]:
                rec["long_seal_gbps"] = round(size / (rec["seal"]["long_ms"] * 1e-3) / 1e9, 2)
                rec["long_open_gbps"] = round(size / (rec["open"]["long_ms"] * 1e-3) / 1e9, 2)
                rec["device_copy_gbps"] = copy_gbps(size, a)
            emit(rec)
            points.append(rec)
            case.close()
    thr = threshold(points)
    emit({"bench": "aead_long_threshold", "algs": algs, "long_min_bytes": thr,
          "rule": "smallest measured size from which long < lane at every larger measured size, Seal and Open, all algs"})
    for alg in algs:
        case = Case(alg, a.rows, thr, rng)
        rec = {"bench": "aead_long_rows", "alg": alg, "rows": a.rows, "bytes": thr, "aad_bytes": len(AAD)}
        rec.update(case.measure(a, True))
        rec["long_wins"] = bool(rec["seal"]["long_ms"] < rec["seal"]["lane_ms"] and
                                rec["open"]["long_ms"] < rec["open"]["lane_ms"])
        emit(rec)
        case.close()
    fh.close()


if __name__ == "__main__":
    main()
