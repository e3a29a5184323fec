"""Resumed ordered segmented Sampler.distinct (batch.SegmentedDistinctOrdered: rsv_distinct_segmented_ordered_update).

The streams are cut into B equal batches and fed as B update launches into one heap-array state, for every B of
--batches, in one run, beside the stateless ordered launch over the same keys and (--case c3) beside
batch.SegmentedDistinct.update over the same cuts.  Device events around every launch, --warmup runs then --steps
timed runs per B (the counts are zeroed before each run, outside the timed windows).

    --case c3     C3's shape: 2^20 streams x 4096 int64 keys, ~30 % repeats, k = 64, default hash (Long.hashCode;
                  tools/bench_segmented_distinct.py make_keys).  Nothing is tied, so the set state ends in the same sets.
    --case tied   every stream tied: 2^16 streams x 4096, --per-hash keys per hashCode, k + 3 hashCodes
                  (tools/bench_segmented_distinct_ordered.py make_tied_keys, its case c).

Per B it reports
    launch_ms[B]     median time of each of the B launches
    sum_ms           median over the runs of the sum of the B launch times (sum_ms_min / _max: the spread)
    steady_ms        B >= 3: the same over launches 3..B alone -- the heap is full from their first element on --
                     and steady_ms_per_launch
    set_launch_ms / set_sum_ms (c3)   the same for SegmentedDistinct.update
    over_stateless   sum_ms / stateless_ms, stateless_ms the median of one rsv_distinct_segmented_ordered launch
    check            result() equals the stateless ordered launch (keys, hashes, counts), bit for bit

    python tools/bench_segmented_distinct_ordered_state.py --case c3|tied [--streams S] [--len N] [--k K]
                                                           [--batches 1,2,8] [--per-hash 3] [--steps 10] [--warmup 3]
                                                           [--out FILE]
prints one JSON line (and appends it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_segmented_distinct import make_keys  # noqa: E402
from bench_segmented_distinct_ordered import make_tied_keys  # noqa: E402
from bench_segmented_distinct_state import pieces, timed  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["c3", "tied"], required=True)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--batches", default=None)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--per-hash", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from reservoir_amd import batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_distinct_ordered_state needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    c3 = a.case == "c3"
    S = a.streams if a.streams is not None else (1 << 20 if c3 else 1 << 16)
    n, k = a.len, a.k
    Bs = [int(x) for x in (a.batches or ("1,2,8" if c3 else "1,8")).split(",")]
    if any(n % B for B in Bs):
        raise SystemExit("--len must be a multiple of every number of batches")
    keys = make_keys(torch, dev, S, n, a.dup) if c3 else make_tied_keys(torch, dev, S, n, k, a.per_hash)
    flat = keys.view(-1)
    offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    sl = []
    for step in range(a.warmup + a.steps):
        ms, ref = timed(torch, lambda: batch.distinct_segmented_ordered(flat, offs, k, seed=11, hash="default"))
        if step >= a.warmup:
            sl.append(ms)
        if step < a.warmup + a.steps - 1:
            del ref
    sl_ms = statistics.median(sl)
    tied = int(ref[3].sum().item())

    out = {"bench": "segmented_distinct_ordered_state", "case": a.case, "streams": S, "len": n, "k": k, "hash": "default",
           "dup": a.dup if c3 else None, "per_hash": None if c3 else a.per_hash, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "tied_streams": tied, "stateless_ms": sl_ms,
           "stateless_ms_min": min(sl), "stateless_ms_max": max(sl), "stateless_us_per_stream": sl_ms * 1e3 / S,
           "batches": {}}
    ok = True
    so = batch.SegmentedDistinctOrdered(S, k, seed=11, hash="default", device=dev)
    sd = batch.SegmentedDistinct(S, k, seed=11, hash="default", device=dev) if c3 else None

    def summary(runs, B, prefix=""):
        sums = [sum(r) for r in runs]
        d = {prefix + "launch_ms": [statistics.median(r[t] for r in runs) for t in range(B)],
             prefix + "sum_ms": statistics.median(sums), prefix + "sum_ms_min": min(sums), prefix + "sum_ms_max": max(sums)}
        if B >= 3:
            steady = [sum(r[2:]) for r in runs]
            d[prefix + "steady_ms"] = statistics.median(steady)
            d[prefix + "steady_ms_per_launch"] = statistics.median(steady) / (B - 2)
        return d

    for B in Bs:
        parts, poffs = ([flat], offs) if B == 1 else pieces(torch, keys, B)
        torch.cuda.synchronize()
        res = {}
        for state, prefix in ((so, ""), (sd, "set_")):
            if state is None:
                continue
            runs = []
            for step in range(a.warmup + a.steps):
                state.counts.zero_()
                per = [timed(torch, lambda t=t: state.update(parts[t], poffs))[0] for t in range(B)]
                if step >= a.warmup:
                    runs.append(per)
            res.update(summary(runs, B, prefix))
        got = so.result()
        res["check"] = bool(all(torch.equal(x, y) for x, y in zip(got, ref[:3])))
        if sd is not None and tied == 0:  # nothing tied: the set state holds the same sets
            res["set_check"] = bool(torch.equal(sd.keys, ref[0]) and torch.equal(sd.counts, ref[2]))
        res["over_stateless"] = res["sum_ms"] / sl_ms
        res["us_per_stream"] = res["sum_ms"] * 1e3 / S
        if "set_sum_ms" in res:
            res["over_set_state"] = res["sum_ms"] / res["set_sum_ms"]
        ok = ok and res["check"] and res.get("set_check", True)
        out["batches"][str(B)] = res
        del parts, got
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the state and the stateless ordered launch disagree")


if __name__ == "__main__":
    main()
