"""Resumed ordered segmented Sampler.distinct over byte keys (batch.SegmentedDistinctRowsOrdered:
rsv_distinct_segmented_rows_ordered_update).  16-byte rows (java.util.UUID) under UUID.hashCode computed in the kernel.

The streams are cut into B equal batches and fed as B update launches into one state, for every B of --batches, in
one run, beside -- from the same session --
    the stateless batch.distinct_segmented_rows_ordered launch over the same rows,
    batch.SegmentedDistinctRows.update (the set order's state) over the same cuts,
    batch.SegmentedDistinctOrdered.update over Long keys with the same offsets and cuts (after the rows are freed).
Device events around every launch, --warmup runs then --steps timed runs per B (the counts are zeroed before each
run, outside the timed windows).

    --case c3     C3's shape: 2^20 streams x 4096 UUIDs, ~30 % repeats, k = 64 (tools/bench_segmented_distinct_rows_ordered.py
                  make_random_uuids; Long keys: tools/bench_segmented_distinct.py make_keys).  Few streams or none are tied.
    --case tied   every stream tied: 2^16 streams x 4096, --per-hash UUIDs per hashCode, k + 3 hashCodes
                  (make_tied_uuids; Long keys: tools/bench_segmented_distinct_ordered.py make_tied_keys).

Per B it reports
    launch_ms[B]     median time of each of the B launches
    sum_ms           median over the runs of the sum of the B launch times (sum_ms_min / _max: the spread)
    steady_ms        B >= 3: the same over launches 3..B alone -- the heap is full from their first element on --
                     and steady_ms_per_launch
    set_*            the same for SegmentedDistinctRows.update
    long_*           the same for SegmentedDistinctOrdered.update over Long keys
    over_stateless   sum_ms / stateless_ms, stateless_ms the median of one rsv_distinct_segmented_rows_ordered launch
    check            result() equals the stateless ordered launch (rows, hashes, counts), bit for bit

    python tools/bench_segmented_distinct_rows_ordered_state.py --case c3|tied [--streams S] [--len N] [--k K]
                                                                [--batches 1,2,8] [--per-hash 3] [--steps 10]
                                                                [--warmup 3] [--out FILE]
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
from bench_segmented_distinct_rows_ordered import make_random_uuids, make_tied_uuids  # noqa: E402
from bench_segmented_distinct_state import pieces as key_pieces  # noqa: E402
from bench_segmented_distinct_state import timed  # noqa: E402

W = 16


def row_pieces(torch, words, S, n, B):
    """B contiguous column slices of the (S, n) streams: [rows int64 [S * n / B, 2]], their offsets."""
    w = n // B
    offs = torch.arange(0, S * w + 1, w, dtype=torch.int64, device=words.device)
    if B == 1:
        return [words], offs
    wv = words.view(S, n, 2)
    return [wv[:, t * w:(t + 1) * w].contiguous().view(-1, 2) for t in range(B)], offs


def summary(runs, B, prefix=""):
    sums = [sum(r) for r in runs]
    d = {prefix + "launch_ms": [statistics.median(r[t] for r in runs) for t in range(B)],
         prefix + "sum_ms": statistics.median(sums), prefix + "sum_ms_min": min(sums), prefix + "sum_ms_max": max(sums)}
    if B >= 3:
        steady = [sum(r[2:]) for r in runs]
        d[prefix + "steady_ms"] = statistics.median(steady)
        d[prefix + "steady_ms_per_launch"] = statistics.median(steady) / (B - 2)
    return d


def feed(torch, state, parts, poffs, B, warmup, steps):
    runs = []
    for step in range(warmup + steps):
        state.counts.zero_()
        per = [timed(torch, lambda t=t: state.update(parts[t], poffs))[0] for t in range(B)]
        if step >= warmup:
            runs.append(per)
    return runs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["c3", "tied"], required=True)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--per-hash", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from reservoir_amd import batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_distinct_rows_ordered_state needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    c3 = a.case == "c3"
    S = a.streams if a.streams is not None else (1 << 20 if c3 else 1 << 16)
    n, k = a.len, a.k
    Bs = [int(x) for x in a.batches.split(",")]
    if any(B <= 0 or n % B for B in Bs):
        raise SystemExit("--len must be a multiple of every number of batches")
    words = make_random_uuids(torch, dev, S, n, a.dup) if c3 else make_tied_uuids(torch, dev, S, n, k, a.per_hash)
    offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    sl = []
    for step in range(a.warmup + a.steps):
        ms, ref = timed(torch, lambda: batch.distinct_segmented_rows_ordered(words, offs, k, seed=11))
        if step >= a.warmup:
            sl.append(ms)
        if step < a.warmup + a.steps - 1:
            del ref
    sl_ms = statistics.median(sl)
    tied = int(ref[3].sum().item())

    out = {"bench": "segmented_distinct_rows_ordered_state", "case": a.case, "streams": S, "len": n, "k": k, "key_width": W,
           "hash": "uuid", "dup": a.dup if c3 else None, "per_hash": None if c3 else a.per_hash, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "tied_streams": tied, "stateless_ms": sl_ms,
           "stateless_ms_min": min(sl), "stateless_ms_max": max(sl), "stateless_us_per_stream": sl_ms * 1e3 / S,
           "batches": {}}
    ok = True
    so = batch.SegmentedDistinctRowsOrdered(S, k, W, seed=11, device=dev)
    sd = batch.SegmentedDistinctRows(S, k, W, seed=11, device=dev)
    for B in Bs:
        parts, poffs = row_pieces(torch, words, S, n, B)
        torch.cuda.synchronize()
        res = summary(feed(torch, so, parts, poffs, B, a.warmup, a.steps), B)
        res.update(summary(feed(torch, sd, parts, poffs, B, a.warmup, a.steps), B, "set_"))
        got = so.result()
        res["check"] = bool(all(torch.equal(x, y) for x, y in zip(got, ref[:3])))
        if tied == 0:  # nothing tied: the set state holds the same sets
            res["set_check"] = bool(torch.equal(sd.rows, ref[0]) and torch.equal(sd.counts, ref[2]))
        res["over_stateless"] = res["sum_ms"] / sl_ms
        res["us_per_stream"] = res["sum_ms"] * 1e3 / S
        res["over_set_state"] = res["sum_ms"] / res["set_sum_ms"]
        ok = ok and res["check"] and res.get("set_check", True)
        out["batches"][str(B)] = res
        del parts, got
    del words, ref, so, sd
    torch.cuda.empty_cache()

    keys = make_keys(torch, dev, S, n, a.dup) if c3 else make_tied_keys(torch, dev, S, n, k, a.per_hash)
    sl_long = batch.SegmentedDistinctOrdered(S, k, seed=11, hash="default", device=dev)
    for B in Bs:
        parts, poffs = ([keys.view(-1)], offs) if B == 1 else key_pieces(torch, keys, B)
        torch.cuda.synchronize()
        res = out["batches"][str(B)]
        res.update(summary(feed(torch, sl_long, parts, poffs, B, a.warmup, a.steps), B, "long_"))
        res["over_long_state"] = res["sum_ms"] / res["long_sum_ms"]
        del parts
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
