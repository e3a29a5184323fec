"""Resumed segmented Sampler.distinct over byte keys (batch.SegmentedDistinctRows:
rsv_distinct_segmented_rows_update / _merge).

--mode update (default): the streams of tools/bench_segmented_distinct_rows.py (its make_rows:
S streams x len 16-byte rows, ~dup repeats inside each stream, precomputed 64-bit hashes) cut into B
equal batches and fed as B update launches into one state, for every B of --batches, against one
stateless rsv_distinct_segmented_rows launch over the same rows in the same run.  Device events around
every launch, --warmup runs then --steps timed runs of the B launches (the counts are zeroed before
each run, outside the timed windows).  Reports, one JSON line per B,

    launch_ms[B]      median time of each of the B launches
    sum_ms            median over the runs of the sum of the B launch times (sum_ms_min / _max: the spread)
    stateless_ms      median of one stateless launch (stateless_ms_min / _max)
    ratio             sum_ms / stateless_ms
    state_bytes       B x S x 2 x (W + 8) x k: every launch reading and writing every row, an upper bound
                      (an update reads a row's hashes, its rows only on ties, and writes what moves)
    later_over_first  mean of launches 2..B over launch 1: what a known threshold saves
    check             the state equals the stateless result (rows, hashes, counts)

--mode merge: P parts (the stateless results of P index-split pieces of every stream) merged in one
launch into an empty state (merge_ms) and once more into the merged state (remerge_ms: every entry
ties with a member, row compares throughout), against a device copy of the same part bytes in the same
run (copy_ms); merge_over_copy = merge_ms / copy_ms.  check: the merged state equals the stateless
result over the whole streams.

    python tools/bench_segmented_distinct_rows_state.py [--mode update] [--streams 1048576] [--len 4096] [--k 64]
                                                        [--batches 1,2,8] [--dup 0.3] [--steps 10] [--warmup 3]
    python tools/bench_segmented_distinct_rows_state.py --mode merge [--parts 8] [--streams 1048576] [--len 2048]
    [--out profiles/segmented_distinct_rows_state/bench.json]
prints one JSON line per result (and appends it to --out).
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

from bench_segmented_distinct_rows import make_rows  # noqa: E402

W = 16


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def pieces(torch, words, hashes, S, n, B):
    """B contiguous column slices of the (S, n) streams: [(rows int64 [S * n / B, 2], hashes)], their offsets."""
    w = n // B
    offs = torch.arange(0, S * w + 1, w, dtype=torch.int64, device=words.device)
    if B == 1:
        return [(words, hashes)], offs
    wv, hv = words.view(S, n, 2), hashes.view(S, n)
    return [(wv[:, t * w:(t + 1) * w].contiguous().view(-1, 2), hv[:, t * w:(t + 1) * w].contiguous().view(-1))
            for t in range(B)], offs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["update", "merge"], default="update")
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=None)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmented_distinct_rows_state", "bench.json"))
    a = ap.parse_args()

    import torch

    from reservoir_amd import batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_distinct_rows_state needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S, k = a.streams, a.k
    n = a.len if a.len is not None else (4096 if a.mode == "update" else 2048)
    Bs = [int(b) for b in a.batches.split(",")] if a.mode == "update" else [a.parts]
    if any(b <= 0 or n % b for b in Bs):
        raise SystemExit("--len must be a multiple of every number of pieces")
    words, hashes = make_rows(torch, dev, S, n, a.dup)
    offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def stateless():
        return batch.distinct_segmented_rows(words, offs, k, seed=11, hashes=hashes)

    def same(sd, ref):
        return bool(torch.equal(sd.rows, ref[0]) and torch.equal(sd.hashes, ref[1]) and torch.equal(sd.counts, ref[2]))

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if not out["check"]:
            raise SystemExit("the state and the stateless launch disagree")

    base = {"bench": "segmented_distinct_rows_state", "mode": a.mode, "streams": S, "len": n, "k": k, "key_width": W,
            "dup": a.dup, "hash": "precomputed", "form": "wave" if k <= 256 else "workgroup", "steps": a.steps,
            "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    sd = batch.SegmentedDistinctRows(S, k, W, seed=11, hash="precomputed", device=dev)

    if a.mode == "update":
        sl = []
        for step in range(a.warmup + a.steps):
            ms, ref = timed(torch, stateless)
            if step >= a.warmup:
                sl.append(ms)
            if step < a.warmup + a.steps - 1:
                del ref
        sl_ms = statistics.median(sl)
        for B in Bs:
            parts, poffs = pieces(torch, words, hashes, S, n, B)
            runs = []
            for step in range(a.warmup + a.steps):
                sd.counts.zero_()
                per = [timed(torch, lambda t=t: sd.update(parts[t][0], poffs, hashes=parts[t][1]))[0] for t in range(B)]
                if step >= a.warmup:
                    runs.append(per)
            del parts
            sums = [sum(r) for r in runs]
            launch = [statistics.median(r[t] for r in runs) for t in range(B)]
            sum_ms = statistics.median(sums)
            emit(dict(base, batches=B, launch_ms=launch, sum_ms=sum_ms, sum_ms_min=min(sums), sum_ms_max=max(sums),
                      stateless_ms=sl_ms, stateless_ms_min=min(sl), stateless_ms_max=max(sl), ratio=sum_ms / sl_ms,
                      state_bytes=B * S * 2 * (W + 8) * k,
                      later_over_first=(statistics.mean(launch[1:]) / launch[0]) if B > 1 else None,
                      check=same(sd, ref)))
    else:
        B = Bs[0]
        ref = stateless()
        parts, poffs = pieces(torch, words, hashes, S, n, B)
        pr, ph, pc = [], [], []
        for t in range(B):
            r = batch.distinct_segmented_rows(parts[t][0], poffs, k, seed=11, hashes=parts[t][1])
            pr.append(r[0]), ph.append(r[1]), pc.append(r[2])
        pr, ph, pc = torch.stack(pr), torch.stack(ph), torch.stack(pc)
        cr, ch, cc = torch.empty_like(pr), torch.empty_like(ph), torch.empty_like(pc)
        del parts, words, hashes
        torch.cuda.synchronize()

        def copy():
            cr.copy_(pr)
            ch.copy_(ph)
            cc.copy_(pc)

        mg, rm, cp = [], [], []
        for step in range(a.warmup + a.steps):
            sd.counts.zero_()
            t0 = timed(torch, lambda: sd.merge(pr, ph, pc))[0]
            if step == 0 and not same(sd, ref):
                raise SystemExit("the merged state and the stateless launch disagree")
            t1 = timed(torch, lambda: sd.merge(pr, ph, pc))[0]
            t2 = timed(torch, copy)[0]
            if step >= a.warmup:
                mg.append(t0), rm.append(t1), cp.append(t2)
        nbytes = pr.numel() + ph.numel() * 8 + pc.numel() * 8
        m, c = statistics.median(mg), statistics.median(cp)
        emit(dict(base, parts=B, part_bytes=nbytes, merge_ms=m, merge_ms_min=min(mg), merge_ms_max=max(mg),
                  remerge_ms=statistics.median(rm), copy_ms=c, copy_ms_min=min(cp), copy_ms_max=max(cp),
                  merge_GBps=nbytes / m / 1e6, copy_GBps=nbytes / c / 1e6, merge_over_copy=m / c, check=same(sd, ref)))


if __name__ == "__main__":
    main()
