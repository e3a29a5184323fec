"""Ordered segmented Sampler.distinct (rsv_distinct_segmented_ordered) against the set launch and against
one ordered handle per stream.  Medians over --steps launches after --warmup, device events around each.

    --case a   C3's shape (2^20 streams x 4096 int64 keys, k = 64, ~30 % repeats), identity hash: nothing
               is tied, so ordered_ms - set_ms is the tie bookkeeping of kernel 1 plus the
               second kernel's pass over an all-zero tied[].  The two launches alternate in one loop and
               their results are compared bit for bit.
    --case b   the same shape, random Longs under the default hash (Long.hashCode, 32 bits): the number
               of tied streams and the time, again beside the set launch.
    --case c   every full stream tied: per element lo in [0, k + 3), hi in [0, --per-hash), key = hi << 32 |
               lo ^ hi (--per-hash keys per hashCode, k + 3 hashCodes).  Streams this long see every key, so
               the k-th entry closes a bucket when --per-hash divides k; the default 3 leaves k = 64 and
               k = 4096 one entry into a bucket of three.  Beside it one Sampler.distinct(k,
               order="ordered") handle per stream over the first --handles streams (create, sample_all,
               result; host clock), each checked against the launch as a set.

    python tools/bench_segmented_distinct_ordered.py --case a|b|c [--streams S] [--len N] [--k K]
                                                     [--per-hash 3] [--steps 10] [--warmup 3] [--handles 256]
                                                     [--out FILE]
prints one JSON line (and appends it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_segmented_distinct import make_keys  # noqa: E402


def make_tied_keys(torch, dev, S, n, k, per_hash):
    g = torch.Generator(device=dev)
    g.manual_seed(0x71ED)
    keys = torch.empty((S, n), dtype=torch.int64, device=dev)
    rows = max(1, (1 << 27) // n)
    for r0 in range(0, S, rows):
        r1 = min(S, r0 + rows)
        lo = torch.randint(0, k + 3, (r1 - r0, n), dtype=torch.int64, device=dev, generator=g)
        hi = torch.randint(0, per_hash, (r1 - r0, n), dtype=torch.int64, device=dev, generator=g)
        keys[r0:r1] = (hi << 32) | (lo ^ hi)
        del lo, hi
    return keys


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c"], required=True)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--per-hash", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--handles", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from reservoir_amd import Sampler, batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_distinct_ordered needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S = a.streams if a.streams is not None else (1 << 16 if a.case == "c" else 1 << 20)
    n, k = a.len, a.k
    total = S * n
    hash_name = "identity" if a.case == "a" else "default"
    keys = make_tied_keys(torch, dev, S, n, k, a.per_hash) if a.case == "c" else make_keys(torch, dev, S, n, a.dup)
    flat = keys.view(-1)
    offs = torch.arange(0, total + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def run_set():
        return batch.distinct_segmented(flat, offs, k, seed=11, hash=hash_name)

    def run_ordered():
        return batch.distinct_segmented_ordered(flat, offs, k, seed=11, hash=hash_name)

    first = run_ordered()
    ref = run_set()
    tied = first[3]
    n_tied = int(tied.sum().item())
    full = int((first[2] == k).sum().item())
    same_rows = (first[0] == ref[0]).all(dim=1)
    # a stream that is not tied is the set launch's row; a tied one may or may not differ from it
    if not bool(same_rows[tied == 0].all().item()) or not torch.equal(first[2], ref[2]):
        raise SystemExit("an untied stream differs from the set launch")
    differing = int((~same_rows).sum().item())
    del ref, same_rows
    t_set, t_ord = [], []
    for step in range(a.warmup + a.steps):
        ms_s, out = timed(run_set)
        del out
        ms_o, out = timed(run_ordered)
        del out
        if step >= a.warmup:
            t_set.append(ms_s)
            t_ord.append(ms_o)
    set_ms, ord_ms = statistics.median(t_set), statistics.median(t_ord)

    out = {"bench": "segmented_distinct_ordered", "case": a.case, "streams": S, "len": n, "k": k, "hash": hash_name,
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "per_hash": a.per_hash if a.case == "c" else None, "full_streams": full, "tied_streams": n_tied, "rows_differing_from_set": differing,
           "set_ms": set_ms, "set_ms_min": min(t_set), "set_ms_max": max(t_set),
           "ordered_ms": ord_ms, "ordered_ms_min": min(t_ord), "ordered_ms_max": max(t_ord),
           "ordered_minus_set_ms": ord_ms - set_ms, "ordered_over_set": ord_ms / set_ms,
           "ordered_us_per_stream": ord_ms * 1e3 / S, "ordered_GBps": total * 8 / 1e9 / (ord_ms / 1e3)}

    if a.case == "c":
        H = min(a.handles, S)
        fk, fc = first[0][:H].cpu().numpy(), first[2][:H].cpu().numpy()
        per = []
        for s in range(H):
            seg = keys[s]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = Sampler.distinct(k, seed=11 + s, order="ordered")(hash="java_long")
            h.sample_all(seg)
            got = h.result()
            per.append((time.perf_counter() - t0) * 1e6)
            if not np.array_equal(np.sort(got), np.sort(fk[s, :fc[s]])):
                raise SystemExit(f"stream {s}: the launch and the single ordered handle disagree")
        warm = per[min(8, H - 1):]  # the first handles pay one-time set-up
        out.update({"handles": H, "handles_us_per_stream": statistics.median(warm), "handles_us_per_stream_min": min(warm),
                    "handles_over_ordered": statistics.median(warm) / (ord_ms * 1e3 / S), "checked_streams": H})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
