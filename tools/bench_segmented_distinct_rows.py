"""Segmented Sampler.distinct over byte keys (rsv_distinct_segmented_rows): S independent distinct
samplers over 16-byte rows (java.util.UUID) in one launch.

Default shape = K5's first (2^20 streams x 4096 rows, k = 64), ~30 % repeats inside each stream.  Per
hash kind of --hash (precomputed 64-bit hashes, and/or UUID.hashCode computed in the kernel) it
reports, as medians over --steps launches after --warmup:

    ms               one rsv_distinct_segmented_rows launch (device events around it)
    GBps             the bytes the element loop has to read (8 B x elements for precomputed hashes,
                     16 B x elements for UUID.hashCode) over that time
    us_per_stream    ms / streams
    int64_*          (a) batch.distinct_segmented over the same number of int64 keys with the same
                     repeats (the rows' 64-bit hashes as keys, identity hash), in the same run;
                     ratio_to_int64 = ms / int64_ms: what the index entries and the tie reads cost
    handles_*        (b) the only alternative without this entry point: one
                     Sampler.distinct(k, key_type="bytes16", order="set") handle per stream (create,
                     sample_all of the segment, result), over the first 256 streams, host clock, as
                     time per stream; handles_over_segmented has to be above 1

The result of the first launch is checked against the single handles of the first 256 streams.

    python tools/bench_segmented_distinct_rows.py [--streams 1048576] [--len 4096] [--k 64] [--dup 0.3]
                                                  [--hash precomputed,uuid] [--steps 10] [--warmup 3]
                                                  [--out profiles/segmented_distinct_rows/bench.json]
prints one JSON line per hash kind (and appends it to --out).
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

G = 0x9E3779B97F4A7C15 - 2**64  # as a signed 64-bit multiplier (int64 products wrap)


def make_rows(torch, dev, S, n, dup):
    """(rows int64 [S * n, 2], hashes int64 [S * n]): word 0 random, ~dup of each stream's positions
    repeating another position of that stream; word 1 and the hash are functions of word 0, so equal
    rows carry equal hashes and the hash is injective on the rows."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    rows = torch.empty((S, n, 2), dtype=torch.int64, device=dev)
    hashes = torch.empty((S, n), dtype=torch.int64, device=dev)
    step = max(1, (1 << 27) // n)
    for a in range(0, S, step):
        b = min(S, a + step)
        v = torch.randint(-2**63, 2**63 - 1, (b - a, n), dtype=torch.int64, device=dev, generator=g)
        src = torch.randint(0, n, (b - a, n), dtype=torch.int64, device=dev, generator=g)
        rep = torch.rand((b - a, n), device=dev, generator=g) < dup
        w0 = torch.where(rep, torch.gather(v, 1, src), v)
        del v, src, rep
        rows[a:b, :, 0] = w0
        rows[a:b, :, 1] = (w0 ^ 0x5A5A5A5A5A5A5A5A) * G
        hashes[a:b] = (w0 * G) ^ (w0 >> 29)
        del w0
    return rows.view(S * n, 2), hashes.view(-1)


def timed(torch, launch, warmup, steps):
    times = []
    for step in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch()
        e1.record()
        e1.synchronize()
        if step >= warmup:
            times.append(e0.elapsed_time(e1))
        del out
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--hash", default="precomputed,uuid")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--handles", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmented_distinct_rows", "bench.json"))
    a = ap.parse_args()
    kinds = a.hash.split(",")
    if not kinds or any(h not in ("precomputed", "uuid") for h in kinds):
        raise SystemExit("--hash takes precomputed, uuid or both")

    import numpy as np
    import torch

    from reservoir_amd import Sampler, batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_distinct_rows needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S, n, k = a.streams, a.len, a.k
    total = S * n

    words, hashes = make_rows(torch, dev, S, n, a.dup)
    rows = words.view(torch.uint8)  # (total, 16): the documented form over the same memory
    offs = torch.arange(0, total + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    # (a) the Long-key launch over as many keys with the same repeats
    i_times = timed(torch, lambda: batch.distinct_segmented(hashes, offs, k, seed=11, hash="identity"), a.warmup, a.steps)
    int64_ms = statistics.median(i_times)

    H = min(a.handles, S)
    for kind in kinds:
        hs = hashes if kind == "precomputed" else None

        def launch():
            return batch.distinct_segmented_rows(rows, offs, k, seed=11, hashes=hs)

        first = launch()
        times = timed(torch, launch, a.warmup, a.steps)
        ms = statistics.median(times)
        gbytes = total * (8 if kind == "precomputed" else 16) / 1e9

        # (b) one handle per stream, the first H streams; checked against the launch
        fr, fc = first[0][:H].cpu().numpy(), first[2][:H].cpu().numpy()
        del first
        per = []
        for s in range(H):
            seg = rows[s * n:(s + 1) * n]
            seg_h = hashes[s * n:(s + 1) * n] if hs is not None else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if hs is not None:
                h = Sampler.distinct(k, key_type="bytes16", seed=11 + s, order="set")(hash=lambda b: 0)
                h.sample_all(seg, hashes=seg_h)
            else:
                h = Sampler.distinct(k, key_type="bytes16", seed=11 + s, order="set")()
                h.sample_all(seg)
            got = h.result()
            per.append((time.perf_counter() - t0) * 1e6)
            held = sorted(bytes(r) for r in np.asarray(got).reshape(-1, 16))
            if held != sorted(bytes(r) for r in fr[s, :fc[s]]):
                raise SystemExit(f"stream {s}: the launch and the single handle disagree")
        warm = per[min(8, H - 1):]  # the first handles pay one-time set-up
        handles_us = statistics.median(warm)
        if handles_us <= ms * 1e3 / S:
            raise SystemExit("one handle per stream was not slower than the segmented launch")

        out = {"bench": "segmented_distinct_rows", "streams": S, "len": n, "k": k, "key_width": 16, "dup": a.dup,
               "hash": kind, "form": "wave" if k <= 256 else "workgroup", "steps": a.steps, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0),
               "ms": ms, "ms_min": min(times), "ms_max": max(times), "GBps": gbytes / (ms / 1e3),
               "us_per_stream": ms * 1e3 / S,
               "int64_ms": int64_ms, "int64_ms_min": min(i_times), "int64_ms_max": max(i_times),
               "ratio_to_int64": ms / int64_ms,
               "handles": H, "handles_us_per_stream": handles_us, "handles_us_per_stream_min": min(warm),
               "handles_over_segmented": handles_us / (ms * 1e3 / S), "checked_streams": H}
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
