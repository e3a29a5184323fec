"""Segmented Sampler.distinct (rsv_distinct_segmented): S independent distinct samplers in one launch.

Default shape = C3's (2^20 streams x 4096 int64 keys, k = 64), ~30 % duplicates inside each stream,
identity hash.  Reports, as medians over --steps launches after --warmup:

    ms               one rsv_distinct_segmented launch (device events around it)
    GBps             8 B x elements over that time
    us_per_stream    ms / streams
    k3_*             the single-stream K3 filter over the same flat array in the same run: one
                     Sampler.distinct(65536, hash="identity") fed the array in pieces of <= 2^29 keys,
                     kernel time summed by rsv_profile_read; ratio_to_k3 = GBps / k3_GBps
    handles_*        the only alternative without this entry point: one Sampler.distinct handle per
                     stream (create, sample_all of the segment, result), over the first 256 streams,
                     host clock, as time per stream

The result of the first launch is checked against the single handles of the first 256 streams.

    python tools/bench_segmented_distinct.py [--streams 1048576] [--len 4096] [--k 64] [--dup 0.3]
                                             [--steps 10] [--warmup 3] [--out FILE]
prints one JSON line (and appends it to --out).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_keys(torch, dev, S, n, dup):
    """(S, n) random int64 keys; ~dup of each stream's positions repeat another position of that stream."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    keys = torch.empty((S, n), dtype=torch.int64, device=dev)
    rows = max(1, (1 << 27) // n)
    for r0 in range(0, S, rows):
        r1 = min(S, r0 + rows)
        v = torch.randint(-2**63, 2**63 - 1, (r1 - r0, n), dtype=torch.int64, device=dev, generator=g)
        src = torch.randint(0, n, (r1 - r0, n), dtype=torch.int64, device=dev, generator=g)
        rep = torch.rand((r1 - r0, n), device=dev, generator=g) < dup
        keys[r0:r1] = torch.where(rep, torch.gather(v, 1, src), v)
        del v, src, rep
    return keys


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--handles", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from reservoir_amd import Sampler, batch
    from reservoir_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_distinct needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = N.load()
    S, n, k = a.streams, a.len, a.k
    total = S * n

    keys = make_keys(torch, dev, S, n, a.dup)
    flat = keys.view(-1)
    offs = torch.arange(0, total + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def launch():
        return batch.distinct_segmented(flat, offs, k, seed=11, hash="identity")

    first = launch()
    times = []
    for step in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch()
        e1.record()
        e1.synchronize()
        if step >= a.warmup:
            times.append(e0.elapsed_time(e1))
        del out
    ms = statistics.median(times)
    gbytes = total * 8 / 1e9

    # K3 over the same bytes
    d = Sampler.distinct(65536, seed=11)(hash="identity")
    N.check(L.rsv_profile_enable(d.handle, 1))
    piece = 1 << 29
    for p in range(0, total, piece):
        d.sample_all(flat[p:p + piece])
    k3_ms, k3_launches = C.c_double(), C.c_int64()
    N.check(L.rsv_profile_read(d.handle, C.byref(k3_ms), C.byref(k3_launches)))
    d.close()

    # one handle per stream, the first `handles` streams; checked against the launch
    H = min(a.handles, S)
    fk, fc = first[0][:H].cpu().numpy(), first[2][:H].cpu().numpy()
    per = []
    for s in range(H):
        seg = keys[s]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = Sampler.distinct(k, seed=11 + s, order="set")(hash="identity")
        h.sample_all(seg)
        got = h.result()
        per.append((time.perf_counter() - t0) * 1e6)
        if not np.array_equal(got, fk[s, :fc[s]]):
            raise SystemExit(f"stream {s}: the launch and the single handle disagree")
    warm = per[min(8, H - 1):]  # the first handles pay one-time set-up

    out = {"bench": "segmented_distinct", "streams": S, "len": n, "k": k, "dup": a.dup, "hash": "identity",
           "form": "wave" if k <= 256 else "workgroup", "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "ms": ms, "ms_min": min(times), "ms_max": max(times), "GBps": gbytes / (ms / 1e3),
           "us_per_stream": ms * 1e3 / S,
           "k3_ms": k3_ms.value, "k3_launches": k3_launches.value, "k3_GBps": gbytes / (k3_ms.value / 1e3),
           "ratio_to_k3": (k3_ms.value / ms),
           "handles": H, "handles_us_per_stream": statistics.median(warm), "handles_us_per_stream_min": min(warm),
           "handles_over_segmented": statistics.median(warm) / (ms * 1e3 / S), "checked_streams": H}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
