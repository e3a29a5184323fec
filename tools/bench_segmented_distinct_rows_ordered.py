"""Ordered segmented Sampler.distinct over byte keys (rsv_distinct_segmented_rows_ordered) against the set-rows
launch and against one ordered handle per stream.  16-byte rows (java.util.UUID) under UUID.hashCode computed
in the kernels.  Medians over --steps launches after --warmup, device events around each; the set-rows launch
and the ordered-rows launch alternate in one loop.

    --case a   C3's shape (2^20 streams x 4096 UUIDs, k = 64, ~30 % repeats), random UUIDs: UUID.hashCode
               folds 128 random bits to 32, so few streams or none are tied and ordered_ms - set_ms is the tie
               bookkeeping of kernel 1 plus the second kernel's pass over tied[].
    --case b   2^16 x 4096, k = 64, every full stream tied: per element c in [0, k + 3), v in [0, --per-hash),
               msb = mix(v, c), lsb = msb ^ (v << 32 | c ^ v), so UUID.hashCode = c and a hashCode holds
               --per-hash UUIDs.  Streams this long see every UUID, so the k-th entry closes a bucket when
               --per-hash divides k; the default 3 leaves k = 64 and k = 4096 one entry into a bucket of three.
    --case c   256 x 2^17, k = 4096, the same generator.
For b and c, beside the launch: one Sampler.distinct(k, key_type="bytes16", order="ordered") handle per stream
over the first --handles streams (create, sample_all, result; host clock).  The launch's rows and hashes of those
streams must equal oracle.DistinctRows on the host; handles whose set differs from the oracle's are listed.

    python tools/bench_segmented_distinct_rows_ordered.py --case a|b|c [--streams S] [--len N] [--k K]
                                                          [--per-hash 3] [--steps 10] [--warmup 3]
                                                          [--handles 256] [--out FILE]
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

G = 0x9E3779B97F4A7C15 - 2**64  # as a signed 64-bit multiplier (int64 products wrap)
SHAPES = {"a": (1 << 20, 4096, 64), "b": (1 << 16, 4096, 64), "c": (256, 1 << 17, 4096)}


def make_random_uuids(torch, dev, S, n, dup):
    """int64 [S * n, 2]: msb random with ~dup of each stream's positions repeating another position of
    that stream, lsb a mix of msb (equal msb = equal UUID)."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    rows = torch.empty((S, n, 2), dtype=torch.int64, device=dev)
    step = max(1, (1 << 27) // n)
    for a in range(0, S, step):
        b = min(S, a + step)
        v = torch.randint(-2**63, 2**63 - 1, (b - a, n), dtype=torch.int64, device=dev, generator=g)
        src = torch.randint(0, n, (b - a, n), dtype=torch.int64, device=dev, generator=g)
        rep = torch.rand((b - a, n), device=dev, generator=g) < dup
        w0 = torch.where(rep, torch.gather(v, 1, src), v)
        del v, src, rep
        rows[a:b, :, 0] = w0
        rows[a:b, :, 1] = ((w0 ^ 0x5A5A5A5A5A5A5A5A) * G) ^ (w0 >> 31)
        del w0
    return rows.view(S * n, 2)


def make_tied_uuids(torch, dev, S, n, k, per_hash):
    """int64 [S * n, 2]: per_hash UUIDs per hashCode over k + 3 hashCodes (the docstring's case b)."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x71ED)
    rows = torch.empty((S, n, 2), dtype=torch.int64, device=dev)
    step = max(1, (1 << 27) // n)
    for a in range(0, S, step):
        b = min(S, a + step)
        c = torch.randint(0, k + 3, (b - a, n), dtype=torch.int64, device=dev, generator=g)
        v = torch.randint(0, per_hash, (b - a, n), dtype=torch.int64, device=dev, generator=g)
        low = (v << 32) | (c ^ v)
        msb = (low + 1) * G
        msb = (msb ^ (msb >> 29)) * G
        rows[a:b, :, 0] = msb
        rows[a:b, :, 1] = msb ^ low
        del c, v, low, msb
    return rows.view(S * n, 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c"], required=True)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--len", type=int, default=None)
    ap.add_argument("--k", type=int, default=None)
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
        raise SystemExit("bench_segmented_distinct_rows_ordered needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S0, n0, k0 = SHAPES[a.case]
    S = a.streams if a.streams is not None else S0
    n = a.len if a.len is not None else n0
    k = a.k if a.k is not None else k0
    total = S * n
    words = make_random_uuids(torch, dev, S, n, a.dup) if a.case == "a" else make_tied_uuids(torch, dev, S, n, k, a.per_hash)
    rows = words.view(torch.uint8)  # (total, 16): the documented form over the same memory
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
        return batch.distinct_segmented_rows(rows, offs, k, seed=11)

    def run_ordered():
        return batch.distinct_segmented_rows_ordered(rows, offs, k, seed=11)

    first = run_ordered()
    ref = run_set()
    tied = first[3]
    n_tied = int(tied.sum().item())
    full = int((first[2] == k).sum().item())
    same_rows = (first[0] == ref[0]).all(dim=2).all(dim=1)
    # a stream that is not tied is the set launch's row block; a tied one may or may not differ from it
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

    out = {"bench": "segmented_distinct_rows_ordered", "case": a.case, "streams": S, "len": n, "k": k, "key_width": 16,
           "hash": "uuid", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "per_hash": a.per_hash if a.case != "a" else None, "full_streams": full, "tied_streams": n_tied,
           "rows_differing_from_set": differing,
           "set_ms": set_ms, "set_ms_min": min(t_set), "set_ms_max": max(t_set),
           "ordered_ms": ord_ms, "ordered_ms_min": min(t_ord), "ordered_ms_max": max(t_ord),
           "ordered_minus_set_ms": ord_ms - set_ms, "ordered_over_set": ord_ms / set_ms,
           "ordered_us_per_stream": ord_ms * 1e3 / S, "ordered_GBps": total * 16 / 1e9 / (ord_ms / 1e3)}

    if a.case != "a":
        # the first H streams: the launch against oracle.DistinctRows on the host (it has to agree), and one
        # ordered handle per stream, timed; a handle that disagrees with the oracle is counted, not hidden
        from oracle import oracle as O

        H = min(a.handles, S)
        fr, fh, fc = (t[:H].cpu().numpy() for t in first[:3])
        host = rows[:H * n].cpu().numpy()
        per, off = [], []
        for s in range(H):
            ref = O.DistinctRows(k, 11 + s, 16, "uuid")
            ref.sample_all(host[s * n:(s + 1) * n])
            rr, rh = ref.result()
            m = rr.shape[0]
            if fc[s] != m or not np.array_equal(fr[s, :m], rr) or not np.array_equal(fh[s, :m], rh):
                raise SystemExit(f"stream {s}: the launch and the oracle disagree")
            seg = rows[s * n:(s + 1) * n]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = Sampler.distinct(k, key_type="bytes16", seed=11 + s, order="ordered")()
            h.sample_all(seg)
            got = h.result()
            per.append((time.perf_counter() - t0) * 1e6)
            if sorted(bytes(r) for r in np.asarray(got).reshape(-1, 16)) != sorted(bytes(r) for r in rr):
                off.append(s)
        warm = per[min(8, H - 1):]  # the first handles pay one-time set-up
        out.update({"handles": H, "handles_us_per_stream": statistics.median(warm), "handles_us_per_stream_min": min(warm),
                    "handles_over_ordered": statistics.median(warm) / (ord_ms * 1e3 / S), "checked_streams": H,
                    "launch_equals_oracle": True, "handles_differing_from_oracle": off})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
