"""The by-id front door (batch.group_by_stream, update_by_id) against what a caller can do today, one session.

Grouping alone, n ids over S rows, int32 and int64 ids:
    uniform   S = 2^20, ids uniform over the rows
    zipf      S = 4096, ids from the continuous 1 / (i + 1) law (inverse CDF: floor((S + 1)^u) - 1)
against torch.sort(ids, stable=True) over the same tensor.  model_bytes is what the design moves -- per pass the
histogram's read, the scatter's read and its 8-byte write: (2 w + 8) n for the first pass over w-byte ids, 20 n for
each later one -- and GBps = model_bytes / the time.  passes[] repeats the uniform int32 measurement at S = 255,
65535 and 2^20 (one, two and three passes), which prices a pass.

update_by_id end to end at k = 64, int64 keys and ids, both shapes:
    SegmentedSampler.update_by_id   against   torch.sort(stable) -> searchsorted to dense offsets -> keys.index_select
    SegmentedDistinct.update_by_id            -> update(check_ids=False)   (today's route without a host wait)
The state is reset before every timed call, outside the timed window, and the two routes' states are compared.

Every figure is the minimum of --reps (>= 5) repetitions after --warmup, the two sides of a comparison interleaved
call by call, timed by device events; min and max of each side are kept beside it (the spread).

    python tools/bench_group_by_stream.py [--n 67108864] [--reps 7] [--warmup 2] [--out profiles/group_by_stream/bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def interleaved(torch, fns, reps, warmup, before=None):
    """ms lists of fns, called in turn reps times after warmup rounds; before(): untimed, ahead of every call."""
    ms = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            if before:
                before(i)
            t, out = timed(torch, fn)
            del out
            if r >= warmup:
                ms[i].append(t)
    return ms


def stats(ms):
    return {"ms": min(ms), "ms_max": max(ms), "runs": len(ms)}


def plan(S):
    bits = max(1, int(S).bit_length())
    passes = (bits + 7) // 8
    return passes, (bits + passes - 1) // passes


def model_bytes(n, S, width):
    passes, _ = plan(S)
    return n * ((2 * width + 8) + 20 * (passes - 1))


def make_ids(torch, dev, shape, n, S, dtype, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if shape == "uniform":
        return torch.randint(0, S, (n,), generator=g, device=dev, dtype=torch.int64).to(dtype)
    u = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    return (torch.exp(u * math.log(S + 1)).floor().to(torch.int64) - 1).clamp_(0, S - 1).to(dtype)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_by_stream", "bench.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")

    import torch

    from reservoir_amd import batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_group_by_stream needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, k = a.n, a.k
    shapes = {"uniform": 1 << 20, "zipf": 4096}
    out = {"bench": "group_by_stream", "n": n, "k": k, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "grouping": [], "passes": [], "update_by_id": []}

    for shape, S in shapes.items():
        for dtype in (torch.int32, torch.int64):
            ids = make_ids(torch, dev, shape, n, S, dtype, 1)
            torch.cuda.synchronize()
            g, s = interleaved(torch, [lambda: batch.group_by_stream(ids, S), lambda: torch.sort(ids, stable=True)],
                               a.reps, a.warmup)
            offs, order = batch.group_by_stream(ids, S)
            ref = torch.sort(ids, stable=True)
            check = bool(torch.equal(order.to(torch.int64), ref[1])) and int(offs[-1]) == n
            del offs, order, ref
            mb = model_bytes(n, S, ids.element_size())
            passes, bits = plan(S)
            out["grouping"].append({"shape": shape, "S": S, "ids": str(dtype).split(".")[1], "passes": passes,
                                    "digit_bits": bits, "group": stats(g), "torch_sort_stable": stats(s),
                                    "group_over_sort": min(g) / min(s), "model_bytes": mb,
                                    "model_GBps": mb / min(g) / 1e6, "check": check})
            print(json.dumps(out["grouping"][-1]), flush=True)
            del ids
            torch.cuda.empty_cache()

    for S in (255, 65535, 1 << 20):
        ids = make_ids(torch, dev, "uniform", n, S, torch.int32, 2)
        torch.cuda.synchronize()
        (g,) = interleaved(torch, [lambda: batch.group_by_stream(ids, S)], a.reps, a.warmup)
        mb = model_bytes(n, S, 4)
        out["passes"].append({"S": S, "passes": plan(S)[0], "digit_bits": plan(S)[1], "group": stats(g),
                              "model_bytes": mb, "model_GBps": mb / min(g) / 1e6})
        print(json.dumps(out["passes"][-1]), flush=True)
        del ids
        torch.cuda.empty_cache()

    def today(state, keys, ids, S):
        sid, perm = torch.sort(ids, stable=True)
        offs = torch.searchsorted(sid, torch.arange(S + 1, device=dev, dtype=ids.dtype))
        return state.update(keys.index_select(0, perm), offs, check_ids=False)

    for shape, S in shapes.items():
        ids = make_ids(torch, dev, shape, n, S, torch.int64, 3)
        g = torch.Generator(device=dev)
        g.manual_seed(4)
        keys = torch.randint(-2**62, 2**62, (n,), generator=g, device=dev, dtype=torch.int64)
        for name, make, reset in (
                ("SegmentedSampler", lambda: batch.SegmentedSampler(S, k, seed=11, device=dev),
                 lambda st: (st.idx.fill_(-1), st.next.zero_())),
                ("SegmentedDistinct", lambda: batch.SegmentedDistinct(S, k, seed=11, device=dev),
                 lambda st: st.counts.zero_())):
            mine, theirs = make(), make()
            sides = [mine, theirs]
            torch.cuda.synchronize()
            m, t = interleaved(torch, [lambda: mine.update_by_id(keys, ids), lambda: today(theirs, keys, ids, S)],
                               a.reps, a.warmup, before=lambda i: reset(sides[i]))
            torch.cuda.synchronize()
            counts = mine.counts
            live = torch.arange(k, device=dev)[None, :] < counts[:, None]
            check = all(bool(torch.equal(x if x.dim() == 1 else x * live, y if y.dim() == 1 else y * live))
                        for x, y in zip(mine._state(), theirs._state()))
            out["update_by_id"].append({"state": name, "shape": shape, "S": S, "update_by_id": stats(m),
                                        "sort_gather_update": stats(t), "by_id_over_today": min(m) / min(t),
                                        "check": check})
            print(json.dumps(out["update_by_id"][-1]), flush=True)
            del mine, theirs, sides
            torch.cuda.empty_cache()
        del ids, keys
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ok = all(r["check"] for r in out["grouping"] + out["update_by_id"])
    if not ok:
        raise SystemExit("a result differs between the two routes")


if __name__ == "__main__":
    main()
