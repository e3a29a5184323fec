"""Segmented Sampler.distinct for any B (rsv_distinct_segmented_candidates, batch.SegmentedObjectDistinct).

Four cases, all in one run (device events around every launch, medians over --steps after --warmup):

    c3        2^20 streams x 4096 int64 hashes, ~30 % repeats, k = 64: one candidate launch on fresh rows (the
              counts zeroed before each, outside the timed window) against batch.distinct_segmented over the same
              words as identity keys -- the same bytes read, the same merges run; the difference is the emission
              and its writes.  cap is batch.segmented_candidate_cap; rerun_rate is the share of segments that
              overflowed it, candidates_per_stream the mean count, and over the first --replayed streams
              reference_admissions is what RandomValues itself admits.
    k4096     4096 streams x 2^17, k = 4096, the same pair.
    feed      c3's streams cut into 8 pieces and fed as 8 launches into one state (the shadow's bound alone, as
              a caller who has not replayed yet): launch_ms[8], sum_ms.
    handles   --handles streams of 4096 strings through one SegmentedObjectDistinct.update (launch, read-back,
              map, replay: host clock) against one Sampler.distinct(key_type="object") handle per stream fed the
              same elements and hashes; per stream, and checked equal.

    python tools/bench_segmented_object_distinct.py [--streams 1048576] [--len 4096] [--k 64] [--steps 10]
                                                    [--warmup 3] [--handles 256] [--out FILE]
prints one JSON line (and writes it to --out).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_segmented_distinct import make_keys  # noqa: E402
from bench_segmented_distinct_state import pieces, timed  # noqa: E402


def spread(xs):
    return {"ms": statistics.median(xs), "ms_min": min(xs), "ms_max": max(xs)}


def pair(torch, batch, S, n, k, dup, steps, warmup, replayed):
    """The candidate launch against the Long-key stateless launch over the same words."""
    import numpy as np

    from reservoir_amd.values import RandomValues

    dev = torch.device("cuda", 0)
    keys = make_keys(torch, dev, S, n, dup)
    flat = keys.view(-1)
    offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
    cap = batch.segmented_candidate_cap(k, n)
    state = (torch.empty((S, k), dtype=torch.int64, device=dev), torch.zeros(S, dtype=torch.int64, device=dev), None, None)
    torch.cuda.synchronize()
    cand, keyed = [], []
    for step in range(warmup + steps):
        state[1].zero_()
        ms, out = timed(torch, lambda: batch.distinct_segmented_candidates(flat, offs, k, 11, cap=cap, state=state))
        ms2, ref = timed(torch, lambda: batch.distinct_segmented(flat, offs, k, seed=11, hash="identity"))
        if step >= warmup:
            cand.append(ms), keyed.append(ms2)
        if step < warmup + steps - 1:
            del out, ref
    pos, hs, counts = out
    # the shadow is the Long-key launch's hash column wherever nothing overflowed
    fits = counts <= cap
    same = bool(torch.equal(state[1][fits], ref[2][fits]) and torch.equal(state[0][fits], ref[1][fits]))
    # the reference's own admissions over the first streams, and the replay of the candidates against it
    R = min(replayed, S)
    hk = keys[:R].cpu().numpy()
    sub = batch.distinct_segmented_candidates(keys[:R].reshape(-1), offs[:R + 1], k, 11, cap=n)
    sp, sh, sc = (t.cpu().numpy() for t in sub)
    adm, exact = 0, True
    for s in range(R):
        c = int(sc[s])
        p = sp[s, :c] - s * n
        v = RandomValues(k)
        for e, h in zip(hk[s, p].tolist(), sh[s, :c].tolist()):  # (an element that is no candidate is not admitted)
            adm += v.admits(e, h)
            v.sample(e, h)
        exact &= v.hashes() == ref[1][s, :int(ref[2][s])].cpu().tolist()
    c = spread(cand)
    kd = spread(keyed)
    total = float(counts.sum())
    return {"streams": S, "len": n, "k": k, "dup": dup, "cap": cap, "out_bytes": S * cap * 16,
            "candidates": c, "long_key_stateless": kd, "candidates_over_long_key": c["ms"] / kd["ms"],
            "candidates_GBps": S * n * 8 / c["ms"] / 1e6, "us_per_stream": c["ms"] * 1e3 / S,
            "candidates_per_stream": total / S, "max_candidates": int(counts.max()),
            "rerun_rate": float((~fits).sum()) / S, "emitted_bytes": int(min(total, S * cap) * 16),
            "replayed_streams": R, "reference_admissions_per_stream": adm / R,
            "candidates_per_stream_replayed": float(np.mean(sc)), "shadow_equals_long_key_hashes": same,
            "replay_equals_long_key_set": bool(exact)}, keys


def feed(torch, batch, keys, k, B, steps, warmup):
    dev = keys.device
    S, n = keys.shape
    parts, poffs = pieces(torch, keys, B)
    cap = batch.segmented_candidate_cap(k, n // B)
    state = (torch.empty((S, k), dtype=torch.int64, device=dev), torch.zeros(S, dtype=torch.int64, device=dev), None, None)
    runs, over = [], []
    for step in range(warmup + steps):
        state[1].zero_()
        per, ov = [], []
        for t in range(B):
            ms, out = timed(torch, lambda t=t: batch.distinct_segmented_candidates(parts[t], poffs, k, 11, cap=cap,
                                                                                   state=state))
            per.append(ms)
            ov.append(float((out[2] > cap).sum()) / S)
            del out
        if step >= warmup:
            runs.append(per), over.append(ov)
    sums = [sum(r) for r in runs]
    return {"batches": B, "cap": cap, "launch_ms": [statistics.median(r[t] for r in runs) for t in range(B)],
            "sum_ms": statistics.median(sums), "sum_ms_min": min(sums), "sum_ms_max": max(sums),
            "rerun_rate_per_launch": over[-1]}


def handles(torch, batch, H, n, k):
    import numpy as np

    from reservoir_amd import Sampler

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 3 * n // 4, size=(H, n))
    elems = [f"user-{s}-{i}" for s in range(H) for i in ids[s].tolist()]
    hashes = np.array([hash(e) for e in elems], dtype=np.int64)
    hd = torch.from_numpy(hashes).to(dev)
    offs = np.arange(0, H * n + 1, n, dtype=np.int64)
    torch.cuda.synchronize()
    seg = []
    for rep in range(3):
        so = batch.SegmentedObjectDistinct(H, k, 11, device=dev)
        t0 = time.perf_counter()
        so.update(elems, hd, offs)
        torch.cuda.synchronize()
        seg.append((time.perf_counter() - t0) * 1e6 / H)
    per, same = [], True
    for s in range(H):
        sub, hv = elems[s * n:(s + 1) * n], hd[s * n:(s + 1) * n]
        t0 = time.perf_counter()
        d = Sampler.distinct(k, key_type="object", seed=11 + s)()
        d.sample_all(sub, hashes=hv)
        got = d.result()
        per.append((time.perf_counter() - t0) * 1e6)
        same &= got == so.result(s)
    warm = per[min(8, H - 1):]  # the first handles pay one-time set-up
    return {"streams": H, "len": n, "k": k, "segmented_us_per_stream": statistics.median(seg),
            "segmented_us_per_stream_min": min(seg), "handles_us_per_stream": statistics.median(warm),
            "handles_us_per_stream_min": min(warm), "handles_over_segmented": statistics.median(warm) / statistics.median(seg),
            "info": so.info(), "equal": bool(same)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--handles", type=int, default=256)
    ap.add_argument("--replayed", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from reservoir_amd import batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_object_distinct needs a GPU")
    torch.cuda.set_device(0)
    out = {"bench": "segmented_object_distinct", "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    out["c3"], keys = pair(torch, batch, a.streams, a.len, a.k, a.dup, a.steps, a.warmup, a.replayed)
    out["feed"] = feed(torch, batch, keys, a.k, 8, a.steps, a.warmup)
    del keys
    torch.cuda.empty_cache()
    out["k4096"], keys = pair(torch, batch, max(1, a.streams >> 8), a.len << 5, 4096, a.dup, a.steps, a.warmup, 4)
    del keys
    torch.cuda.empty_cache()
    out["handles"] = handles(torch, batch, a.handles, a.len, a.k)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ok = all(out[c]["shadow_equals_long_key_hashes"] and out[c]["replay_equals_long_key_set"] for c in ("c3", "k4096"))
    if not (ok and out["handles"]["equal"]):
        raise SystemExit("a check failed")


if __name__ == "__main__":
    main()
