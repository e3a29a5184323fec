"""Resumed segmented Sampler.apply (batch.SegmentedSampler: rsv_sample_segmented_update / _merge).

--mode update (default): S streams x len int64 keys (splitmix64, as C3 in tools/bench_paths.py) cut
into B equal batches and fed as B update launches into one fresh state, for every B of --batches,
against one stateless rsv_sample_segmented launch over the same keys in the same run.  Device events
around every launch, --warmup runs then --steps timed runs of the B launches (idx and next are reset
before each run, outside the timed windows).  One JSON line per B:

    launch_ms[B]      median time of each of the B launches
    sum_ms            median over the runs of the sum of the B launch times (sum_ms_min / _max: the spread)
    stateless_ms      median of one stateless launch, timed just before (stateless_ms_min / _max)
    ratio             sum_ms / stateless_ms
    state_bytes       B x S x 24 x k: every launch reading idx and writing key and idx of every slot, an
                      upper bound (only slots with a winner are read, only slots that win are written)
    model_ms          stateless_ms + state_bytes / (8 B x elements / stateless_ms): the state moved at the
                      rate the stateless launch itself achieved; model_ratio = model_ms / stateless_ms
    check             the state equals the stateless result (keys; every idx >= 0; next = len)

--mode merge: P parts (states that each saw one of P index ranges of every stream, fed with bases)
merged in one launch into a fresh state (merge_ms) and once more into the merged state (remerge_ms:
no slot is beaten, nothing is written), against a device copy of the same part bytes in the same run
(copy_ms); merge_over_copy = merge_ms / copy_ms.  check: the merged state equals the stateless result
over the whole streams.

    python tools/bench_segmented_state.py [--mode update] [--streams 1048576] [--len 4096] [--k 64]
                                          [--batches 1,2,8] [--steps 10] [--warmup 3] [--out FILE]
    python tools/bench_segmented_state.py --mode merge [--parts 8] [--streams 1048576] [--len 2048] [--k 64]
prints its JSON lines (and appends them to --out).
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


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def pieces(torch, keys, B):
    """B contiguous (S, len / B) column slices with their offsets (B = 1: the keys themselves)."""
    S, n = keys.shape
    w = n // B
    offs = torch.arange(0, S * w + 1, w, dtype=torch.int64, device=keys.device)
    if B == 1:
        return [keys.view(-1)], offs
    return [keys[:, t * w:(t + 1) * w].contiguous().view(-1) for t in range(B)], offs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["update", "merge"], default="update")
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=None)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from reservoir_amd import batch
    from workloads import splitmix_fill

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_state needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S, k = a.streams, a.k
    n = a.len if a.len is not None else (4096 if a.mode == "update" else 2048)
    Bs = [int(b) for b in a.batches.split(",")] if a.mode == "update" else [a.parts]
    if any(n % B for B in Bs):
        raise SystemExit("--len must be a multiple of the number of pieces")
    if n < k:
        raise SystemExit("--len must be at least --k (the check compares full rows)")
    flat = torch.empty(S * n, dtype=torch.int64, device=dev)
    splitmix_fill(flat, 0)
    keys = flat.view(S, n)
    offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def stateless():
        return batch.sample_segmented(flat, offs, k, seed=11)

    def same(st, ref):
        return bool(torch.equal(st.keys, ref[0]) and bool((st.idx >= 0).all()) and bool((st.next == n).all()))

    def reset(st):
        st.idx.fill_(-1)
        st.next.zero_()

    base = {"bench": "segmented_state", "mode": a.mode, "streams": S, "len": n, "k": k,
            "form": "wave" if k < 512 else "workgroup", "steps": a.steps, "warmup": a.warmup,
            "device": torch.cuda.get_device_name(0)}
    st = batch.SegmentedSampler(S, k, seed=11, device=dev)
    lines = []

    if a.mode == "update":
        for B in Bs:
            parts, poffs = pieces(torch, keys, B)
            torch.cuda.synchronize()
            sl = []
            for step in range(a.warmup + a.steps):
                ms, ref = timed(torch, stateless)
                if step >= a.warmup:
                    sl.append(ms)
                if step < a.warmup + a.steps - 1:
                    del ref
            runs = []
            for step in range(a.warmup + a.steps):
                reset(st)
                per = [timed(torch, lambda t=t: st.update(parts[t], poffs, check_ids=False))[0] for t in range(B)]
                if step >= a.warmup:
                    runs.append(per)
            sums = [sum(r) for r in runs]
            launch = [statistics.median(r[t] for r in runs) for t in range(B)]
            sl_ms, sum_ms = statistics.median(sl), statistics.median(sums)
            state_bytes = B * S * 24 * k
            rate = S * n * 8 / sl_ms  # bytes per ms of the stateless launch
            model = sl_ms + state_bytes / rate
            lines.append(dict(base, batches=B, launch_ms=launch, sum_ms=sum_ms, sum_ms_min=min(sums),
                              sum_ms_max=max(sums), stateless_ms=sl_ms, stateless_ms_min=min(sl),
                              stateless_ms_max=max(sl), ratio=sum_ms / sl_ms, state_bytes=state_bytes,
                              stateless_GBps=rate / 1e6, model_ms=model, model_ratio=model / sl_ms,
                              sum_over_model=sum_ms / model, check=same(st, ref)))
            del parts, ref
            torch.cuda.empty_cache()
    else:
        P = Bs[0]
        ref = stateless()
        parts, poffs = pieces(torch, keys, P)
        w = n // P
        pk, pi, pn = [], [], []
        for t in range(P):
            s = batch.SegmentedSampler(S, k, seed=11, device=dev)
            s.update(parts[t], poffs, bases=torch.full((S,), t * w, dtype=torch.int64, device=dev), check_ids=False)
            pk.append(s.keys), pi.append(s.idx), pn.append(s.next)
        pk, pi, pn = torch.stack(pk), torch.stack(pi), torch.stack(pn)
        ck, ci, cn = torch.empty_like(pk), torch.empty_like(pi), torch.empty_like(pn)
        del parts, keys, flat
        torch.cuda.synchronize()

        def copy():
            ck.copy_(pk)
            ci.copy_(pi)
            cn.copy_(pn)

        mg, rm, cp = [], [], []
        for step in range(a.warmup + a.steps):
            reset(st)
            t0 = timed(torch, lambda: st.merge(pk, pi, pn))[0]
            if step == 0 and not same(st, ref):
                raise SystemExit("the merged state and the stateless launch disagree")
            t1 = timed(torch, lambda: st.merge(pk, pi, pn))[0]
            t2 = timed(torch, copy)[0]
            if step >= a.warmup:
                mg.append(t0), rm.append(t1), cp.append(t2)
        nbytes = (pk.numel() + pi.numel() + pn.numel()) * 8
        m, c = statistics.median(mg), statistics.median(cp)
        lines.append(dict(base, parts=P, part_bytes=nbytes, merge_ms=m, merge_ms_min=min(mg), merge_ms_max=max(mg),
                          remerge_ms=statistics.median(rm), copy_ms=c, copy_ms_min=min(cp), copy_ms_max=max(cp),
                          merge_GBps=nbytes / m / 1e6, copy_GBps=nbytes / c / 1e6, merge_over_copy=m / c,
                          check=same(st, ref)))
    for out in lines:
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    if not all(out["check"] for out in lines):
        raise SystemExit("the state and the stateless launch disagree")


if __name__ == "__main__":
    main()
