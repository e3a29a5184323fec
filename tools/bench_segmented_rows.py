"""Segmented Sampler.apply over byte keys (batch.sample_segmented_rows, batch.SegmentedSamplerRows).

Rows are splitmix64 words (row r = [smix(2r) | smix(2r + 1) | ...]), streams are equal-length slices as
C3 in tools/bench_paths.py.  Device events around every launch, --warmup runs then --steps timed runs,
medians with their min / max.  Every leg is one entry of the JSON document written to --out:

    c3            2^20 streams x 4096 rows of 16 bytes, k = 64: rows_ms (the rows launch), long_ms (the
                  Long-key sample_segmented launch over the same offsets, reading the same memory as
                  int64 keys), gather_ms (torch.gather of the same 2^26 winner rows by precomputed
                  indices, as 8-byte and as 16-byte elements, the faster one: the memory floor); rows_over_long, rows_over_gather.  check: the launch's
                  rows equal the torch gather at the resumed state's last writers.
    c3_plain      the same rows launch in a child process with RSV_K2_ROWS_DEFER=0: the plain gather
                  after each stream instead of the one deferred past the next stream's draws
    k4096         4096 streams x 2^17 rows, k = 4096 (one workgroup per stream), against the Long-key launch
    w64           C3's stream length and k at 64-byte rows; the stream count is the largest power of two
                  whose rows fit (2^20 streams would be 256 GiB), against the Long-key launch at that count
    update        C3's shape fed as B = 1, 2, 8 update launches into a fresh state (sum_ms), against rows_ms
    merge         8 states that each saw an eighth of every stream merged in one launch, against a device
                  copy of the same part bytes

    python tools/bench_segmented_rows.py [--streams 1048576] [--legs c3,c3_plain,k4096,w64,update,merge]
                                         [--steps 10] [--warmup 3] [--out profiles/segmented_rows/bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED = 11


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def series(torch, fn, a, before=None):
    """Timed runs of fn (before() runs outside the window): {ms, ms_min, ms_max} and the last result."""
    ms, out = [], None
    for step in range(a.warmup + a.steps):
        del out
        if before:
            before()
        t, out = timed(torch, fn)
        if step >= a.warmup:
            ms.append(t)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}, out


def put(d, name, s):
    d[name + "_ms"], d[name + "_ms_min"], d[name + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]


def make_rows(torch, dev, n_rows, W):
    from workloads import splitmix_fill

    words = torch.empty(n_rows * (W // 8), dtype=torch.int64, device=dev)
    splitmix_fill(words, 0)
    return words.view(torch.uint8).view(n_rows, W), words


def fit_streams(torch, dev, S, n, W, copies=1.0):
    """S halved until copies x (S n W) bytes fit in 85 % of the free device memory."""
    free = torch.cuda.mem_get_info(dev)[0] * 0.85
    while S > 1 and copies * S * n * W > free:
        S //= 2
    return S


def leg_stateless(torch, batch, dev, a, S, n, k, W, gather):
    """The rows launch against the Long-key launch over the same offsets (and the torch gather floor)."""
    rows, words = make_rows(torch, dev, S * n, W)
    offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    d = {"streams": S, "len": n, "k": k, "width": W, "form": "wave" if k < 512 else "workgroup"}
    s_long, ref = series(torch, lambda: batch.sample_segmented(words[:S * n], offs, k, seed=SEED), a)
    del ref
    s_rows, out = series(torch, lambda: batch.sample_segmented_rows(rows, offs, k, seed=SEED), a)
    put(d, "rows", s_rows)
    put(d, "long", s_long)
    d["rows_over_long"] = s_rows["ms"] / s_long["ms"]
    d["rows_GBps_out"] = S * k * W / s_rows["ms"] / 1e6
    # the winners' positions within their streams, from the resumed form: the check, and the indices of the
    # gather floor -- torch.gather of k positions per stream, as C3's gather_floor in tools/bench_paths.py
    st = batch.SegmentedSamplerRows(S, k, W, seed=SEED, device=dev).update(rows, offs, check_ids=False)
    loc = st.idx
    d["check"] = bool((loc >= 0).all()) and bool(torch.equal(st.rows, out[0]))
    del st
    g64 = words.view(S, n, W // 8)
    ix = loc[:, :, None].expand(S, k, W // 8)
    if not gather:
        d["check"] = d["check"] and bool(torch.equal(torch.gather(g64, 1, ix).view(torch.uint8).view(S, k, W), out[0]))
        return d, rows, offs, out[0]
    s_g, got = series(torch, lambda: torch.gather(g64, 1, ix), a)  # 8-byte elements, W / 8 per row
    d["check"] = d["check"] and bool(torch.equal(got.view(torch.uint8).view(S, k, W), out[0]))
    del got
    put(d, "gather_i64", s_g)
    floor = s_g["ms"]
    if W == 16:  # one 16-byte element per index
        c128 = words.view(torch.complex128).view(S, n)
        s_c, got = series(torch, lambda: torch.gather(c128, 1, loc), a)
        d["check"] = d["check"] and bool(torch.equal(torch.view_as_real(got).view(torch.uint8).view(S, k, W), out[0]))
        del got
        put(d, "gather_c128", s_c)
        floor = min(floor, s_c["ms"])
    d["gather_ms"] = floor
    d["rows_over_gather"] = s_rows["ms"] / floor
    return d, rows, offs, out[0]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 20)
    ap.add_argument("--legs", default="c3,c3_plain,k4096,w64,update,merge")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="print the c3 leg's rows timing only (c3_plain's child)")
    a = ap.parse_args()
    legs = a.legs.split(",")

    doc = {"bench": "segmented_rows", "steps": a.steps, "warmup": a.warmup, "legs": {}}
    if "c3_plain" in legs and not a.child:  # first: the child needs the device memory
        env = dict(os.environ, RSV_K2_ROWS_DEFER="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams),
                            "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env, capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise SystemExit("c3_plain failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        doc["legs"]["c3_plain"] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({"c3_plain": doc["legs"]["c3_plain"]}), flush=True)

    import torch

    from reservoir_amd import batch

    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented_rows needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc["device"] = torch.cuda.get_device_name(0)
    n, k, W = 4096, 64, 16

    def done(name, d):
        doc["legs"][name] = d
        print(json.dumps({name: d}), flush=True)

    if a.child:
        S = fit_streams(torch, dev, a.streams, n, W, 1.1)
        rows, _ = make_rows(torch, dev, S * n, W)
        offs = torch.arange(0, S * n + 1, n, dtype=torch.int64, device=dev)
        s_rows, _ = series(torch, lambda: batch.sample_segmented_rows(rows, offs, k, seed=SEED), a)
        d = {"streams": S, "len": n, "k": k, "width": W, "defer": os.environ.get("RSV_K2_ROWS_DEFER", "1")}
        put(d, "rows", s_rows)
        print(json.dumps(d), flush=True)
        return

    if "k4096" in legs:
        d, rows, offs, out = leg_stateless(torch, batch, dev, a, 4096, 1 << 17, 4096, 16, False)
        done("k4096", d)
        del rows, offs, out
        torch.cuda.empty_cache()
    if "w64" in legs:
        S64 = fit_streams(torch, dev, a.streams, n, 64, 1.1)
        d, rows, offs, out = leg_stateless(torch, batch, dev, a, S64, n, k, 64, True)
        done("w64", d)
        del rows, offs, out
        torch.cuda.empty_cache()
    if not set(legs) & {"c3", "update", "merge"}:
        S = 0
    else:
        S = fit_streams(torch, dev, a.streams, n, W, 1.1)
        d, rows, offs, ref = leg_stateless(torch, batch, dev, a, S, n, k, W, True)
        if "c3_plain" in doc["legs"] and doc["legs"]["c3_plain"]["streams"] == S:
            d["plain_ms"] = doc["legs"]["c3_plain"]["rows_ms"]
            d["deferred_over_plain"] = d["rows_ms"] / d["plain_ms"]
        done("c3", d)
        rows_ms = d["rows_ms"]

    if "update" in legs and S:
        st = batch.SegmentedSamplerRows(S, k, W, seed=SEED, device=dev)

        def reset():
            st.idx.fill_(-1)
            st.next.zero_()

        r3 = rows.view(S, n, W)
        for B in (1, 2, 8):
            # B = 1 feeds the rows themselves; the column slices of B > 1 are copies, so the stream count
            # is what fits beside the rows
            Sb = S if B == 1 else min(S, fit_streams(torch, dev, S, n, W, 1.0))
            w = n // B
            poffs = torch.arange(0, Sb * w + 1, w, dtype=torch.int64, device=dev)
            parts = [rows] if B == 1 else [r3[:Sb, t * w:(t + 1) * w].contiguous().view(-1, W) for t in range(B)]
            runs = []
            for step in range(a.warmup + a.steps):
                reset()
                per = [timed(torch, lambda t=t: st.update(parts[t], poffs, check_ids=False))[0] for t in range(B)]
                if step >= a.warmup:
                    runs.append(per)
            sums = [sum(r) for r in runs]
            d = {"streams": Sb, "len": n, "k": k, "width": W, "batches": B,
                 "launch_ms": [statistics.median(r[t] for r in runs) for t in range(B)],
                 "sum_ms": statistics.median(sums), "sum_ms_min": min(sums), "sum_ms_max": max(sums),
                 "check": bool(torch.equal(st.rows[:Sb], ref[:Sb]) and bool((st.next[:Sb] == n).all()))}
            if Sb == S:
                d["stateless_rows_ms"] = rows_ms
                d["ratio"] = d["sum_ms"] / rows_ms
            done(f"update_{B}", d)
            del parts
            torch.cuda.empty_cache()
        del st

    if "merge" in legs and S:
        P = 8
        w = n // P
        poffs = torch.arange(0, S * w + 1, w, dtype=torch.int64, device=dev)
        r3 = rows.view(S, n, W)
        pr, pi, pn = [], [], []
        for t in range(P):
            piece = r3[:, t * w:(t + 1) * w].contiguous().view(-1, W)
            s = batch.SegmentedSamplerRows(S, k, W, seed=SEED, device=dev)
            s.update(piece, poffs, bases=torch.full((S,), t * w, dtype=torch.int64, device=dev), check_ids=False)
            pr.append(s.rows), pi.append(s.idx), pn.append(s.next)
            del piece
        del rows, r3
        pr, pi, pn = torch.stack(pr), torch.stack(pi), torch.stack(pn)
        cr, ci, cn = torch.empty_like(pr), torch.empty_like(pi), torch.empty_like(pn)
        st = batch.SegmentedSamplerRows(S, k, W, seed=SEED, device=dev)
        torch.cuda.synchronize()

        def reset():
            st.idx.fill_(-1)
            st.next.zero_()

        def copy():
            cr.copy_(pr)
            ci.copy_(pi)
            cn.copy_(pn)

        s_m, _ = series(torch, lambda: st.merge(pr, pi, pn), a, before=reset)
        ok = bool(torch.equal(st.rows, ref) and bool((st.idx >= 0).all()) and bool((st.next == n).all()))
        s_r, _ = series(torch, lambda: st.merge(pr, pi, pn), a)  # no slot is beaten: nothing is written
        s_c, _ = series(torch, copy, a)
        nbytes = pr.numel() + (pi.numel() + pn.numel()) * 8
        d = {"streams": S, "len": n, "k": k, "width": W, "parts": P, "part_bytes": nbytes, "check": ok}
        put(d, "merge", s_m)
        put(d, "remerge", s_r)
        put(d, "copy", s_c)
        d["merge_over_copy"] = s_m["ms"] / s_c["ms"]
        d["merge_GBps"], d["copy_GBps"] = nbytes / s_m["ms"] / 1e6, nbytes / s_c["ms"] / 1e6
        done("merge", d)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not all(d.get("check", True) for d in doc["legs"].values()):
        raise SystemExit("a leg's check failed")


if __name__ == "__main__":
    main()
