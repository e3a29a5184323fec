"""Keyless segmented Sampler.apply (batch.sample_segmented_indexed, rsv_sample_segmented_indexed_update / _merge,
batch.SegmentedObjectSampler).

Only offsets reach the device, so a shape costs 8 bytes per stream whatever its streams' lengths.  Device events
around every launch, --warmup runs then --steps timed runs, medians with their min / max.  RSV_K2_SPLIT_LEN is read
once per process, so every split setting is measured in a child process of this script; a group of settings that
are to be compared is run round-robin, --rounds times, so that their spreads come from one session.  The document
written to --out holds one entry per leg:

    c3        2^20 streams x 4096, k = 64: the keyless launch at the built-in split length and with the split off
              (every round of each), and in the first child the keyed sample_segmented over int64 keys with the same
              offsets, alternated with the keyless launch; keyless_over_keyed
    skew      2^16 streams x 4096 plus one stream of 2^32 indices, at k = 64 and k = 1024, with the split off and at
              2^18, 2^20 and 2^22 (the unsplit launch of one 2^32-index stream runs for seconds: it is timed
              --slow-steps times without a warm-up)
    k4096     4096 streams x 2^17 at k = 4096 (one workgroup per stream)
    update    C3's streams fed as 1, 2 and 8 update launches into a fresh state (sum_ms, last_ms: the steady
              per-launch time), against the stateless keyless launch
    merge     8 states that each saw an eighth of every C3 stream merged in one launch, against a device copy of
              the same part bytes
    objects   256 streams x 4096 strings end to end through SegmentedObjectSampler (one update), against one
              Sampler(key_type="object") handle per stream (host wall clock around a device synchronise)
    keyed_ab  with --ab-lib: the keyed C3 launch under that library (the parent commit's build) and under this
              tree's, alternating child processes; one JSON line per child in --ab-out

    python tools/bench_segmented_indexed.py [--legs c3,skew,k4096,update,merge,objects] [--ab-lib PATH]
           [--steps 10] [--warmup 3] [--rounds 2] [--out profiles/segmented_indexed/bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 11
C3_S, C3_L, C3_K = 1 << 20, 4096, 64


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def series(torch, fn, steps, warmup, before=None):
    ms = []
    for step in range(warmup + steps):
        if before:
            before()
        t, _ = timed(torch, fn)
        if step >= warmup:
            ms.append(t)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": len(ms)}


def equal_offsets(torch, dev, S, L):
    return torch.arange(S + 1, dtype=torch.int64, device=dev) * L


# ---- the legs, each inside a child process ---------------------------------------------------------
def leg_c3(torch, batch, dev, a):
    offs = equal_offsets(torch, dev, a.streams, C3_L)
    out = {"keyless": series(torch, lambda: batch.sample_segmented_indexed(offs, C3_K, SEED), a.steps, a.warmup)}
    if a.keyed:
        keys = torch.empty(a.streams * C3_L, dtype=torch.int64, device=dev).zero_()
        run = {"keyed": lambda: batch.sample_segmented(keys, offs, C3_K, SEED),
               "keyless": lambda: batch.sample_segmented_indexed(offs, C3_K, SEED)}
        ms = {"keyed": [], "keyless": []}
        for step in range(a.warmup + a.steps):   # alternated
            for name, fn in run.items():
                t, _ = timed(torch, fn)
                if step >= a.warmup:
                    ms[name].append(t)
        for name, v in ms.items():
            out[name + "_alternated"] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "runs": len(v)}
        out["keyless_over_keyed"] = out["keyless_alternated"]["ms"] / out["keyed_alternated"]["ms"]
    return out


def leg_skew(torch, batch, dev, a):
    lens = torch.full((a.skew_streams + 1,), C3_L, dtype=torch.int64, device=dev)
    lens[a.skew_streams // 2] = 1 << 32
    offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)])
    slow = os.environ.get("RSV_K2_SPLIT_LEN") == "0"
    out = {}
    for k in (64, 1024):
        steps, warmup = (a.slow_steps, 0) if slow else (a.steps, a.warmup)
        out[f"k{k}"] = series(torch, lambda: batch.sample_segmented_indexed(offs, k, SEED), steps, warmup)
    return out


def leg_k4096(torch, batch, dev, a):
    offs = equal_offsets(torch, dev, 4096, 1 << 17)
    return series(torch, lambda: batch.sample_segmented_indexed(offs, 4096, SEED), a.steps, a.warmup)


def _update_call(torch, L, dev, offs, k, idx, nxt, hits, hc):
    from reservoir_amd import _native as N

    p = lambda t: C.c_void_p(t.data_ptr())
    N.check(L.rsv_sample_segmented_indexed_update(p(offs), None, None, offs.numel() - 1, idx.shape[0], k, SEED, 0,
                                                  p(idx), p(nxt), p(hits), p(hc),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def leg_update(torch, batch, dev, a):
    from reservoir_amd import _native as N

    L = N.load()
    S = a.streams
    idx = torch.empty((S, C3_K), dtype=torch.int64, device=dev)
    nxt = torch.empty(S, dtype=torch.int64, device=dev)
    hits = torch.empty((S, C3_K), dtype=torch.int64, device=dev)
    hc = torch.empty(S, dtype=torch.int64, device=dev)
    whole = equal_offsets(torch, dev, S, C3_L)
    out = {"stateless": series(torch, lambda: batch.sample_segmented_indexed(whole, C3_K, SEED), a.steps, a.warmup)}
    for B in (1, 2, 8):
        offs = equal_offsets(torch, dev, S, C3_L // B)
        sums, lasts = [], []
        for step in range(a.warmup + a.steps):
            idx.fill_(-1)
            nxt.zero_()
            ts = [timed(torch, lambda: _update_call(torch, L, dev, offs, C3_K, idx, nxt, hits, hc))[0] for _ in range(B)]
            if step >= a.warmup:
                sums.append(sum(ts))
                lasts.append(ts[-1])
        out[f"B{B}"] = {"sum_ms": statistics.median(sums), "sum_ms_min": min(sums), "sum_ms_max": max(sums),
                        "last_ms": statistics.median(lasts), "sum_over_stateless": statistics.median(sums) / out["stateless"]["ms"]}
    got, _ = batch.sample_segmented_indexed(whole, C3_K, SEED)
    out["check_idx_equals_stateless"] = bool(torch.equal(got, idx))
    return out


def leg_merge(torch, batch, dev, a):
    from reservoir_amd import _native as N

    L = N.load()
    S, P = a.streams, 8
    p = lambda t: C.c_void_p(t.data_ptr())
    part_idx = torch.full((P, S, C3_K), -1, dtype=torch.int64, device=dev)
    part_next = torch.zeros((P, S), dtype=torch.int64, device=dev)
    hits = torch.empty((S, C3_K), dtype=torch.int64, device=dev)
    hc = torch.empty(S, dtype=torch.int64, device=dev)
    offs = equal_offsets(torch, dev, S, C3_L // P)
    for q in range(P):   # state q saw the q-th eighth of every stream
        part_next[q].fill_(q * (C3_L // P))
        _update_call(torch, L, dev, offs, C3_K, part_idx[q], part_next[q], hits, hc)
    idx = torch.empty((S, C3_K), dtype=torch.int64, device=dev)
    nxt = torch.empty(S, dtype=torch.int64, device=dev)
    src = torch.empty((S, C3_K), dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fresh():
        idx.fill_(-1)
        nxt.zero_()

    def merge():
        N.check(L.rsv_sample_segmented_indexed_merge(p(part_idx), p(part_next), P, S, C3_K, p(idx), p(nxt), p(src), st))

    out = {"merge": series(torch, merge, a.steps, a.warmup, before=fresh)}
    dst_i, dst_n = torch.empty_like(part_idx), torch.empty_like(part_next)
    out["copy"] = series(torch, lambda: (dst_i.copy_(part_idx), dst_n.copy_(part_next)), a.steps, a.warmup)
    out["part_bytes"] = part_idx.numel() * 8 + part_next.numel() * 8
    out["merge_over_copy"] = out["merge"]["ms"] / out["copy"]["ms"]
    got, _ = batch.sample_segmented_indexed(equal_offsets(torch, dev, S, C3_L), C3_K, SEED)
    out["check_idx_equals_stateless"] = bool(torch.equal(got, idx))
    return out


def leg_objects(torch, batch, dev, a):
    import numpy as np

    from reservoir_amd import Sampler

    S, n, k = 256, 4096, 64
    elements = [f"user-{i}" for i in range(S * n)]
    offs = np.arange(S + 1, dtype=np.int64) * n

    def segmented():
        st = batch.SegmentedObjectSampler(S, k, SEED, device=dev)
        st.update(elements, offs)
        return st.results()

    def handles():
        res = []
        for s in range(S):
            h = Sampler(k, seed=SEED, stream_id=s, key_type="object")()
            h.sample_all(elements[s * n:(s + 1) * n])
            res.append(list(h.result()))
        return res

    out = {}
    for name, fn in (("segmented", segmented), ("handles", handles)):
        ms = []
        for step in range(1 + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if step:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": len(ms)}
        out[name + "_result"] = res
    out["check_equal"] = out.pop("segmented_result") == out.pop("handles_result")
    out["handles_over_segmented"] = out["handles"]["ms"] / out["segmented"]["ms"]
    return out


def leg_keyed(torch, batch, dev, a):
    """The keyed C3 launch through a binding of its own, so that a library built before the keyless entry points
    existed loads too (--lib)."""
    from reservoir_amd import _native as N

    lib = C.CDLL(os.path.abspath(a.lib) if a.lib else N.LIB_PATH)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    lib.rsv_sample_segmented.argtypes = [vp, vp, i64, i32, i32, u64, u64, vp, vp, vp]
    lib.rsv_sample_segmented.restype = i32
    offs = equal_offsets(torch, dev, a.streams, C3_L)
    keys = torch.empty(a.streams * C3_L, dtype=torch.int64, device=dev).zero_()
    out = torch.empty((a.streams, C3_K), dtype=torch.int64, device=dev)
    counts = torch.empty(a.streams, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        rc = lib.rsv_sample_segmented(keys.data_ptr(), offs.data_ptr(), a.streams, 8, C3_K, SEED, 0, out.data_ptr(),
                                      counts.data_ptr(), st)
        assert rc == 0, rc

    return series(torch, launch, a.steps, a.warmup)


LEGS = {"c3": leg_c3, "skew": leg_skew, "k4096": leg_k4096, "update": leg_update, "merge": leg_merge,
        "objects": leg_objects, "keyed": leg_keyed}


def child(a):
    import torch

    from reservoir_amd import batch

    assert torch.cuda.is_available(), "the benchmark needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"leg": a.child, "split_len_env": os.environ.get("RSV_K2_SPLIT_LEN"), "lib": a.lib or "tree",
           "device": torch.cuda.get_device_name(0), "result": LEGS[a.child](torch, batch, dev, a)}
    print("RESULT " + json.dumps(out), flush=True)


# ---- the driver -----------------------------------------------------------------------------------
def run_child(a, leg, split=None, lib=None, keyed=False):
    env = {k: v for k, v in os.environ.items() if k != "RSV_K2_SPLIT_LEN"}
    if split is not None:
        env["RSV_K2_SPLIT_LEN"] = str(split)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--streams", str(a.streams), "--skew-streams", str(a.skew_streams), "--slow-steps", str(a.slow_steps)]
    if lib:
        cmd += ["--lib", lib]
    if keyed:
        cmd += ["--keyed"]
    print(f"[bench] {leg} split={split} lib={lib or 'tree'}", flush=True)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        raise RuntimeError(f"{leg} (split={split}) failed with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,skew,k4096,update,merge,objects")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--slow-steps", type=int, default=1)
    ap.add_argument("--streams", type=int, default=C3_S)
    ap.add_argument("--skew-streams", type=int, default=1 << 16)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmented_indexed", "bench.json"))
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "segmented_indexed", "stateless_ab.jsonl"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--keyed", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    from reservoir_amd import batch

    legs = a.legs.split(",")
    doc = {"tool": "tools/bench_segmented_indexed.py", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "streams": a.streams, "split_len_built_in": batch.SPLIT_LEN_DEFAULT, "legs": {}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    if "c3" in legs:
        runs = []
        for rnd in range(a.rounds):
            for split in (None, 0):
                r = run_child(a, "c3", split=split, keyed=(rnd == 0 and split is None))
                r["round"] = rnd
                runs.append(r)
        off = [r["result"]["keyless"] for r in runs if r["split_len_env"] == "0"]
        on = [r["result"]["keyless"] for r in runs if r["split_len_env"] is None]
        lo, hi = min(x["ms_min"] for x in off), max(x["ms_max"] for x in off)
        med_on = statistics.median(x["ms"] for x in on)
        doc["legs"]["c3"] = {"runs": runs, "split_off_spread_ms": [lo, hi], "split_on_median_ms": med_on,
                             "split_on_within_off_spread": bool(lo <= med_on <= hi) or med_on < lo}
        doc["device"] = runs[0]["device"]
        save()
    if "skew" in legs:
        runs = [run_child(a, "skew", split=split) for split in (1 << 18, 1 << 20, 1 << 22, 0)]
        best = {}
        for k in ("k64", "k1024"):
            t = {r["split_len_env"]: r["result"][k]["ms"] for r in runs}
            best[k] = {"ms_by_split_len": t, "fastest": min(t, key=t.get)}
        doc["legs"]["skew"] = {"runs": runs, "summary": best}
        save()
    for leg in ("k4096", "update", "merge", "objects"):
        if leg in legs:
            doc["legs"][leg] = run_child(a, leg)
            save()
    if a.ab_lib:
        os.makedirs(os.path.dirname(a.ab_out), exist_ok=True)
        with open(a.ab_out, "w") as f:
            for rnd in range(a.rounds + 1):
                for name, lib in (("parent", a.ab_lib), ("tree", None)):
                    r = run_child(a, "keyed", lib=lib)
                    f.write(json.dumps({"config": f"C3 keyed sample_segmented int64, {a.streams} x {C3_L}, k={C3_K}",
                                        "lib": name, "round": rnd, **r["result"]}) + "\n")
                    f.flush()
    print(json.dumps({k: (v.get("summary") or v.get("result") or {kk: vv for kk, vv in v.items() if kk != "runs"})
                      for k, v in doc["legs"].items()}, indent=1))


if __name__ == "__main__":
    main()
