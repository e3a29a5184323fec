"""Sampler.distinct for any B, hashes only: C4's per-GPU share (5e8 device-resident int64 hashes,
30 % duplicates, k = 65536, a fresh sampler per step) through rsv_distinct_candidates.

Reports, per step and as medians: the obj_filter kernel time (rsv_profile_read: HIP events around
every obj_filter launch of the batch's chunk loop), the bytes it moved over that time, n_cand, and
the end-to-end time from rsv_distinct_candidates to the return of rsv_candidates_read (host clock;
both calls return with their device work done).

Comparator, same process, alternating with it: the byte-key set-mode leg with a precomputed hash
(Sampler.distinct over "bytes16" rows, order="set": wide_filter_hashes over the same n hashes, then
the gather and merge of its candidates), kernel time through the same rsv_profile_read bracket and
end to end through result().

    python tools/bench_object_distinct.py [--n 500000000] [--k 65536] [--steps 5] [--warmup 1] [--out FILE]
prints one JSON line (and writes it to --out).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-comparator", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import workloads as W

    from reservoir_amd import Sampler
    from reservoir_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("bench_object_distinct needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = N.load()
    vals = W.c4_data(a.n, dev)
    hs = W.smix(vals ^ 0x5A5A)
    rows = None if a.no_comparator else W.uuid_rows(vals)
    del vals
    torch.cuda.synchronize()
    offs = np.empty(1, dtype=np.int64)
    ch = np.empty(1, dtype=np.int64)

    def profile(h):
        ms, launches = C.c_double(), C.c_int64()
        N.check(L.rsv_profile_read(h, C.byref(ms), C.byref(launches)))
        return ms.value, launches.value

    def object_step():
        nonlocal offs, ch
        cfg = N.RsvConfig()
        N.check(L.rsv_config_init(C.byref(cfg)))
        cfg.kind, cfg.max_sample_size, cfg.hash_kind, cfg.seed = N.KIND_DISTINCT, a.k, N.HASH_PRECOMPUTED, 7
        h = C.c_void_p()
        N.check(L.rsv_create(C.byref(cfg), C.byref(h)))
        N.check(L.rsv_profile_enable(h, 1))
        nc = C.c_int64()
        t0 = time.perf_counter()
        N.check(L.rsv_distinct_candidates(h, C.c_void_p(hs.data_ptr()), a.n, N.MEM_DEVICE, C.byref(nc)))
        if nc.value > offs.size:
            offs = np.empty(nc.value, dtype=np.int64)
            ch = np.empty(nc.value, dtype=np.int64)
        N.check(L.rsv_candidates_read(h, offs.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.c_void_p), offs.size))
        e2e = (time.perf_counter() - t0) * 1e3
        N.check(L.rsv_candidates_abort(h))
        ms, launches = profile(h)
        L.rsv_destroy(h)
        return {"filter_ms": ms, "filter_launches": launches, "n_cand": nc.value, "e2e_ms": e2e}

    def single_launch_step():
        """a sampler that has seen the first quarter takes the rest as ONE chunk: one obj_filter launch
        over 3/4 of the hashes, the rate the chunked batch is compared with"""
        cfg = N.RsvConfig()
        N.check(L.rsv_config_init(C.byref(cfg)))
        cfg.kind, cfg.max_sample_size, cfg.hash_kind, cfg.seed = N.KIND_DISTINCT, a.k, N.HASH_PRECOMPUTED, 7
        h = C.c_void_p()
        N.check(L.rsv_create(C.byref(cfg), C.byref(h)))
        N.check(L.rsv_profile_enable(h, 1))
        nc = C.c_int64()
        q = a.n // 4
        N.check(L.rsv_distinct_candidates(h, C.c_void_p(hs.data_ptr()), q, N.MEM_DEVICE, C.byref(nc)))
        N.check(L.rsv_candidates_commit(h, 0, 0))
        ms0, l0 = profile(h)
        N.check(L.rsv_distinct_candidates(h, C.c_void_p(hs.data_ptr() + 8 * q), a.n - q, N.MEM_DEVICE, C.byref(nc)))
        N.check(L.rsv_candidates_abort(h))
        ms1, l1 = profile(h)
        L.rsv_destroy(h)
        return {"filter_ms": ms1 - ms0, "filter_launches": l1 - l0, "elements": a.n - q, "n_cand": nc.value}

    def wide_step():
        d = Sampler.distinct(a.k, key_type="bytes16", seed=7, order="set")(hash=lambda b: 0)
        N.check(L.rsv_profile_enable(d.handle, 1))
        t0 = time.perf_counter()
        d.sample_all(rows, hashes=hs)
        d.synchronize()
        e2e = (time.perf_counter() - t0) * 1e3
        ms, launches = profile(d.handle)
        d.close()
        return {"filter_ms": ms, "filter_launches": launches, "e2e_ms": e2e}

    obj, wide, single = [], [], []
    for step in range(a.warmup + a.steps):
        o = object_step()
        sl = single_launch_step()
        if step >= a.warmup:
            single.append(sl)
        w = None if a.no_comparator else wide_step()
        if step >= a.warmup:
            obj.append(o)
            if w:
                wide.append(w)

    def med(rs, f):
        return statistics.median(r[f] for r in rs)

    gbytes = a.n * 8 / 1e9
    out = {"bench": "object_distinct", "n": a.n, "k": a.k, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "obj_filter_ms": med(obj, "filter_ms"), "obj_filter_launches": obj[0]["filter_launches"],
           "obj_filter_GBps": gbytes / (med(obj, "filter_ms") / 1e3),
           "n_cand": obj[0]["n_cand"], "obj_e2e_ms": med(obj, "e2e_ms"), "obj_steps": obj}
    out.update({"single_launch_ms": med(single, "filter_ms"), "single_launch_launches": single[0]["filter_launches"],
                "single_launch_elements": single[0]["elements"],
                "single_launch_GBps": single[0]["elements"] * 8 / 1e9 / (med(single, "filter_ms") / 1e3)})
    if wide:
        out.update({"wide_filter_ms": med(wide, "filter_ms"), "wide_filter_launches": wide[0]["filter_launches"],
                    "wide_filter_GBps": gbytes / (med(wide, "filter_ms") / 1e3),
                    "wide_e2e_ms": med(wide, "e2e_ms"), "wide_steps": wide,
                    "filter_ratio": med(obj, "filter_ms") / med(wide, "filter_ms")})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
