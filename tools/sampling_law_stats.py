"""Run the sampling-law families (tests/sampling_law.py) on the CPU oracle or on the GPU engine and
record every integer table and every statistic with its bound.

    python tools/sampling_law_stats.py --engine oracle --out profiles/sampling_law/oracle_stats.json
    python tools/sampling_law_stats.py --engine gpu    --out profiles/sampling_law/gpu_stats.json

The oracle record is the advance check that a correct implementation is inside every bound at the
final T and seeds; the engine and the oracle agree bit for bit, so the two files hold equal tables.
tests/test_gpu_sampling_law.py and tests/test_sampling_law_oracle.py run the same functions.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sampling_law as SL  # noqa: E402


def _signed(v: int) -> int:
    v &= SL.M64
    return v - (1 << 64) if v >> 63 else v


def _add(total: dict, part: dict) -> dict:
    for name, t in part.items():
        total[name] = total.get(name, 0) + np.asarray(t, dtype=np.int64)
    return total


def _key_index(keys: np.ndarray, sets: np.ndarray) -> np.ndarray:
    """The sampled keys as their positions in `keys` (every sampled key must be one of them)."""
    order = np.argsort(keys)
    pos = np.searchsorted(keys[order], sets)
    assert np.array_equal(keys[order][pos], sets)
    return order[pos]


def _distinct_tables(fam: dict, keys: np.ndarray, sets: np.ndarray) -> dict:
    idx = _key_index(keys, sets)
    pairs = [(s, s + 1) for s in range(fam["T"] - 1)]
    return dict(per_key=np.bincount(idx.ravel(), minlength=fam["n"]), pairs=np.array([len(pairs)]),
                overlap=np.array([SL.overlap_total(idx, pairs)]))


def _from_zero(fam: dict, W: np.ndarray, pairs=None) -> dict:
    names = [s for s in fam["stats"] if s != "overlap"]
    tables = SL.from_zero_tables(W, fam["n"], fam["k"], names)
    srt = np.sort(W, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "point 1: a k-subset holds no index twice"
    if pairs is not None:
        tables["pairs"] = np.array([len(pairs)])
        tables["overlap"] = np.array([SL.overlap_total(W, pairs)])
    return tables


# ---- the oracle ---------------------------------------------------------------------------------
def run_oracle(fam: dict) -> dict:
    from oracle import oracle as O

    kind, k, T = fam["kind"], fam["k"], fam["T"]
    if kind == "k1":
        return _from_zero(fam, np.stack([O.algo_r_last_writers(*SL.run_ids(t), k, 0, fam["n"]) for t in range(T)]))
    if kind == "k1_adjacent":
        runs, pairs = SL.adjacent_runs(fam["vary"], fam["step"], T)
        W = np.stack([O.algo_r_last_writers(seed, sid, k, 0, fam["n"]) for seed, sid in runs])
        return dict(_from_zero(fam, W, pairs))
    if kind == "k1_window":
        i0, w = SL.WINDOWS[fam["window"]]
        total = {}
        for t in range(T):
            idx = O.algo_r_last_writers(*SL.run_ids(t), k, i0, w)
            slots = np.flatnonzero(idx >= 0)
            _add(total, SL.window_tables(slots, idx[slots], i0, w, k))
        return total
    if kind == "k2":
        seed, base = SL.run_ids(0)
        W = np.stack([O.algo_r_last_writers(seed, base + s, k, 0, fam["n"], 1) for s in range(T)])
        return _from_zero(fam, W, [(s, s + 1) for s in range(T - 1)])
    if kind == "java_l":
        rows = []
        for t in range(T):
            a = O.AlgoL(k, _signed(SL.run_ids(t)[0]), event_cap=0)
            a.sample_all_iota(0, fam["n"])
            rows.append(a.result())
        return _from_zero(fam, np.stack(rows))
    if kind == "distinct":
        keys = SL.splitmix_keys(fam["n"])
        seed, base = SL.run_ids(0)
        hk = O.HASH_IDENTITY if fam["hash"] == "identity" else O.HASH_JAVA_LONG
        rows = []
        for s in range(T):
            d = O.Distinct(k, _signed(seed + base + s), hk)
            d.sample_all(keys)
            rows.append(d.result()[0])
        return _distinct_tables(fam, keys, np.stack(rows))
    raise KeyError(kind)


# ---- the GPU engine -----------------------------------------------------------------------------
_IOTA = {}


def device_iota(cuda):
    """arange(2^26) as int32 device keys, shared by the window families."""
    import torch

    if cuda not in _IOTA:
        _IOTA[cuda] = torch.arange(1 << 26, dtype=torch.int32, device=cuda)
    return _IOTA[cuda]


def _k1_members(Sampler, engine, k, n, seed, sid):
    s = Sampler(k, engine=engine, seed=seed, stream_id=sid)()
    s.sample_all(range(n))  # index-only: the members are the indices
    return s.result()


def run_gpu(fam: dict, cuda) -> dict:
    import torch

    from reservoir_amd import Sampler, batch

    kind, k, T = fam["kind"], fam["k"], fam["T"]
    if kind == "k1":
        return _from_zero(fam, np.stack([_k1_members(Sampler, "philox_r", k, fam["n"], *SL.run_ids(t)) for t in range(T)]))
    if kind == "k1_adjacent":
        runs, pairs = SL.adjacent_runs(fam["vary"], fam["step"], T)
        W = np.stack([_k1_members(Sampler, "philox_r", k, fam["n"], seed, sid) for seed, sid in runs])
        return _from_zero(fam, W, pairs)
    if kind == "k1_window":
        i0, w = SL.WINDOWS[fam["window"]]
        iota = device_iota(cuda)
        total = {}
        for t in range(T):
            seed, sid = SL.run_ids(t)
            s = Sampler(k, seed=seed, stream_id=sid, key_type="int")()
            s.seek(i0)
            s.sample_all(iota[:w])
            idx, keys, _, _ = s.export_state(cuda)
            torch.cuda.synchronize()
            slots = torch.nonzero(idx >= 0).flatten()
            writers = idx[slots].cpu().numpy()
            # the slot's key is its writer's offset in the window
            assert np.array_equal(keys[slots].cpu().numpy().astype(np.int64), writers - i0)
            _add(total, SL.window_tables(slots.cpu().numpy(), writers, i0, w, k))
            s.close()
        return total
    if kind == "k2":
        seed, base = SL.run_ids(0)
        n = fam["n"]
        keys = torch.arange(n, dtype=torch.int32, device=cuda).repeat(T)  # key = position in its stream
        offs = torch.arange(0, T * n + 1, n, dtype=torch.int64, device=cuda)
        out, cnt = batch.sample_segmented(keys, offs, k, seed=seed, stream_base=base)
        assert int(cnt.min()) == k
        W = out.cpu().numpy().astype(np.int64)
        del keys, out
        torch.cuda.empty_cache()
        return _from_zero(fam, W, [(s, s + 1) for s in range(T - 1)])
    if kind == "java_l":
        return _from_zero(fam, np.stack([_k1_members(Sampler, "java_l", k, fam["n"], SL.run_ids(t)[0], 0) for t in range(T)]))
    if kind == "distinct":
        keys = SL.splitmix_keys(fam["n"])
        seed, base = SL.run_ids(0)
        kd = torch.from_numpy(keys).to(cuda).repeat(T)
        offs = torch.arange(0, T * fam["n"] + 1, fam["n"], dtype=torch.int64, device=cuda)
        kw = {} if fam["hash"] == "default" else {"hash": fam["hash"]}
        dk, _, dc = batch.distinct_segmented(kd, offs, k, seed=seed, stream_base=base, **kw)
        assert int(dc.min()) == k
        return _distinct_tables(fam, keys, dk.cpu().numpy())
    raise KeyError(kind)


def run_family(fam: dict, engine: str, cuda=None) -> dict:
    return run_oracle(fam) if engine == "oracle" else run_gpu(fam, cuda)


def record(families: dict, engine: str, alpha: float, cuda=None, only=None, log=None) -> dict:
    out = {"engine": engine, "alpha": alpha, "n_stats": SL.n_stats(families), "families": {}}
    for name, fam in families.items():
        if only and name not in only:
            continue
        t0 = time.time()
        tables = run_family(fam, engine, cuda)
        stats = SL.evaluate(fam, tables, alpha)
        out["families"][name] = {"T": fam["T"], "seconds": round(time.time() - t0, 2),
                                 "stats": stats, "tables": {n: np.asarray(t).tolist() for n, t in tables.items()}}
        if log:
            log(f"{name}: {time.time() - t0:.1f} s  " + "  ".join(
                f"{e['stat']}={e['value']:.4g}/{e['bound']:.4g}{'' if e['ok'] else ' FAIL'}" for e in stats))
    return out


def write_record(rec: dict, path: str) -> None:
    """JSON with every integer table on one line."""
    text = json.dumps(rec, indent=1)
    text = re.sub(r"\[\s+([-\d,\s]+?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--engine", choices=("oracle", "gpu"), default="oracle")
    ap.add_argument("--out", required=True)
    ap.add_argument("--family", action="append", help="only these families (default: all)")
    ap.add_argument("--merge", action="store_true", help="keep the families already recorded in --out")
    a = ap.parse_args()
    cuda = None
    if a.engine == "gpu":
        import torch

        torch.cuda.set_device(0)
        cuda = torch.device("cuda", 0)
    rec = record(SL.GPU_FAMILIES, a.engine, SL.GPU_ALPHA, cuda, a.family, lambda m: print(m, flush=True))
    if a.merge and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        old["families"].update(rec["families"])
        rec["families"] = {n: old["families"][n] for n in SL.GPU_FAMILIES if n in old["families"]}
    write_record(rec, a.out)
    bad = [(n, e["stat"]) for n, r in rec["families"].items() for e in r["stats"] if not e["ok"]]
    print("outside their bounds:", bad if bad else "none")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
