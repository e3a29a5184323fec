"""Algorithm R's exact law as statistics with derived bounds (helper; no GPU, no oracle import).

The parity tests compare the kernels with the oracle, and both restate draw format R2 (DESIGN.md
section 2).  This module states what a fair sampler must do whatever its draw format, so that a slip
shared by the two restatements, or an unfairness of the format itself, has a test to fail.

The law.  One stream of n elements into k < n slots; W_j is the last writer of slot j.
  1. {W_j} is a uniformly random k-subset of [0, n): the member count of an index class of size c
     over T independent streams has mean T k c / n and a hypergeometric (sub-multinomial) covariance.
  2. For m >= k - 1, P(W_j <= m) = (m + 1) / n for every slot j: a slot bin x position bin table
     has equal cells when the position bin edges are multiples of n / B >= k.
  3. A fresh sampler after seek(i0), i0 >= k, then w draws: a slot stays unwritten with probability
     i0 / (i0 + w); the written slots are negatively associated (variance at most binomial), their
     writers uniform on the window, the slots themselves uniform over j.
  4. Two independent streams of the same n, k share a hypergeometric number of members, mean k^2 / n,
     variance at most the mean.
Nothing here is a measured tolerance: every bound follows from the law and alpha, and every test
file gives each of its N statistics alpha = 1e-6 / N.

The seed schedule and the families are fixed here so that nobody tunes them: a statistic that fails
on correct-looking code is a finding to explain.
"""
from __future__ import annotations

import math

import numpy as np

SUITE_ALPHA = 1e-6
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


# ---- critical values ----------------------------------------------------------------------------
def _gamma_pq(a: float, x: float):
    """(P(a, x), Q(a, x)), the regularised incomplete gammas; the smaller one is computed directly
    (series below x = a + 1, Lentz's continued fraction above), so small tails keep their digits."""
    if x <= 0.0:
        return 0.0, 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        ap = a
        for _ in range(100_000):
            ap += 1.0
            term *= x / ap
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        p = total * lead
        return p, 1.0 - p
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100_000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    q = lead * h
    return 1.0 - q, q


def chi2_sf(x: float, dof: int) -> float:
    return _gamma_pq(dof / 2.0, x / 2.0)[1]


def chi2_crit(dof: int, alpha: float) -> float:
    """x with P(chi2_dof > x) = alpha."""
    lo, hi = float(dof), float(dof) + 10.0
    while chi2_sf(hi, dof) > alpha:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if chi2_sf(mid, dof) > alpha:
            lo = mid
        else:
            hi = mid
        if hi - lo < 1e-12 * hi:
            break
    return 0.5 * (lo + hi)


def normal_two_sided(alpha: float) -> float:
    """z with P(|N(0, 1)| > z) = alpha."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > alpha:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def poisson_sf(c: int, mean: float) -> float:
    """P(Poisson(mean) >= c)."""
    return 1.0 if c <= 0 else _gamma_pq(float(c), mean)[0]


def poisson_upper(mean: float, alpha: float) -> int:
    """The smallest c with P(Poisson(mean) >= c) <= alpha: a count below c is accepted."""
    c = int(mean) + 1
    while poisson_sf(c, mean) > alpha:
        c += 1
    return c


def alpha_for(n_stats: int) -> float:
    return SUITE_ALPHA / n_stats


# ---- seed schedules -----------------------------------------------------------------------------
def run_ids(t: int):
    """(seed, stream_id) of run t of a family."""
    seed = t if t % 2 == 0 else (GOLDEN * (t + 1)) & M64
    return seed, (t * 0x100000001) & M64


ADJ_BASE = 0xD1B54A32D192ED03  # all four 32-bit words nonzero and distinct
ADJ_VARY = ("stream", "seed")
ADJ_STEP = ("inc", "inc32", "flip63")


def adjacent_runs(vary: str, step: str, T: int):
    """How callers derive ids (seed + s): one of seed / stream_id held at GOLDEN, the other at
    base + t (inc), base + (t << 32) (inc32), or base ^ (1 << 63) paired with base (flip63, over the
    bases ADJ_BASE + t // 2).  Returns ([(seed, stream_id)] * T, [(run a, run b)] pairs)."""
    if step == "inc":
        ids = [(ADJ_BASE + t) & M64 for t in range(T)]
    elif step == "inc32":
        ids = [(ADJ_BASE + (t << 32)) & M64 for t in range(T)]
    elif step == "flip63":
        ids = [((ADJ_BASE + t // 2) & M64) ^ ((t & 1) << 63) for t in range(T)]
    else:
        raise ValueError(step)
    pairs = [(t, t + 1) for t in range(0, T - 1, 2 if step == "flip63" else 1)]
    runs = [(GOLDEN, v) if vary == "stream" else (v, GOLDEN) for v in ids]
    return runs, pairs


def splitmix_keys(n: int) -> np.ndarray:
    """splitmix64 of 0 .. n-1 as int64: the distinct families' keys."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.view(np.int64)


# ---- the families -------------------------------------------------------------------------------
FROM_ZERO_TABLES = ("pos64", "mod16", "mod2", "lane64", "slot_x_pos8")
K_WIN = 1 << 20
WINDOWS = {  # name: (i0, w), tests/test_gpu_k1_forms.py's RANGES
    "fast_ghi1": (2**36 + 2**33 + 5, 1 << 23),
    "ends_at_2pow40": (2**40 - (1 << 26), 1 << 26),
    "starts_at_2pow40": (2**40, 1 << 26),
    "straddles_3x2pow33": (3 * 2**33 - (1 << 21) - 9, 1 << 22),
}
WINDOW_STATS = ("written", "pos16", "slot64")
D_KEYS, D_K = 1000, 100

# name: kind, shape, runs, statistics.  T is the number of independent streams behind a family; the
# totals behind pos64 are the smallest at which the 5 % position defect of the power test is
# rejected by every draw (tests/test_sampling_law_oracle.py), which is what set k1_past_2pow33's T
# and java_l's; k2_wave's is the smallest power of two at which its overlap total resolves 1.5 x its
# mean, and k1_sparse's the smallest multiple of 1024 at which slot_x_pos8 resolves a slot bin at 0.97
# of its share.
GPU_FAMILIES = {
    "k1_sparse": dict(kind="k1", k=1024, n=1 << 26, T=15360, stats=FROM_ZERO_TABLES),
    "k1_past_2pow33": dict(kind="k1", k=1024, n=2**33 + 2**21, T=512, stats=FROM_ZERO_TABLES),
    **{f"k1_adjacent_{v}_{s}": dict(kind="k1_adjacent", k=1024, n=1 << 26, T=512, vary=v, step=s, stats=("overlap",))
       for v in ADJ_VARY for s in ADJ_STEP},
    **{f"k1_window_{w}": dict(kind="k1_window", k=K_WIN, window=w, T=64, stats=WINDOW_STATS) for w in WINDOWS},
    "k2_wave": dict(kind="k2", k=4, n=4096, T=1 << 18, stats=("pos64", "mod16", "lane64", "slot_x_pos8", "overlap")),
    "k2_wg": dict(kind="k2", k=512, n=1 << 18, T=1024, stats=("pos64", "mod16", "lane64", "slot_x_pos8", "overlap")),
    "java_l": dict(kind="java_l", k=64, n=1 << 22, T=8192, stats=("pos64", "slot_x_pos8")),
    "distinct_identity": dict(kind="distinct", k=D_K, n=D_KEYS, T=16384, hash="identity", stats=("per_key", "overlap")),
    "distinct_default": dict(kind="distinct", k=D_K, n=D_KEYS, T=16384, hash="default", stats=("per_key", "overlap")),
}
# the oracle at reduced T (CPU suite): the same runs, fewer of them, plus K1 at n = 10^9
ORACLE_FAMILIES = {
    "k1_sparse": dict(GPU_FAMILIES["k1_sparse"], T=256),
    "k1_1e9": dict(kind="k1", k=1024, n=10**9, T=64, stats=FROM_ZERO_TABLES),
    **{f"k1_window_{w}": dict(GPU_FAMILIES[f"k1_window_{w}"], T=16) for w in WINDOWS},
    "java_l": dict(GPU_FAMILIES["java_l"], T=256),
    "distinct_identity": dict(GPU_FAMILIES["distinct_identity"], T=4000),
    "distinct_default": dict(GPU_FAMILIES["distinct_default"], T=4000),
}


def n_stats(families) -> int:
    return sum(len(f["stats"]) for f in families.values())


GPU_ALPHA = alpha_for(n_stats(GPU_FAMILIES))
ORACLE_ALPHA = alpha_for(n_stats(ORACLE_FAMILIES))


# ---- tables: integer counts, and the law's expectation of every cell ------------------------------
def _slot_bins(k: int) -> int:
    return min(32, k)


def _pos_bin_sizes(n: int, bins: int) -> np.ndarray:
    """Sizes of the classes (i * bins) // n over i in [0, n)."""
    edges = [-(-b * n // bins) for b in range(bins + 1)]
    return np.diff(np.array(edges, dtype=np.int64))


def _periodic_sizes(n: int, period: int, fn, classes: int) -> np.ndarray:
    one = np.bincount(fn(np.arange(period, dtype=np.int64)), minlength=classes).astype(np.int64)
    return one * (n // period) + np.bincount(fn(np.arange(n % period, dtype=np.int64)), minlength=classes)


_CLASS = {
    "mod16": (16, lambda i: i & 15, 16),
    "mod2": (2, lambda i: i & 1, 2),
    "lane64": (1024, lambda i: (i >> 4) & 63, 64),
}


def from_zero_tables(W: np.ndarray, n: int, k: int, names) -> dict:
    """Integer tables of the last writers W[..., k] (slot = last axis) of streams of n elements."""
    W = np.asarray(W, dtype=np.int64).reshape(-1, k)
    assert W.min() >= 0 and W.max() < n
    out = {}
    for name in names:
        if name == "pos64":
            out[name] = np.bincount((W * 64 // n).ravel(), minlength=64)
        elif name in _CLASS:
            _, fn, classes = _CLASS[name]
            out[name] = np.bincount(fn(W).ravel(), minlength=classes)
        elif name == "slot_x_pos8":
            sb = _slot_bins(k)
            cell = (np.arange(k, dtype=np.int64) * sb // k)[None, :] * 8 + W * 8 // n
            out[name] = np.bincount(cell.ravel(), minlength=sb * 8)
    return out


def from_zero_shares(name: str, n: int, k: int) -> np.ndarray:
    """The law's share of every cell of a from-zero table (sums to 1)."""
    if name == "pos64":
        return _pos_bin_sizes(n, 64) / n
    if name in _CLASS:
        period, fn, classes = _CLASS[name]
        return _periodic_sizes(n, period, fn, classes) / n
    if name == "slot_x_pos8":
        assert n % 8 == 0 and n // 8 >= k, "position bin edges must be multiples of n / 8 >= k (point 2)"
        sb = _slot_bins(k)
        slots = np.bincount(np.arange(k) * sb // k, minlength=sb) / k
        return np.outer(slots, np.full(8, 0.125)).ravel()
    raise KeyError(name)


def chi2_stat(obs, shares) -> float:
    obs = np.asarray(obs, dtype=np.float64)
    exp = obs.sum() * np.asarray(shares, dtype=np.float64)
    return float(((obs - exp) ** 2 / exp).sum())


def chi2_entry(name, obs, shares, alpha) -> dict:
    dof = len(shares) - 1
    v, b = chi2_stat(obs, shares), chi2_crit(dof, alpha)
    return dict(stat=name, test="chi2", dof=dof, value=v, bound=b, ok=bool(v < b))


def overlap_total(sets, pairs) -> int:
    """Members shared by the paired runs, summed (sets[r]: the members of run r, no repeats)."""
    sets = np.asarray(sets)
    a = np.array([p[0] for p in pairs])
    b = np.array([p[1] for p in pairs])
    if sets.shape[1] <= 16:
        return int((sets[a][:, :, None] == sets[b][:, None, :]).sum())
    return int(sum(np.intersect1d(sets[x], sets[y], assume_unique=True).size for x, y in zip(a, b)))


def overlap_entry(total: int, n_pairs: int, k: int, n: int, alpha: float) -> dict:
    """Point 4: mean n_pairs k^2 / n, variance at most the mean.  A two-sided normal bound from an
    expected total of 100, below it the Poisson upper tail."""
    mean = n_pairs * k * k / n
    if mean >= 100.0:
        z = normal_two_sided(alpha)
        dev = abs(total - mean) / math.sqrt(mean)
        return dict(stat="overlap", test="normal", mean=mean, value=dev, bound=z, total=int(total), ok=bool(dev < z))
    c = poisson_upper(mean, alpha)
    return dict(stat="overlap", test="poisson", mean=mean, value=int(total), bound=c, total=int(total), ok=bool(total < c))


def window_tables(slots, writers, i0: int, w: int, k: int) -> dict:
    """Point 3's tables of one window [i0, i0 + w): the written slots (export_state's idx >= 0) and
    their writers."""
    slots, writers = np.asarray(slots, dtype=np.int64), np.asarray(writers, dtype=np.int64)
    assert slots.shape == writers.shape and np.unique(slots).size == slots.size
    assert writers.min(initial=i0) >= i0 and writers.max(initial=i0) < i0 + w
    return dict(written=np.array([slots.size]),
                pos16=np.bincount((writers - i0) * 16 // w, minlength=16),
                slot64=np.bincount(slots * 64 // k, minlength=64))


def window_entries(tables: dict, i0: int, w: int, k: int, T: int, alpha: float) -> list:
    p = w / (i0 + w)
    mean, sd = T * k * p, math.sqrt(T * k * p * (1.0 - p))
    z = normal_two_sided(alpha)
    written = int(tables["written"][0])
    dev = abs(written - mean) / sd
    return [dict(stat="written", test="normal", mean=mean, value=dev, bound=z, total=written, ok=bool(dev < z)),
            chi2_entry("pos16", tables["pos16"], _pos_bin_sizes(w, 16) / w, alpha),
            chi2_entry("slot64", tables["slot64"], np.full(64, 1 / 64), alpha)]


def evaluate(fam: dict, tables: dict, alpha: float) -> list:
    """Every statistic of a family from its integer tables, with the bound the law and alpha give."""
    kind, k, T = fam["kind"], fam["k"], fam["T"]
    if kind == "k1_window":
        i0, w = WINDOWS[fam["window"]]
        return window_entries(tables, i0, w, k, T, alpha)
    out = []
    for name in fam["stats"]:
        if name == "overlap":
            out.append(overlap_entry(int(tables["overlap"][0]), int(tables["pairs"][0]), k, fam["n"], alpha))
        elif name == "per_key":
            out.append(chi2_entry(name, tables[name], np.full(fam["n"], 1.0 / fam["n"]), alpha))
        else:
            out.append(chi2_entry(name, tables[name], from_zero_shares(name, fam["n"], k), alpha))
    return out


# ---- defects for the power test -------------------------------------------------------------------
def defect_shares(name: str, n: int, k: int) -> np.ndarray:
    """The cell shares of a sampler with the defect that table `name` is there to catch."""
    p = from_zero_shares(name, n, k).copy()
    if name == "mod16":  # residue 15 never a member beyond 256 k
        p[15] *= min(1.0, 256 * k / n)
    elif name == "pos64":  # the second half of the positions 5 % over-weighted
        p[32:] *= 1.05
    elif name == "slot_x_pos8":  # one slot bin at 0.97 of its share
        p[:8] *= 0.97
    else:
        raise KeyError(name)
    return p / p.sum()


def noncentrality(total: int, shares, defect) -> float:
    """total * sum (q - p)^2 / p: what the defect adds to the chi-square's mean."""
    p, q = np.asarray(shares), np.asarray(defect)
    return float(total * ((q - p) ** 2 / p).sum())
