"""Every distinct kernel at exact scrambled-hash values, with planted keys (tests/hash_targets.py).

The scrambled hash of a random key is uniform on int64, so random streams never meet the code that
only matters at particular values: Long.MinValue / Long.MaxValue as "no bound" and as sort padding,
the strict `h < maxHash`, a bucket of exactly 64 / 128 / 256 entries, a bucket spanning exactly 2^58.
`unscramble` inverts the scramble, so a Long key under the identity hash (the key is the preimage), or
any key with a precomputed hash (the hash is the preimage; ties on purpose), lands exactly there.

Every case is bit-exact against oracle.Distinct / oracle.DistinctRows, or numpy's lexsort((key, h))[:k]
over the distinct keys where set mode with ties is meant, and asserts on the reference side -- before
the GPU is touched -- that the planted elements are where the case needs them.

Groups: A range ends; B dense low cluster (direct bucket branch, hbits-limited radix merge); C bucket
occupancy and the packed sort; D the admission bound; E segmented distinct (K5); F object distinct;
G byte keys; H the packed-row combine.
"""
import numpy as np
import pytest
from hash_targets import MAX, MIN, bucket_log, bucket_nobound, direct_branch, plant, r01, unscramble
from segdistinct_ref import _expected, _scramble
from segdistinct_ref import _r01 as _seg_r01

import test_gpu_object_distinct as OD  # the raw candidate protocol (Handle, _run) and the byte rows of an id

pytestmark = pytest.mark.gpu

ORDERS = ["set", "ordered"]
BUCKET_CAP = 256  # rsv_distinct.hip kBucketCap


# ---- reference side ---------------------------------------------------------------------------------
def _scr(r0, r1, hashed):
    """Scrambled hashes of an int64 array of hash values under one (r0, r1)."""
    hashed = np.asarray(hashed, dtype=np.int64)
    return _scramble(np.full(hashed.shape, r0, dtype=np.int64), np.full(hashed.shape, r1, dtype=np.int64), hashed)


def _rand(rng, n):
    return rng.integers(MIN, MAX, size=n, dtype=np.int64)


def _all_distinct(*arrays):
    a = np.concatenate([np.asarray(x, dtype=np.int64).ravel() for x in arrays])
    assert np.unique(a).size == a.size, "a planted key repeats another key"


def _cand_limit(k):  # rsv_distinct.hip: the most candidates one filter pass may keep
    return 4 * k + 4096


def _log_bmax(k):  # rsv_distinct.hip: buckets for the largest merge (k + cand_limit entries)
    return bucket_log(k + _cand_limit(k))


def _wants(oracle, k, seed, batches):
    """oracle.Distinct (identity hash) fed the batches: [(keys, hashes) after each batch]."""
    ref = oracle.Distinct(k, seed, oracle.HASH_IDENTITY)
    out = []
    for b in batches:
        ref.sample_all(b)
        rk, rh = ref.result()
        out.append((rk.tolist(), rh.tolist()))
    return out


class _KeyOracle:
    """RandomValues over Int / Long keys with precomputed hashes: oracle.DistinctRows over the 16-byte
    rows [key | ~key] (equality by key, so several keys may share a hash)."""

    def __init__(self, oracle, k, seed):
        self.ref = oracle.DistinctRows(k, seed, 16)

    def feed(self, keys, hashes):
        keys = np.asarray(keys, dtype=np.int64)
        self.ref.sample_all(np.stack([keys, ~keys], axis=1).view(np.uint8), np.asarray(hashes, dtype=np.int64))
        return self.result()

    def result(self):
        rows, hs = self.ref.result()
        return np.ascontiguousarray(rows).view(np.int64).reshape(-1, 2)[:, 0].tolist(), hs.tolist()


def _bottomk(keys, h, k):
    """Set mode: the k smallest (h, key) over the distinct keys."""
    keys, first = np.unique(np.asarray(keys, dtype=np.int64), return_index=True)
    h = np.asarray(h, dtype=np.int64)[first]
    o = np.lexsort((keys, h))[:k]
    return keys[o].tolist(), h[o].tolist()


# ---- GPU side ---------------------------------------------------------------------------------------
def _dev(cuda, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _identity_run(cuda, k, seed, order, batches, wants):
    """A reusable identity-hash sampler read after every batch: the oracle's keys, in its order."""
    from reservoir_amd import Sampler

    d = Sampler.distinct(k, seed=seed, order=order, reusable=True)(hash="identity")
    seen = 0
    for i, (b, (wk, _)) in enumerate(zip(batches, wants)):
        d.sample_all(_dev(cuda, b))
        seen += b.size
        assert d.result().tolist() == wk, (order, i)
        assert d.count == seen
    return d


def _hashed_sampler(k, seed, order, key_type="long"):
    from reservoir_amd import Sampler

    return Sampler.distinct(k, seed=seed, order=order, key_type=key_type, reusable=True)(hash=lambda x: 0)


def _feed_hashed(cuda, d, keys, hashes, key_type="long"):
    dt = np.int32 if key_type == "int" else np.int64
    d.sample_all(_dev(cuda, np.asarray(keys).astype(dt)), hashes=_dev(cuda, np.asarray(hashes, dtype=np.int64)))


# ---- A. range ends, single stream -------------------------------------------------------------------
@pytest.mark.parametrize("arrange", ["first", "last", "alone"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", [1, 5, 64, 700])
def test_range_ends(cuda, oracle, k, order, arrange):
    """Keys at Long.MinValue, MinValue + 1, MaxValue - 1, MaxValue (each twice) around 3000 random keys."""
    seed = 17
    r0, r1 = r01(oracle, seed)
    targets = [MIN, MIN + 1, MAX - 1, MAX]
    planted = plant(r0, r1, targets)
    rand = _rand(np.random.default_rng(k), 3000)
    _all_distinct(rand, planted)
    twice = np.concatenate([planted, planted])
    if arrange == "first":
        batches = [np.concatenate([twice, rand])]
    elif arrange == "last":
        batches = [np.concatenate([rand, twice])]
    else:
        batches = [twice[i:i + 1] for i in range(8)] + [rand]
    wants = _wants(oracle, k, seed, batches)
    fk, fh = wants[-1]
    assert fh[:min(k, 2)] == targets[:min(k, 2)] and fk[:min(k, 2)] == planted[:min(k, 2)].tolist()
    assert len(fh) == k and MAX not in fh and MAX - 1 not in fh  # kept at the bottom, dropped at the top
    if arrange == "alone":  # before the random keys arrive the planted ones are the whole set
        assert wants[7][1] == sorted(targets)[:k]
        assert [w[1] for w in wants[:2]] == [[MIN], [MIN, MIN + 1][:k]]
    _identity_run(cuda, k, seed, order, batches, wants)


@pytest.mark.parametrize("order", ORDERS)
def test_not_full_with_top_at_max(cuda, oracle, order):
    """k = 64: 20 keys with h = Long.MaxValue among them (set_top = MaxValue while m < k), 30 more,
    then 5000 that cross k."""
    k, seed = 64, -5
    r0, r1 = r01(oracle, seed)
    top = plant(r0, r1, [MAX])
    rand = _rand(np.random.default_rng(2), 5049)
    _all_distinct(rand, top)
    batches = [np.concatenate([rand[:7], top, rand[7:19]]), rand[19:49], rand[49:]]
    assert [b.size for b in batches] == [20, 30, 5000]
    wants = _wants(oracle, k, seed, batches)
    assert len(wants[0][1]) == 20 and wants[0][1][-1] == MAX
    assert len(wants[1][1]) == 50 and wants[1][1][-1] == MAX
    assert len(wants[2][1]) == k and wants[2][1][-1] < MAX
    _identity_run(cuda, k, seed, order, batches, wants)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n2", [3000, 20_000])
def test_full_with_max_hash_at_max(cuda, oracle, order, n2):
    """k = 8, exactly 8 distinct keys with h = Long.MaxValue among them: the set is full and its bound
    is the "no bound" value.  3000 more keys fit the candidate buffer (set mode: the no-bound route
    with a full set); 20 000 do not (the threshold is tightened starting from Long.MaxValue)."""
    k, seed = 8, 17
    assert 3000 <= _cand_limit(k) < 20_000
    r0, r1 = r01(oracle, seed)
    top = plant(r0, r1, [MAX])
    rand = _rand(np.random.default_rng(n2), 7 + n2)
    _all_distinct(rand, top)
    batches = [np.concatenate([rand[:3], top, rand[3:7]]), rand[7:]]
    wants = _wants(oracle, k, seed, batches)
    assert len(wants[0][1]) == k and wants[0][1][-1] == MAX
    assert wants[1][1][-1] < MAX
    _identity_run(cuda, k, seed, order, batches, wants)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("repeats", [150, 300])
def test_full_with_max_hash_at_min(cuda, oracle, order, repeats):
    """k = 1 holding h = Long.MinValue: nothing is below it.  Set mode's candidates are the repeats of
    the member alone, merged over a span of 0, where q = 2^64 - 1 takes the direct bucket branch for
    every lb >= 1: 150 repeats -> 151 entries, lb = 1, one bucket below its capacity (merged on the
    device); 300 repeats -> 301 entries, lb = 2, all in bucket 0, which overflows, so the set is merged
    by the radix sort over span_bits(MinValue) = 1 bit.  Ordered mode leaves the chunk loop at once and
    still counts what it skipped."""
    k, seed = 1, 17
    r0, r1 = r01(oracle, seed)
    low = plant(r0, r1, [MIN])
    rng = np.random.default_rng(4)
    rand = _rand(rng, 5010)
    _all_distinct(rand, low)
    b2 = np.concatenate([rand[10:], np.repeat(low, repeats)])
    rng.shuffle(b2)
    batches = [np.concatenate([rand[:6], low, rand[6:10]]), b2]
    wants = _wants(oracle, k, seed, batches)
    assert wants[0] == wants[1] == (low.tolist(), [MIN])
    raw = k + int((_scr(r0, r1, b2) <= MIN).sum())  # the member and the candidates: all in bucket u = 0
    lb = bucket_log(raw, _log_bmax(k))
    assert raw == 1 + repeats <= _cand_limit(k) and direct_branch(MIN, lb)
    assert (lb, raw > BUCKET_CAP) == ((1, False) if repeats == 150 else (2, True))
    _identity_run(cuda, k, seed, order, batches, wants)


def test_ordered_heap_tied_at_min(cuda, oracle):
    """Precomputed hashes, k = 3: three distinct keys all hashed to Long.MinValue fill the heap; a
    fourth key at MinValue among 2000 more is not below the maximum.  The first three stay."""
    k, seed = 3, 17
    r0, r1 = r01(oracle, seed)
    pre = unscramble(r0, r1, MIN)
    rng = np.random.default_rng(6)
    more = _rand(rng, 2000)
    more_h = _rand(rng, 2000)
    first, fourth = np.array([101, 102, 103], dtype=np.int64), 104
    _all_distinct(more, first, [fourth])
    more[777], more_h[777] = fourth, pre
    batches = [(first, np.full(3, pre, dtype=np.int64)), (more, more_h)]
    ref = _KeyOracle(oracle, k, seed)
    wants = [ref.feed(*b) for b in batches]
    assert sorted(wants[0][0]) == sorted(wants[1][0]) == [101, 102, 103] and wants[1][1] == [MIN] * 3
    d = _hashed_sampler(k, seed, "ordered")
    for b, w in zip(batches, wants):
        _feed_hashed(cuda, d, *b)
        assert sorted(d.result().tolist()) == sorted(w[0])


# ---- B. dense low cluster ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_dense_low_cluster_direct_branch(cuda, oracle, order):
    """k = 20 over the 40 hashes MinValue + j.  Batch 1 (odd j + 200 random keys) fills the set:
    max_h = MinValue + 39.  Batch 2 brings the even j and 105 repeats of every j < 39 among 3000 random
    keys: only planted keys pass the bound, so the merge holds m = 20 members + c = 20 + 39 * 105 = 4115
    candidates = 4135 entries -> lb = bucket_log(4135) = 6, and with span + 1 = 40 the map's
    q = floor((2^64 - 1) / 40) has q >> (64 - 6) = 1: the direct branch b = u (lb = 5 would give
    q >> 59 = 0, the multiply).  Batch 3 sends 300 repeats of the key at MinValue (with 5 repeats of
    every planted key): about 400 candidates + 20 members -> lb = 2, span + 1 = 20, the multiply: the
    first of the 4 buckets takes at least u < 5, more than 256 entries, overflows, and the set is merged
    by the radix sort over span_bits(MinValue + 19) = 5 bits."""
    k, seed = 20, 23
    r0, r1 = r01(oracle, seed)
    low = plant(r0, r1, [MIN + j for j in range(40)])
    odd, even = low[1::2], low[0::2]
    rng = np.random.default_rng(8)
    ra, rb = _rand(rng, 200), _rand(rng, 3000)
    _all_distinct(low, ra, rb)
    assert _scr(r0, r1, np.concatenate([ra, rb])).min() > MIN + 39  # no random key passes a bound
    b1 = np.concatenate([odd, ra])
    b2 = np.concatenate([even, np.tile(low[:39], 105), rb])
    b3 = np.concatenate([np.repeat(low[:1], 300), np.tile(low, 5)])
    for b in (b1, b2, b3):
        rng.shuffle(b)
    batches = [b1, b2, b3]
    wants = _wants(oracle, k, seed, batches)
    assert wants[0][1] == [MIN + j for j in range(1, 40, 2)]
    assert wants[1][1] == wants[2][1] == [MIN + j for j in range(20)]
    # batch 2: the same candidates under the inclusive set bound (MinValue + 39) and the ordered one (+ 38)
    c2 = int((_scr(r0, r1, b2) <= MIN + 38).sum())
    assert c2 == int((_scr(r0, r1, b2) <= MIN + 39).sum()) == 4115 <= _cand_limit(k)
    lb2 = bucket_log(k + c2, _log_bmax(k))
    assert lb2 == 6 and direct_branch(MIN + 39, lb2) and not direct_branch(MIN + 39, lb2 - 1)
    # batch 3: bucket 0 of floor(u * 4 / 20) takes u < 5 and overflows
    h3 = _scr(r0, r1, b3)
    for c3 in (int((h3 <= MIN + 18).sum()), int((h3 <= MIN + 19).sum())):  # ordered / set bound
        lb3 = bucket_log(k + c3, _log_bmax(k))
        assert lb3 == 2 and not direct_branch(MIN + 19, lb3) and c3 <= _cand_limit(k)
    assert int((h3 < MIN + 5).sum()) > BUCKET_CAP
    _identity_run(cuda, k, seed, order, batches, wants)


@pytest.mark.parametrize("order", ORDERS)
def test_low_cluster_overflows_a_nobound_bucket(cuda, oracle, order):
    """k = 2000, one batch of 3000 keys, 300 of them at MinValue + j: without a bound (lb = 5) they share
    bucket 0, entry 257 raises the overflow word, and the radix merge runs on the injective path."""
    k, seed = 2000, 23
    r0, r1 = r01(oracle, seed)
    low = plant(r0, r1, [MIN + j for j in range(300)])
    rng = np.random.default_rng(9)
    rand = _rand(rng, 2700)
    _all_distinct(low, rand)
    batch = np.concatenate([low, rand])
    rng.shuffle(batch)
    assert batch.size <= _cand_limit(k) // 2  # no threshold estimate: every key is a candidate
    lb = bucket_log(batch.size, _log_bmax(k))
    assert lb == 5 and np.bincount(bucket_nobound(_scr(r0, r1, batch), lb))[0] > BUCKET_CAP
    wants = _wants(oracle, k, seed, [batch])
    assert wants[0][1][:300] == [MIN + j for j in range(300)] and len(wants[0][1]) == k
    _identity_run(cuda, k, seed, order, [batch], wants)


# ---- C. bucket occupancy and the packed sort, no-bound merges ---------------------------------------
def _bucket_hashes(rng, lb, b, n):
    """n distinct hashes of bucket b of 2^lb (no-bound map), its first and last value among them."""
    assert 1 <= lb <= 2 and n >= 2
    lo, size = b << (64 - lb), 1 << (64 - lb)
    us = {lo, lo + size - 1}
    while len(us) < n:
        us.add(lo + int(rng.integers(0, 2**62)))
    return [u - 2**63 for u in us]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("total,counts,dups", [(200, [64, 136], 0), (200, [65, 135], 0), (200, [128, 72], 0),
                                               (260, [129, 44, 44, 43], 0), (300, [255, 15, 15, 15], 0),
                                               (300, [256, 15, 15, 14], 0), (300, [257, 15, 14, 14], 0),
                                               (300, [256, 15, 15, 14], 20)],
                         ids=["64", "65", "128_72", "129", "255", "256", "257", "256_with_20_dups"])
def test_bucket_occupancy(cuda, oracle, order, total, counts, dups):
    """A fresh sampler with k above the batch: no bound (q = 1), bucket = u >> (64 - lb).  total = 200 ->
    lb = 1; 260 and 300 -> lb = 2.  The named bucket holds exactly 64 / 65 (R = 1 / 2 registers per lane),
    128 / 129 (R = 2 / 4), 255 / 256 / 257 entries (257: the overflow path); counts are RAW entries --
    the last case has 236 distinct keys and 20 repeats in the 256-entry bucket."""
    k, seed = 1000, 31
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(total + counts[0] + dups)
    lb = bucket_log(total, _log_bmax(k))
    assert lb == len(counts).bit_length() - 1 and sum(counts) == total <= _cand_limit(k) // 2
    hs = []
    for b, n in enumerate(counts):
        own = _bucket_hashes(rng, lb, b, n - (dups if b == 0 else 0))
        hs += own + (own[:dups] if b == 0 else [])
    batch = plant(r0, r1, hs)
    assert np.unique(batch).size == total - dups
    rng.shuffle(batch)
    assert np.bincount(bucket_nobound(_scr(r0, r1, batch), lb), minlength=1 << lb).tolist() == counts
    wants = _wants(oracle, k, seed, [batch])
    assert wants[0][1] == sorted(set(hs))
    _identity_run(cuda, k, seed, order, [batch], wants)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("anchor", ["min", "max"])
@pytest.mark.parametrize("total,D", [(40, 2**58 - 1), (40, 2**58), (40, 2**58 + 1), (64, 2**58 - 1)],
                         ids=["40_below", "40_at", "40_above", "64_below"])
def test_packed_sort_span_boundary(cuda, oracle, order, anchor, total, D):
    """One bucket (lb = 0) of <= 64 entries is sorted on (u - lo) << 6 | lane when its hashes span less
    than 2^58.  Smallest hash h0, largest h0 + D for D = 2^58 - 1 (packed), 2^58 and 2^58 + 1 (the full
    network), anchored at Long.MinValue and at Long.MaxValue; 64 entries leave no pad lane."""
    k, seed = 1000, 37
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(total + D % 7)
    h0 = MIN if anchor == "min" else MAX - D
    offs = {0, D}
    while len(offs) < total:
        offs.add(int(rng.integers(1, D)))
    hs = [h0 + o for o in offs]
    assert min(hs) == (MIN if anchor == "min" else MAX - D) and max(hs) - min(hs) == D and max(hs) <= MAX
    batch = plant(r0, r1, hs)
    rng.shuffle(batch)
    sh = _scr(r0, r1, batch)
    assert bucket_log(total, _log_bmax(k)) == 0 and total <= 64
    assert int(sh.max()) - int(sh.min()) == D and ((D >> 58) == 0) == (D == 2**58 - 1)
    wants = _wants(oracle, k, seed, [batch])
    assert wants[0][1] == sorted(hs)
    _identity_run(cuda, k, seed, order, [batch], wants)


@pytest.mark.parametrize("k", [1000, 39])
@pytest.mark.parametrize("key_type", ["int", "long"])
def test_pad_collision(cuda, oracle, key_type, k):
    """The bucket sort pads with (Long.MaxValue, the key type's maximum); here a real entry equals the
    pad (sent twice) next to (MaxValue, 5).  40 distinct keys, 41 raw entries, one bucket.  Set mode keeps
    the bottom-k by (h, key): both while not full, and with k = 39 the larger key drops."""
    seed = 41
    r0, r1 = r01(oracle, seed)
    big = 2**31 - 1 if key_type == "int" else MAX
    pre = unscramble(r0, r1, MAX)
    rng = np.random.default_rng(k)
    keys = np.concatenate([np.arange(1000, 1038, dtype=np.int64) * 7919, [big, 5, big]])
    hashes = np.concatenate([_rand(rng, 38), [pre, pre, pre]])
    assert np.unique(keys).size == 40 and keys.size == 41 and bucket_log(41, _log_bmax(k)) == 0
    sh = _scr(r0, r1, hashes)
    assert sh[-3:].tolist() == [MAX] * 3 and sh[:-3].max() < MAX
    wk, wh = _bottomk(keys, sh, k)
    if k == 39:
        assert wk[-1] == 5 and wh[-1] == MAX and big not in wk and len(wk) == 39
    else:
        assert wk[-2:] == [5, big] and wh[-2:] == [MAX, MAX] and len(wk) == 40
    p = rng.permutation(keys.size)
    d = _hashed_sampler(k, seed, "set", key_type)
    _feed_hashed(cuda, d, keys[p], hashes[p], key_type)
    assert d.result().astype(np.int64).tolist() == wk


# ---- D. the admission bound -------------------------------------------------------------------------
def _bound_case(oracle, key_type, seed, k=64):
    """5000 prefix keys with random precomputed hashes, M = the oracle's maximum after them, three fresh
    keys, and 1000 further keys whose scrambled hashes all lie above M."""
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(seed)
    keys = (rng.permutation(400_000)[:6500] - 200_000).astype(np.int64)
    if key_type == "long":
        keys = keys * 0x10000000001 + 3
    hv = _rand(rng, keys.size)
    assert np.unique(hv).size == hv.size
    pre = (keys[:5000], hv[:5000])
    ref = _KeyOracle(oracle, k, seed)
    wk, wh = ref.feed(*pre)
    M = max(wh)
    assert len(wh) == k and MIN + 1 < M < MAX - 1 and wh.count(M) == 1
    above = _scr(r0, r1, hv[5003:]) > M + 1
    more = (keys[5003:][above][:1000], hv[5003:][above][:1000])
    assert more[0].size == 1000
    return r0, r1, ref, pre, (wk, wh), M, keys[5000:5003], more


@pytest.mark.parametrize("same_batch", [False, True], ids=["next_batch", "same_batch"])
@pytest.mark.parametrize("key_type", ["long", "int"])
def test_ordered_admission_bound(cuda, oracle, key_type, same_batch):
    """Ordered mode admits h < maxHash only.  With the heap's maximum at M, fresh keys arrive at M (it
    meets maxHash == M: rejected), M + 1 (rejected) and M - 1 (admitted; nothing later is below it, so
    it stays as the new maximum) -- in the batch after the prefix (the filter bound is M - 1), and inside
    the prefix's own batch (the chunk loop and the host replay decide)."""
    k, seed = 64, 29
    r0, r1, ref, pre, _, M, trio, more = _bound_case(oracle, key_type, seed)
    trio_h = plant(r0, r1, [M, M + 1, M - 1])
    wk, wh = ref.feed(trio, trio_h)
    assert int(trio[2]) in wk and int(trio[0]) not in wk and int(trio[1]) not in wk and max(wh) == M - 1
    wk, wh = ref.feed(*more)
    assert int(trio[2]) in wk and max(wh) == M - 1 and len(wk) == k
    tail = (np.concatenate([trio, more[0]]), np.concatenate([trio_h, more[1]]))
    if same_batch:
        batches = [tuple(np.concatenate([a, b]) for a, b in zip(pre, tail))]
    else:
        batches = [pre, tail]
    d = _hashed_sampler(k, seed, "ordered", key_type)
    for b in batches:
        _feed_hashed(cuda, d, *b, key_type)
    assert sorted(d.result().astype(np.int64).tolist()) == sorted(wk)


@pytest.mark.parametrize("key_type", ["long", "int"])
def test_set_admission_ties_at_the_bound(cuda, oracle, key_type):
    """Set mode's bound is inclusive: fresh keys at exactly h = M, one smaller and one larger than the
    boundary key.  The smaller one replaces the boundary key, the larger one stays out."""
    k, seed = 64, 43
    r0, r1, _, pre, _, M, trio, more = _bound_case(oracle, key_type, seed)
    sh = _scr(r0, r1, pre[1])
    wk, wh = _bottomk(pre[0], sh, k)
    assert wh[-1] == M
    tk = wk[-1]
    t_hash = int(pre[1][np.flatnonzero(pre[0] == tk)[0]])  # the boundary key's own hash value
    lo, hi = -200_001, 200_001  # outside the range every other key is drawn from
    if key_type == "long":
        lo, hi = lo * 0x10000000001 + 3, hi * 0x10000000001 + 3
    assert lo < tk < hi
    _all_distinct(pre[0], more[0], [lo, hi])
    b2 = (np.concatenate([[hi, lo], more[0]]), np.concatenate([[t_hash, t_hash], more[1]]))
    fk, fh = _bottomk(np.concatenate([pre[0], b2[0]]), _scr(r0, r1, np.concatenate([pre[1], b2[1]])), k)
    assert fk[:-1] == wk[:-1] and fk[-1] == lo and fh[-1] == M and tk not in fk and hi not in fk
    d = _hashed_sampler(k, seed, "set", key_type)
    _feed_hashed(cuda, d, *pre, key_type)
    assert d.result().astype(np.int64).tolist() == wk
    _feed_hashed(cuda, d, *b2, key_type)
    assert d.result().astype(np.int64).tolist() == fk


@pytest.mark.parametrize("k", [2, 1])
def test_scheduled_pass_extreme_plan(cuda, oracle, k):
    """A full heap next to Long.MinValue and a batch long enough (>= 9 candidate buffers) for the
    scheduled pass: its plan starts from t0 = MinValue + 4 (k = 2) or t0 = MinValue itself (k = 1), where
    k / ufrac(t0) is about k * 2^64 and every later bound is MinValue.  The pass is launched with that
    plan (asserted: it either verifies or falls back to the chunk loop, one of the two counters moves);
    whichever it does, the set is the oracle's: the key at MinValue (index 40 000) and, for k = 2,
    MinValue + 1."""
    seed, n = 47, 65_536
    assert n >= 9 * _cand_limit(k)
    r0, r1 = r01(oracle, seed)
    first = plant(r0, r1, [MIN + 1, MIN + 5] if k == 2 else [MIN + 1])
    late = plant(r0, r1, [MIN, MIN + 3])
    b2 = _rand(np.random.default_rng(k), n)
    _all_distinct(b2, first, late)
    b2[40_000], b2[7] = late
    batches = [first, b2]
    wants = _wants(oracle, k, seed, batches)
    assert wants[0][1] == ([MIN + 1, MIN + 5] if k == 2 else [MIN + 1])
    assert wants[1][1] == [MIN, MIN + 1][:k]
    d = _identity_run(cuda, k, seed, "ordered", batches, wants)
    info = d.distinct_info()
    print("scheduled pass at the range's end:", info)
    assert info["sched_passes"] + info["sched_fallbacks"] == 1, info


@pytest.mark.parametrize("c,passes", [(40, 1), (100, 1), (200, 1), (300, 0)])
def test_scheduled_pass_tagged_sort_keeps_first_arrival(cuda, oracle, c, passes):
    """The scheduled merge sorts each bucket by (h, key, arrival tag) and keeps an element's first arrival.
    k = 64, a full heap, then 65 536 distinct random keys with c repeats of X, the member planted at
    Long.MinValue, scattered among them: X never leaves the set and passes every range bound, so its merge bucket
    holds the member (tag 0) and c entries equal in (h, key) that differ in their tag alone.  c = 40 fits
    one register per lane, c = 100 needs R >= 2, c = 200 needs R = 4 (the pass verifies in all three);
    c = 300 is more than kBucketCap: the overflow verdict, and the chunk loop runs with the set restored."""
    k, seed, n = 64, 73, 65_536
    assert n >= 9 * _cand_limit(k) and (c + 1 > BUCKET_CAP) == (passes == 0)
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(c)
    h1 = _rand(rng, 5000)
    h1[1234] = MIN  # X: nothing is ever below it
    b1 = plant(r0, r1, h1)
    b2 = _rand(rng, n)
    _all_distinct(b1, b2)
    x = b1[np.argmin(_scr(r0, r1, b1))]
    b2[rng.choice(n, c, replace=False)] = x
    batches = [b1, b2]
    wants = _wants(oracle, k, seed, batches)
    assert wants[0][0][0] == wants[1][0][0] == x == b1[1234] and wants[1][1][0] == MIN and len(wants[0][0]) == k
    assert int((b2 == x).sum()) == c
    d = _identity_run(cuda, k, seed, "ordered", batches, wants)
    info = d.distinct_info()
    print(f"c={c}:", info)
    assert info["sched_passes"] + info["sched_fallbacks"] == 1, info
    assert info["sched_passes"] == passes, info


# ---- E. segmented distinct (K5) ---------------------------------------------------------------------
K5_KS = [8, 100, 300, 1100]  # one k per form (k <= 64, <= 256, <= 1024, <= 4096)
K5_S = 6


def _flat(streams):
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in streams]) if offs[-1] else np.empty(0, np.int64)
    return flat, offs


def _seg_equal(got, want, touched=None):
    gk, gh, gc = (t.cpu().numpy() for t in got)
    wk, wh, wc = want
    assert np.array_equal(gc, wc)
    gk, gh = gk.astype(np.int64).copy(), gh.copy()
    if touched is not None:  # a row that never received a key: its count says empty, its slots are not the engine's
        gk[~touched] = 0
        gh[~touched] = 0
    assert np.array_equal(gh, wh)
    assert np.array_equal(gk, wk)


def _seg_run(cuda, k, seed, base, key_streams, hash_streams=None, halves=True):
    """The stateless launch and a resumed state fed each stream in two pieces (or one)."""
    import torch

    from reservoir_amd import batch

    keys, offs = _flat(key_streams)
    kw = {"hash": "identity"}
    if hash_streams is not None:
        kw = {"hashes": _dev(cuda, _flat(hash_streams)[0])}
    stateless = batch.distinct_segmented(_dev(cuda, keys), _dev(cuda, offs), k, seed=seed, stream_base=base, **kw)
    sd = batch.SegmentedDistinct(len(key_streams), k, seed, stream_base=base,
                                 hash="identity" if hash_streams is None else "precomputed", dtype=torch.int64,
                                 device=cuda)
    cuts = [len(s) // 2 if halves else len(s) for s in key_streams]
    for piece in (0, 1):
        sl = [slice(0, c) if piece == 0 else slice(c, None) for c in cuts]
        pk, po = _flat([s[x] for s, x in zip(key_streams, sl)])
        ph = None if hash_streams is None else _dev(cuda, _flat([s[x] for s, x in zip(hash_streams, sl)])[0])
        sd.update(_dev(cuda, pk), _dev(cuda, po), hashes=ph)
    return stateless, (sd.keys, sd.hashes, sd.counts)


@pytest.mark.parametrize("k", K5_KS)
def test_k5_range_ends(cuda, oracle, k):
    """Four streams of 3k random keys with keys at Long.MinValue and Long.MaxValue (each twice), one
    stream shorter than k that holds h = MaxValue (it equals the 'not full' T's hash), one empty stream."""
    seed, base = 53, 7
    r0, r1 = _seg_r01(oracle, k, seed, base, K5_S)
    rng = np.random.default_rng(k)
    streams = []
    for s in range(4):
        rand = _rand(rng, 3 * k)
        lo, hi = plant(int(r0[s]), int(r1[s]), [MIN, MAX])
        _all_distinct(rand, [lo, hi])
        streams.append(np.concatenate([rand[:k - 1], [hi], rand[k - 1:2 * k], [lo, hi], rand[2 * k:], [lo]]))
    short = _rand(rng, max(1, k // 2) - 1)
    hi = plant(int(r0[4]), int(r1[4]), [MAX])
    _all_distinct(short, hi)
    streams += [np.concatenate([short[:1], hi, short[1:]]), np.empty(0, dtype=np.int64)]
    keys, offs = _flat(streams)
    want = _expected(keys, keys, offs, k, r0, r1)
    wk, wh, wc = want
    assert wc.tolist() == [k] * 4 + [max(1, k // 2), 0]
    assert (wh[:4, 0] == MIN).all() and (wh[:4] != MAX).all()
    assert wh[4, wc[4] - 1] == MAX and wk[4, wc[4] - 1] == hi[0] and wc[4] < k
    touched = np.diff(offs) > 0
    stateless, resumed = _seg_run(cuda, k, seed, base, streams)
    _seg_equal(stateless, want)
    _seg_equal(resumed, want, touched)


@pytest.mark.parametrize("k", K5_KS)
def test_k5_entry_equal_to_the_pad(cuda, oracle, k):
    """Precomputed hashes: the entry (h = Long.MaxValue, key = 2^63 - 1) -- the bitonic pad and the
    'not full' T -- twice in a stream whose row ends not full, exactly full (k distinct keys with it) and
    over-full (it must drop); planted at the stream's start (streams 0-2) and at its end (3-5)."""
    seed, base = 59, 3
    r0, r1 = _seg_r01(oracle, k, seed, base, K5_S)
    rng = np.random.default_rng(k + 1)
    ks, hs, distinct = [], [], []
    for s in range(K5_S):
        d = [max(2, k - 3), k, k + 5][s % 3]
        other = _rand(rng, d - 1)
        assert MAX not in other and np.unique(other).size == d - 1
        oh = _rand(rng, d - 1)
        pre = unscramble(int(r0[s]), int(r1[s]), MAX)
        assert _scr(int(r0[s]), int(r1[s]), oh).max() < MAX
        if s < 3:
            ks.append(np.concatenate([[MAX, MAX], other]))
            hs.append(np.concatenate([[pre, pre], oh]))
        else:
            ks.append(np.concatenate([other, [MAX, MAX]]))
            hs.append(np.concatenate([oh, [pre, pre]]))
        distinct.append(d)
    keys, offs = _flat(ks)
    want = _expected(keys, _flat(hs)[0], offs, k, r0, r1)
    wk, wh, wc = want
    assert wc.tolist() == [min(d, k) for d in distinct]
    for s in range(K5_S):
        if s % 3 < 2:  # kept as the row's last entry
            assert (wh[s, wc[s] - 1], wk[s, wc[s] - 1]) == (MAX, MAX)
        else:
            assert wh[s, k - 1] < MAX
    stateless, resumed = _seg_run(cuda, k, seed, base, ks, hs)
    _seg_equal(stateless, want)
    _seg_equal(resumed, want)


@pytest.mark.parametrize("k", K5_KS)
def test_k5_boundary_ties(cuda, oracle, k):
    """A first update fills every row; with T = (Th, Tk) its last entry, a second update brings
    (Th, Tk + 1), (Th, Tk) itself and (Th, Tk - 1): the last replaces T, the others change nothing."""
    import torch

    from reservoir_amd import batch

    seed, base = 61, 11
    r0, r1 = _seg_r01(oracle, k, seed, base, K5_S)
    rng = np.random.default_rng(k + 2)
    k1 = [_rand(rng, 2 * k) for _ in range(K5_S)]
    h1 = [_rand(rng, 2 * k) for _ in range(K5_S)]
    keys1, offs1 = _flat(k1)
    w1 = _expected(keys1, _flat(h1)[0], offs1, k, r0, r1)
    assert (w1[2] == k).all()
    k2, h2 = [], []
    for s in range(K5_S):
        tk = int(w1[0][s, k - 1])
        th_value = int(h1[s][np.flatnonzero(k1[s] == tk)[0]])  # the hash value that scrambles to Th
        assert MIN < tk < MAX
        _all_distinct(k1[s], [tk - 1, tk + 1])
        k2.append(np.array([tk + 1, tk, tk - 1], dtype=np.int64))
        h2.append(np.full(3, th_value, dtype=np.int64))
    keys, offs = _flat([np.concatenate(p) for p in zip(k1, k2)])
    want = _expected(keys, _flat([np.concatenate(p) for p in zip(h1, h2)])[0], offs, k, r0, r1)
    for s in range(K5_S):
        assert want[1][s, k - 1] == w1[1][s, k - 1] and want[0][s, k - 1] == w1[0][s, k - 1] - 1
        assert np.array_equal(want[0][s, :k - 1], w1[0][s, :k - 1])
    sd = batch.SegmentedDistinct(K5_S, k, seed, stream_base=base, hash="precomputed", dtype=torch.int64, device=cuda)
    sd.update(_dev(cuda, keys1), _dev(cuda, offs1), hashes=_dev(cuda, _flat(h1)[0]))
    _seg_equal((sd.keys, sd.hashes, sd.counts), w1)
    keys2, offs2 = _flat(k2)
    sd.update(_dev(cuda, keys2), _dev(cuda, offs2), hashes=_dev(cuda, _flat(h2)[0]))
    _seg_equal((sd.keys, sd.hashes, sd.counts), want)


@pytest.mark.parametrize("k", K5_KS)
def test_k5_merge_stored_extremes(cuda, oracle, k):
    """merge takes h as stored.  Three parts per row: part 0 holds h = Long.MinValue, part 1 (count < k)
    ends with h = Long.MaxValue, part 2 is full with (MaxValue, 2^63 - 1) as its last entry, or empty
    (count 0).  Rows 0-3 see more than k keys (the top entries drop), rows 4-5 fewer (both MaxValue
    entries stay, in key order).  = numpy's bottom-k of the union = one stateless launch over it."""
    import torch

    from reservoir_amd import batch

    seed, base = 67, 5
    r0, r1 = _seg_r01(oracle, k, seed, base, K5_S)
    rng = np.random.default_rng(k + 3)
    pk = [[None] * K5_S for _ in range(3)]
    ph = [[None] * K5_S for _ in range(3)]
    for s in range(K5_S):
        lo, hi = (unscramble(int(r0[s]), int(r1[s]), t) for t in (MIN, MAX))
        big = s < 4
        n0, n1 = (2 * k, max(2, k // 2)) if big else (3, 2)
        a, b = _rand(rng, n0), _rand(rng, n1)
        ah, bh = _rand(rng, n0), _rand(rng, n1)
        ah[n0 // 2], bh[0] = lo, hi
        if s % 2 == 0:
            c = np.concatenate([_rand(rng, (k if big else 2) - 1), [MAX]])
            ch = np.concatenate([_rand(rng, c.size - 1), [hi]])
        else:
            c, ch = np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
        _all_distinct(a, b, c)
        for p, (x, xh) in enumerate(((a, ah), (b, bh), (c, ch))):
            pk[p][s], ph[p][s] = x, xh
    parts = []
    for p in range(3):
        keys, offs = _flat(pk[p])
        parts.append(_expected(keys, _flat(ph[p])[0], offs, k, r0, r1))
    union_k = [np.concatenate([pk[p][s] for p in range(3)]) for s in range(K5_S)]
    union_h = [np.concatenate([ph[p][s] for p in range(3)]) for s in range(K5_S)]
    keys, offs = _flat(union_k)
    want = _expected(keys, _flat(union_h)[0], offs, k, r0, r1)
    # the stored rows hold what the case is about
    assert (parts[0][1][:, 0] == MIN).all() and parts[0][2].tolist() == [k] * 4 + [3, 3]
    assert all(parts[1][1][s, parts[1][2][s] - 1] == MAX and parts[1][2][s] < k for s in range(K5_S))
    for s in range(K5_S):
        c2 = int(parts[2][2][s])
        assert c2 == (0 if s % 2 else (k if s < 4 else 2))
        assert s % 2 or (parts[2][1][s, c2 - 1], parts[2][0][s, c2 - 1]) == (MAX, MAX)
    assert (want[1][:, 0] == MIN).all() and (want[1][:4] != MAX).all() and want[2].tolist() == [k] * 4 + [7, 5]
    assert (want[1][4, 5:7] == MAX).all() and want[0][4, 6] == MAX and want[1][5, 4] == MAX
    sd = batch.SegmentedDistinct(K5_S, k, seed, stream_base=base, hash="precomputed", dtype=torch.int64, device=cuda)
    sd.merge(*(_dev(cuda, np.stack([parts[p][i] for p in range(3)])) for i in range(3)))
    _seg_equal((sd.keys, sd.hashes, sd.counts), want)
    stateless = batch.distinct_segmented(_dev(cuda, keys), _dev(cuda, offs), k, seed=seed, stream_base=base,
                                         hashes=_dev(cuda, _flat(union_h)[0]))
    _seg_equal(stateless, want)


# ---- F. object distinct -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 100])
def test_object_candidates_at_hash_edges(cuda, oracle, k):
    """The hash-only candidate pass (strict h < bound) through the raw ABI, as
    test_gpu_object_distinct.py runs it: every admission of RandomValues is a candidate and the replayed
    set is the oracle's.  Batch A fills the set with its k-th smallest hash at Long.MaxValue (and, for
    k = 100, an element at Long.MinValue as its first, while the set is not full); B brings
    another element at MaxValue (not admitted) and one at MaxValue - 1 (admitted); D brings elements at
    the replica's bound (not admitted) and at bound - 1 (admitted); C1 holds h = Long.MinValue; C2 is
    10 000 more, with repeats of earlier elements."""
    seed = 9
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(k)
    hs_a = np.concatenate([plant(r0, r1, [MIN] if k > 1 else []), _rand(rng, max(k - 2, 0)), plant(r0, r1, [MAX])])
    assert hs_a.size == k
    hs_b = np.concatenate([plant(r0, r1, [MAX, MAX - 1]), _rand(rng, 50)])
    ab = np.concatenate([hs_a, hs_b])
    ids_ab = np.arange(ab.size, dtype=np.int64)
    _, v_ab = OD._admissions(k, ids_ab, OD._scramble(r0, r1, ab))
    bound = v_ab.max_hash
    assert MIN + 1 < bound < MAX and v_ab.size == k
    hs_d = np.concatenate([plant(r0, r1, [bound, bound - 1]), _rand(rng, 2000)])
    hs_c1 = np.concatenate([_rand(rng, 60), plant(r0, r1, [MIN]), _rand(rng, 39)])
    fresh = np.concatenate([ab, hs_d, hs_c1, _rand(rng, 9000)])
    i_max2, i_maxm1 = hs_a.size, hs_a.size + 1
    i_bound, i_boundm1 = ab.size, ab.size + 1
    i_min = ab.size + hs_d.size + 60
    repeats = np.concatenate([[i_min] * 5, rng.integers(0, fresh.size, 995)])
    ids = np.concatenate([np.arange(fresh.size), repeats]).astype(np.int64)
    n_c2 = 9000 + repeats.size
    tail = ids[-n_c2:].copy()
    rng.shuffle(tail)
    ids[-n_c2:] = tail
    hs = fresh[ids]
    cuts = tuple(np.cumsum([0, hs_a.size, hs_b.size, hs_d.size, hs_c1.size, n_c2]).tolist())
    assert cuts[-1] == ids.size and n_c2 == 10_000
    sh = OD._scramble(r0, r1, hs)
    assert [int(sh[i]) for i in (k - 1, i_max2, i_maxm1, i_bound, i_boundm1, i_min)] == \
        [MAX, MAX, MAX - 1, bound, bound - 1, MIN]
    assert k == 1 or int(sh[0]) == MIN  # planted while the set fills
    adm, v = OD._admissions(k, ids, sh)
    adm = set(adm.tolist())
    assert 0 in adm and k - 1 in adm and i_maxm1 in adm and i_boundm1 in adm and i_min in adm
    assert i_max2 not in adm and i_bound not in adm
    assert MIN in v.hashes() and (k > 1 or max(adm) == i_min)  # k = 1: nothing is admitted after MinValue
    pos, got, counts = OD._run(cuda, k, seed, ids, hs, cuts, sh)
    print(f"k={k}: admissions {len(adm)}, candidates per batch {counts}")
    assert adm <= set(pos.tolist()), "an admission of the reference is no candidate"
    assert OD._ids_as_rows(got.result()) == OD._oracle_ids(oracle, k, seed, ids, hs)
    assert got.max_hash == v.max_hash
    if k == 1:
        assert counts[-1] == 0  # bound = Long.MinValue: nothing is strictly below it


# ---- G. byte keys -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("width", [16, 24])
def test_byte_keys_at_hash_edges(cuda, oracle, width, k, order):
    """Fixed-width byte keys with precomputed hashes against oracle.DistinctRows, read after every batch:
    b1 fills the set with its top at Long.MaxValue; b2 is a further batch (2000 rows); b3 brings rows at
    the maximum M (ordered mode only: it ties, and is rejected) and at M - 1 (admitted: the new maximum);
    b4 plants Long.MinValue and another row at MaxValue among 5000; b5 follows (for k = 1 the set then
    sits at MinValue) with a repeat of the row at MinValue."""
    from reservoir_amd import Sampler

    seed = 13
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(width + k)
    ref = oracle.DistinctRows(k, seed, width)
    next_id = [0]

    def step(hashes, repeat_of=None):
        """Fresh rows for `hashes` (and a repeat of row id `repeat_of`) into the oracle; the GPU follows."""
        hashes = np.asarray(hashes, dtype=np.int64)
        ids = np.arange(next_id[0], next_id[0] + hashes.size)
        next_id[0] += hashes.size
        if repeat_of is not None:
            ids, hashes = np.append(ids, repeat_of[0]), np.append(hashes, repeat_of[1])
        rows = OD._rows(ids, width)
        ref.sample_all(rows, hashes)
        want, wh = ref.result()
        pending.append((rows, hashes, sorted(bytes(r) for r in want)))
        return ids, wh.tolist()

    pending = []
    _, wh = step(np.concatenate([_rand(rng, k - 1), plant(r0, r1, [MAX])]))
    assert len(wh) == k and wh[-1] == MAX
    _, wh = step(_rand(rng, 2000))
    M = wh[-1]
    assert MIN + 1 < M < MAX
    hv = _rand(rng, 600)
    hv = hv[_scr(r0, r1, hv) > M][:500]
    edge = plant(r0, r1, [M, M - 1] if order == "ordered" else [M - 1])
    _, wh = step(np.concatenate([edge, hv]))
    assert wh[-1] == M - 1 and wh.count(M) == 0 and len(wh) == k
    b4 = _rand(rng, 5000)
    b4[1234], b4[4321] = plant(r0, r1, [MIN, MAX])
    ids4, wh = step(b4)
    assert wh[0] == MIN and wh[-1] < MAX
    _, wh = step(_rand(rng, 1000), repeat_of=(ids4[1234], b4[1234]))
    assert wh[0] == MIN and (k > 1 or wh == [MIN])
    d = Sampler.distinct(k, key_type=f"bytes{width}", seed=seed, order=order, reusable=True)(hash=lambda b: 0)
    for i, (rows, hashes, want) in enumerate(pending):
        d.sample_all(_dev(cuda, rows), hashes=_dev(cuda, hashes))
        got = d.result()
        assert sorted(bytes(r) for r in np.ascontiguousarray(got)) == want, i


# ---- H. the row combine of distinct shards ----------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_row_combine_of_extreme_shards(cuda, oracle, order):
    """export_packed / merge_packed, k = 64, identity: an empty shard (its row says max_hash =
    Long.MinValue), a shard of 20 keys that holds h = Long.MaxValue (not full), a full shard that holds
    h = Long.MinValue.  The merged sampler equals one sampler over the whole stream; in ordered mode
    the shards retain their logs and merge through distributed.merge_local."""
    import torch

    from reservoir_amd import Sampler
    from reservoir_amd import distributed as D

    k, seed = 64, 71
    r0, r1 = r01(oracle, seed)
    lo, hi = plant(r0, r1, [MIN, MAX])
    rand = _rand(np.random.default_rng(5), 3019)
    _all_distinct(rand, [lo, hi])
    pieces = [np.empty(0, dtype=np.int64), np.concatenate([rand[:9], [hi], rand[9:19]]),
              np.concatenate([rand[19:1500], [lo], rand[1500:], rand[19:300]])]
    wants = [_wants(oracle, k, seed, [p])[0] if p.size else ([], []) for p in pieces]
    assert len(wants[1][1]) == 20 and wants[1][1][-1] == MAX
    assert len(wants[2][1]) == k and wants[2][1][0] == MIN
    whole = _wants(oracle, k, seed, [np.concatenate(pieces)])[0]
    assert whole[1][0] == MIN and MAX not in whole[1] and len(whole[1]) == k
    total = sum(p.size for p in pieces)
    shards = []
    for p in pieces:
        s = Sampler.distinct(k, seed=seed, order=order, retain_log=order == "ordered")(hash="identity")
        if p.size:
            s.sample_all(_dev(cuda, p))
        shards.append(s)
    rows = torch.empty((3, shards[0].packed_width), dtype=torch.int64, device=cuda)
    for r, s in enumerate(shards):
        s.export_packed(rows[r])
    host = rows.cpu().numpy()
    for r in range(3):
        m = len(wants[r][0])
        assert host[r, :m].tolist() == wants[r][0] and host[r, k:k + m].tolist() == wants[r][1]
        assert host[r, 2 * k:2 * k + 2].tolist() == [m, pieces[r].size]
        assert host[r, 2 * k + 3] == (wants[r][1][-1] if m else MIN)
    t = Sampler.distinct(k, seed=seed, order=order)(hash="identity")
    if order == "ordered":
        D.merge_local(t, shards)
    else:
        t.merge_packed(rows, total)
    assert t.count == total
    assert t.result().tolist() == whole[0]
