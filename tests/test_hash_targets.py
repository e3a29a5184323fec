"""tests/hash_targets.py against the oracle: the inverse of the scramble is exact, and RandomValues
(oracle.Distinct) keeps keys planted at the ends of the hash range.  The GPU cases of
test_gpu_distinct_hash_edges.py rely on both."""
import numpy as np
import pytest
from hash_targets import EDGES, MAX, MIN, bucket_log, bucket_nobound, direct_branch, plant, r01, unscramble

SEEDS = [4, -7, 2**62 + 12345]


@pytest.mark.parametrize("seed", SEEDS)
def test_unscramble_round_trip(oracle, seed):
    r0, r1 = r01(oracle, seed)
    rng = np.random.default_rng(abs(seed) % 1000)
    ts = list(EDGES) + [int(t) for t in rng.integers(MIN, MAX, size=1000, dtype=np.int64, endpoint=True)]
    for t in ts:
        x = unscramble(r0, r1, t)
        assert MIN <= x <= MAX
        assert oracle.scramble(r0, r1, x) == t
    assert plant(r0, r1, EDGES).tolist() == [unscramble(r0, r1, t) for t in EDGES]


@pytest.mark.parametrize("k,targets,kept", [(1, [MAX, MIN, MIN + 1], [MIN]), (2, [MAX, MAX - 1], None)])
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_keeps_planted_ends(oracle, seed, k, targets, kept):
    """k = 1: the key at Long.MinValue wins wherever it stands.  k = 2 with only the two largest hashes
    planted: before anything else arrives the oracle holds exactly them (maxHash = Long.MaxValue)."""
    r0, r1 = r01(oracle, seed)
    keys = plant(r0, r1, targets)
    rng = np.random.default_rng(k)
    rand = rng.integers(MIN, MAX, size=2000, dtype=np.int64)
    assert np.unique(np.concatenate([rand, keys])).size == rand.size + keys.size
    if kept is None:  # the planted pair alone, then the random stream pushes both out
        ref = oracle.Distinct(k, seed, oracle.HASH_IDENTITY)
        ref.sample_all(np.concatenate([keys, keys]))
        rk, rh = ref.result()
        assert sorted(rh.tolist()) == sorted(targets) and sorted(rk.tolist()) == sorted(keys.tolist())
        ref.sample_all(rand)
        rk, rh = ref.result()
        assert not set(rk.tolist()) & set(keys.tolist()) and rh.max() < MAX - 1
        return
    for where in (0, 1000, 2000):
        stream = np.concatenate([rand[:where], keys, rand[where:], keys])
        ref = oracle.Distinct(k, seed, oracle.HASH_IDENTITY)
        ref.sample_all(stream)
        rk, rh = ref.result()
        assert rh.tolist() == kept
        assert rk.tolist() == [unscramble(r0, r1, t) for t in kept]


def test_bucket_mirror_arithmetic():
    assert [bucket_log(t) for t in (1, 40, 64, 128, 129, 200, 256, 257, 260, 300, 512, 513)] == \
        [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3]
    assert bucket_log(10**6, 3) == 3
    h = np.array([MIN, -1, 0, MAX, MIN + 2**62 - 1, MIN + 2**62], dtype=np.int64)
    assert bucket_nobound(h, 0).tolist() == [0] * 6
    assert bucket_nobound(h, 1).tolist() == [0, 0, 1, 1, 0, 0]
    assert bucket_nobound(h, 2).tolist() == [0, 1, 2, 3, 0, 1]
    # q = floor((2^64 - 1) / (span + 1)) >= 2^(64 - lb)  <=>  span + 1 < 2^lb: the direct branch
    assert not direct_branch(MAX, 5) and not direct_branch(MIN, 0)
    assert direct_branch(MIN, 1) and not direct_branch(MIN + 1, 1) and direct_branch(MIN + 2, 2)
    assert direct_branch(MIN + 39, 6) and not direct_branch(MIN + 39, 5)
