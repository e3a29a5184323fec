"""reservoir_amd.values.RandomValues -- the pure-Python replica behind Sampler.distinct for any B
(key_type="object") -- against the C oracle of the reference's RandomValues (Sampler.scala:383-412).
CPU only: the replica has no GPU dependency."""
import numpy as np
import pytest

N = 60_000


def _long_hashcode(x: int) -> int:
    """java.lang.Long.hashCode, widened like `.toLong`"""
    v = (x ^ ((x & (2**64 - 1)) >> 32)) & 0xFFFFFFFF
    return v - 2**32 if v >= 2**31 else v


def _colliding(oracle):
    """smoke()'s colliding stream: Long.hashCode folded to 300 values"""
    keys = oracle.splitmix_keys(0x5EED0000, N)
    return ((keys >> 32) << 32) | (((keys >> 32) ^ (keys % 300)) & 0xFFFFFFFF)


def _replay(oracle, k, seed, keys, hash_of):
    from reservoir_amd.values import RandomValues

    ref = oracle.Distinct(k, seed, oracle.HASH_JAVA_LONG)
    r0, r1 = ref.r0, ref.r1
    v = RandomValues(k)
    for x in keys.tolist():
        v.sample(x, oracle.scramble(r0, r1, hash_of(x)))
    return v


@pytest.mark.parametrize("k", [1, 7, 200])
def test_colliding_hash_matches_the_reference_heap(oracle, k):
    """300 hash values over 60,000 elements: the boundary bucket ties, the heap's tie order decides"""
    col = _colliding(oracle)
    ref = oracle.Distinct(k, 4, oracle.HASH_JAVA_LONG)
    ref.sample_all(col)
    want, want_h = ref.result()
    v = _replay(oracle, k, 4, col, _long_hashcode)
    assert v.size == len(want) == k
    assert sorted(v.result()) == sorted(want.tolist())
    assert v.max_hash == int(want_h.max())
    assert v.hashes() == sorted(want_h.tolist())


@pytest.mark.parametrize("k", [1, 100])
def test_distinct_hashes_match_the_reference(oracle, k):
    """an all-distinct hash (identity of a 64-bit key) with 30 % repeated elements"""
    keys = oracle.splitmix_keys(77, 20_000)
    keys = np.concatenate([keys, keys[:6_000]])
    ref = oracle.Distinct(k, 9, oracle.HASH_IDENTITY)
    ref.sample_all(keys)
    want, want_h = ref.result()
    v = _replay(oracle, k, 9, keys, lambda x: x)
    assert sorted(v.result()) == sorted(want.tolist())
    assert v.max_hash == int(want_h.max())
    assert v.result() == [int(x) for x in want[np.argsort(want_h, kind="stable")]]  # ascending by hash


def test_fewer_elements_than_k(oracle):
    keys = _colliding(oracle)[:50]
    ref = oracle.Distinct(200, 4, oracle.HASH_JAVA_LONG)
    ref.sample_all(keys)
    want, want_h = ref.result()
    v = _replay(oracle, 200, 4, keys, _long_hashcode)
    assert v.size == len(want) == len(set(keys.tolist()))
    assert sorted(v.result()) == sorted(want.tolist())
    assert v.max_hash == int(want_h.max())


def test_empty_replica():
    from reservoir_amd.values import LONG_MIN, RandomValues

    v = RandomValues(3)
    assert (v.size, v.max_hash, v.result()) == (0, LONG_MIN, [])
    with pytest.raises(ValueError):
        RandomValues(0)


def test_any_hashable_element():
    """strings and tuples; equal elements are sampled once, the largest hash leaves first"""
    from reservoir_amd.values import RandomValues

    v = RandomValues(2)
    v.sample("a", 5)
    v.sample(("b", 1), 3)
    v.sample("a", 5)
    assert (v.size, v.max_hash) == (2, 5)
    v.sample("c", 7)       # not below maxHash
    v.sample("d", 5)       # strict <
    assert v.result() == [("b", 1), "a"]
    v.sample("e", 4)
    assert v.result() == [("b", 1), "e"] and v.max_hash == 4 and "a" not in v


def test_object_distinct_is_accepted_up_to_the_library():
    """key_type="object" on Sampler.distinct is no argument error: whatever fails without a GPU
    fails in the native layer (creating the handle's stream), after validation."""
    from reservoir_amd import IllegalArgumentException, NullPointerException, Sampler

    try:
        s = Sampler.distinct(5, key_type="object", seed=1)(lambda x: x)
    except (IllegalArgumentException, NullPointerException):
        raise
    except Exception as e:  # no device here
        assert "distinct needs keys" not in str(e)
    else:
        assert s.is_open and s.count == 0
        s.close()
    with pytest.raises(IllegalArgumentException):
        Sampler.distinct(0, key_type="object")(lambda x: x)
    with pytest.raises(NullPointerException):
        Sampler.distinct(5, key_type="object")(lambda x: x, hash=None)
    with pytest.raises(IllegalArgumentException):
        Sampler.distinct(5, key_type="object")(lambda x: x, hash="identity")
