"""The model of the resumed ordered segmented distinct (tests/segdistinct_heap_ref.py), pinned on the CPU:

  against the oracle   fed the same pieces, the model's set is oracle.Distinct's (sample_all once per piece)
  the layout decides   with the heap rebuilt from the sorted set at a cut, some (stream, cut) pair ends in another
                       set than the uncut oracle's: the input the GPU test uses can tell a heap-array state from
                       a sorted one.  (Counted over test_gpu_segmented_distinct_ordered._case1's 12 streams, cut
                       at 1/3, 1/2 and 2/3: 4, 16, 9 and 13 of 36 pairs at k = 5, 64, 65, 256; none at k = 1, 2.)
"""
import numpy as np
import pytest
import segdistinct_heap_ref as H
from segdistinct_ref import _hash_np, _r01
from test_gpu_segmented_distinct_ordered import _case1

SEED = 77
KS = [5, 64, 65, 256]


def feed_cuts(n, k):
    """The piece boundaries of the GPU test's 5-launch feed of a stream of n elements: an empty first piece,
    then k - 1 elements, k elements, 1/2, and a last piece of 1 element."""
    cuts = [0, min(k - 1, n), min(k, n), max(n // 2, min(k, n)), max(n - 1, 0), n]
    return sorted(cuts)


def _pieces(n, cuts):
    b = [0] + list(cuts) + [n]
    return list(zip(b[:-1], b[1:]))


def _oracle_set(oracle, k, seed, seg, bounds):
    d = oracle.Distinct(k, seed, oracle.HASH_JAVA_LONG)
    for a, b in bounds:
        d.sample_all(seg[a:b])
    rk, rh = d.result()
    o = np.lexsort((rk, rh))
    return rk[o], rh[o]


@pytest.fixture(scope="module")
def case(oracle):
    out = {}
    for k in KS:
        keys, offs = _case1(k)
        r0, r1 = _r01(oracle, k, SEED, 0, offs.size - 1)
        out[k] = keys, offs, r0, r1
    return out


@pytest.mark.parametrize("k", KS)
def test_model_is_the_oracle_fed_the_same_pieces(oracle, case, k):
    keys, offs, r0, r1 = case[k]
    hashed = _hash_np(keys, "java_long")
    for s in range(offs.size - 1):
        seg, hs = keys[offs[s]:offs[s + 1]], hashed[offs[s]:offs[s + 1]]
        n = seg.size
        feeds = [_pieces(n, [])] + [_pieces(n, [c]) for c in H.cut_points(n)] + [_pieces(n, feed_cuts(n, k)[:-1])]
        for bounds in feeds:
            m = H.HeapModel(1, k, r0[s:s + 1], r1[s:s + 1])
            for a, b in bounds:
                m.feed(0, seg[a:b], hs[a:b])
            mk, mh, mc = m.sorted_rows()
            wk, wh = _oracle_set(oracle, k, SEED + s, seg, bounds)
            assert mc[0] == wk.size
            assert np.array_equal(mk[0, :wk.size], wk) and np.array_equal(mh[0, :wk.size], wh), (s, bounds)
            # heap(): a max-heap on h in array order, the root its maximum, the keys the set
            e, h = m.rv[0].heap()
            assert all(h[(j - 1) // 2] >= h[j] for j in range(1, len(h)))
            assert h[0] == max(h) == m.rv[0].max_hash and len(set(e)) == len(e)


@pytest.mark.parametrize("k", KS)
def test_layout_decides(oracle, case, k):
    keys, offs, r0, r1 = case[k]
    pairs = H.layout_decides(keys, offs, k, r0, r1)
    assert pairs, "no (stream, cut) pair tells a heap-array state from a sorted one"
    # against the uncut oracle, not only against the model
    for s, c, want, got in pairs:
        seg = keys[offs[s]:offs[s + 1]]
        wk, _ = _oracle_set(oracle, k, SEED + s, seg, [(0, seg.size)])
        assert sorted(wk.tolist()) == want and got != want and len(got) == len(want)


def test_heap_accessor_changes_nothing():
    from reservoir_amd.values import RandomValues

    rv = RandomValues(3)
    for key, h in [(10, 5), (11, 7), (12, 6), (13, 1), (10, 5)]:
        rv.sample(key, h)
    e, h = rv.heap()
    assert (e, h) == ([12, 10, 13], [6, 5, 1])
    e.append(99)
    h.clear()
    assert rv.heap() == ([12, 10, 13], [6, 5, 1]) and rv.size == 3 and rv.max_hash == 6
    assert rv.result() == [13, 10, 12] and rv.hashes() == [1, 5, 6]
    assert RandomValues(2).heap() == ([], [])
