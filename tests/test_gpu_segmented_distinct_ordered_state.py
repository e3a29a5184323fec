"""Resumed ordered segmented Sampler.distinct (rsv_distinct_segmented_ordered_update, batch.SegmentedDistinctOrdered):
the state rows are RandomValues' heap arrays, and every comparison is bit for bit.

  the state   keys, hashes and counts of the rows IN ARRAY ORDER equal the model (tests/segdistinct_heap_ref.py:
              one reservoir_amd.values.RandomValues per stream, read through heap()) after EVERY launch.  The
              expectation is kept for the whole tensors: a row is replaced by the model's array (zeros beyond its
              count) exactly when the launch admitted something into it, and stands byte for byte otherwise, so
              "not touched", "not written" and "zeros beyond the count" are all the same comparison.
  result()    equals the oracle's rows (oracle.Distinct, uncut, ascending by (h, key)) and
              batch.distinct_segmented_ordered over the whole streams.
"""
import ctypes as C

import numpy as np
import pytest
import segdistinct_heap_ref as H
from hash_targets import MAX, MIN, plant, r01
from segdistinct_ref import _hash_np, _r01
from test_gpu_segmented_distinct_ordered import _case1, _differs, _oracle_rows, _reorder

pytestmark = pytest.mark.gpu

FILL = -7  # what the slots hold before the engine writes them


class Pair:
    """A SegmentedDistinctOrdered, the model of its rows, and the expected bytes of its three tensors."""

    def __init__(self, cuda, oracle, S, k, seed, base=0, hash="default", dtype=np.int64):
        import torch

        from reservoir_amd import batch

        self.torch, self.cuda, self.k, self.S, self.hash = torch, cuda, k, S, hash
        self.st = batch.SegmentedDistinctOrdered(S, k, seed, stream_base=base, hash=hash,
                                                 dtype=torch.int32 if dtype == np.int32 else torch.int64, device=cuda)
        assert self.st.keys.shape == (S, k) and self.st.hashes.shape == (S, k) and self.st.counts.shape == (S,)
        assert not self.st.counts.any().item()
        self.st.keys.fill_(FILL)
        self.st.hashes.fill_(FILL)
        r0, r1 = _r01(oracle, k, seed, base, S) if S else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        self.model = H.HeapModel(S, k, r0, r1)
        self.exp = [np.full((S, k), FILL, np.int64), np.full((S, k), FILL, np.int64), np.zeros(S, np.int64)]

    def hashed(self, keys, hashes):
        if hashes is not None:
            return hashes
        kind = self.hash if self.hash != "default" else ("java_int" if keys.dtype == np.int32 else "java_long")
        return _hash_np(keys, kind)

    def expect(self, keys, offs, ids=None, hashes=None):
        """The model takes the launch; the rows it admitted something into become the model's arrays."""
        hashed = self.hashed(keys, hashes)
        for b in range(offs.size - 1):
            s = b if ids is None else int(ids[b])
            if not 0 <= s < self.S:
                continue
            rv = self.model.rv[s]
            before = rv.heap()
            self.model.feed(s, keys[offs[b]:offs[b + 1]], hashed[offs[b]:offs[b + 1]])
            e, h = rv.heap()
            if (e, h) != before:
                for t, v in zip(self.exp, (e, h)):
                    t[s, :len(e)], t[s, len(e):] = v, 0
                self.exp[2][s] = len(e)

    def launch(self, keys, offs, ids=None, hashes=None, check_ids=True):
        t = self.torch
        dev = lambda a: None if a is None else t.from_numpy(np.ascontiguousarray(a)).to(self.cuda)  # noqa: E731
        got = self.st.update(dev(keys), dev(offs), stream_ids=dev(ids), hashes=dev(hashes), check_ids=check_ids)
        assert got is self.st

    def state(self):
        return [x.cpu().numpy().astype(np.int64) for x in (self.st.keys, self.st.hashes, self.st.counts)]

    def check(self, what=""):
        got = self.state()
        assert np.array_equal(got[2], self.exp[2]), (what, np.flatnonzero(got[2] != self.exp[2])[:10])
        for g, e, name in zip(got, self.exp, ("keys", "hashes")):
            bad = np.flatnonzero((g != e).any(axis=1))
            assert bad.size == 0, (what, name, bad[:10], g[bad[0]][:8], e[bad[0]][:8])

    def update(self, keys, offs, ids=None, hashes=None, check_ids=True, what=""):
        self.launch(keys, offs, ids, hashes, check_ids)
        self.expect(keys, offs, ids, hashes)
        self.check(what)

    def result(self):
        before = self.state()
        r = self.st.result()
        assert r[0].dtype == self.st.keys.dtype and r[0].data_ptr() != self.st.keys.data_ptr()
        assert all(np.array_equal(a, b) for a, b in zip(before, self.state()))  # the state is left as it is
        return [x.cpu().numpy().astype(np.int64) for x in r]

    def check_result(self, want, what=""):
        got = self.result()
        for g, w, name in zip(got, want, ("keys", "hashes", "counts")):
            assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[:10])


def _pieces(keys, offs, cuts, hashes=None):
    """The launches of a feed: cuts[s] are stream s's piece boundaries (without 0 and its length); launch j
    holds piece j of every stream.  Yields (keys, offs[, hashes])."""
    S = offs.size - 1
    bounds = [[0] + list(cuts[s]) + [int(offs[s + 1] - offs[s])] for s in range(S)]
    for j in range(len(bounds[0]) - 1):
        idx = [np.arange(offs[s] + bounds[s][j], offs[s] + bounds[s][j + 1]) for s in range(S)]
        o = np.r_[0, np.cumsum([i.size for i in idx])].astype(np.int64)
        idx = np.concatenate(idx).astype(np.int64)
        yield (keys[idx], o) if hashes is None else (keys[idx], o, hashes[idx])


def _feed_cuts(n, k):
    """An empty first piece, then k - 1 elements, k elements, 1/2, and a last piece of 1 element (every one of
    these boundaries is a cut, which makes six launches; n >= 5k + 8 keeps them in this order)."""
    return [0, k - 1, k, n // 2, n - 1]


_REF = {}


def _case1_ref(cuda, oracle, k):
    """Case 1's input, the uncut oracle rows and the stateless ordered launch, once per k."""
    import torch

    from reservoir_amd import batch

    if k not in _REF:
        keys, offs = _case1(k, 4 if k == 4096 else 12)
        want = _oracle_rows(oracle, keys, offs, k, 77, kind=oracle.HASH_JAVA_LONG)
        one = batch.distinct_segmented_ordered(torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                               seed=77, hash="default")
        one = [x.cpu().numpy() for x in one[:3]]
        assert all(np.array_equal(a, b) for a, b in zip(one, want))
        _REF[k] = keys, offs, want
    return _REF[k]


@pytest.mark.parametrize("feed", ["one", "half", "cuts"])
@pytest.mark.parametrize("k", [1, 2, 5, 63, 64, 65, 511, 512, 513, 1024, 4096])
def test_cuts_over_every_size(cuda, oracle, k, feed):
    keys, offs, want = _case1_ref(cuda, oracle, k)
    S = offs.size - 1
    lens = np.diff(offs)
    cuts = {"one": [[] for n in lens], "half": [[n // 2] for n in lens], "cuts": [_feed_cuts(int(n), k) for n in lens]}[feed]
    p = Pair(cuda, oracle, S, k, 77)
    for j, (pk, po) in enumerate(_pieces(keys, offs, cuts)):
        p.update(pk, po, what=(feed, j))
    assert np.array_equal(p.exp[2], want[2])
    p.check_result(want, feed)


@pytest.mark.parametrize("k", [5, 64, 65, 256])
def test_the_input_can_tell_a_sorted_state_from_a_heap(oracle, k):
    """The guard of test_cuts_over_every_size's input, from the CPU models alone: with the heap rebuilt from the
    sorted set at a cut, some (stream, cut) pair ends in another set than the uncut oracle's."""
    keys, offs = _case1(k)
    r0, r1 = _r01(oracle, k, 77, 0, offs.size - 1)
    pairs = H.layout_decides(keys, offs, k, r0, r1)
    assert pairs
    want = _oracle_rows(oracle, keys, offs, k, 77, kind=oracle.HASH_JAVA_LONG)
    s, c, uncut, rebuilt = pairs[0]
    assert sorted(want[0][s, :want[2][s]].tolist()) == uncut != rebuilt


@pytest.mark.parametrize("k", [64, 1024])
@pytest.mark.parametrize("how", ["reversed", "permuted"])
def test_arrival_order_across_a_cut(cuda, oracle, k, how):
    keys, offs, fwd = _case1_ref(cuda, oracle, k)
    keys = _reorder(keys, offs, how)
    want = _oracle_rows(oracle, keys, offs, k, 77, kind=oracle.HASH_JAVA_LONG)
    assert _differs(want, fwd).any()  # the order decides the set
    p = Pair(cuda, oracle, offs.size - 1, k, 77, hash="java_long")
    for pk, po in _pieces(keys, offs, [[n // 3, (2 * n) // 3] for n in np.diff(offs)]):
        p.update(pk, po)
    p.check_result(want)


@pytest.mark.parametrize("k", [5, 64, 512])
def test_precomputed_hashes(cuda, oracle, k):
    """Keys 0 .. 5k under key % (k // 2 + 1): fewer hash values than k, every full stream is tied; 3 pieces."""
    rng = np.random.default_rng(k)
    segs = []
    for s in range(8):
        d = rng.permutation(5 * k + 1) if s < 6 else rng.permutation(5 * k + 1)[:k - 2 if s == 6 else k]
        segs.append(np.r_[d, rng.choice(d, size=max(1, (3 * d.size) // 10))].astype(np.int64))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    keys = np.concatenate(segs)
    hashed = keys % (k // 2 + 1)
    want = _oracle_rows(oracle, keys, offs, k, 11, 3, hashes=hashed)
    assert np.array_equal(want[2], [k] * 6 + [k - 2, k])
    p = Pair(cuda, oracle, 8, k, 11, base=3, hash="precomputed")
    for pk, po, ph in _pieces(keys, offs, [[n // 3, (2 * n) // 3] for n in np.diff(offs)], hashed):
        p.update(pk, po, hashes=ph)
    p.check_result(want)


def _set_state(cuda, S, k, seed, base, hash, dtype):
    import torch

    from reservoir_amd import batch

    return batch.SegmentedDistinct(S, k, seed, stream_base=base, hash=hash, dtype=dtype, device=cuda)


def test_int32_keys_and_the_set_state_under_an_injective_hash(cuda, oracle):
    """int32 keys under java_int, 3 pieces: the state is the model's, and -- the hash being injective -- result()
    is SegmentedDistinct's state fed the same pieces."""
    import torch

    k, S, seed, base = 17, 9, 9, 4
    rng = np.random.default_rng(17)
    lens = rng.integers(0, 900, size=S)
    lens[:4] = [0, 1, k, k + 1]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n = int(offs[-1])
    keys = np.where(rng.random(n) < 0.5, rng.integers(-2**31, 2**31, size=n), rng.integers(-40, 40, size=n)).astype(np.int32)
    want = _oracle_rows(oracle, keys, offs, k, seed, base, kind=oracle.HASH_JAVA_INT)
    p = Pair(cuda, oracle, S, k, seed, base=base, hash="java_int", dtype=np.int32)
    sd = _set_state(cuda, S, k, seed, base, "java_int", torch.int32)
    assert p.st.keys.dtype == torch.int32
    for pk, po in _pieces(keys, offs, [[n // 3, (2 * n) // 3] for n in lens]):
        p.update(pk, po)
        sd.update(torch.from_numpy(pk).to(cuda), torch.from_numpy(po).to(cuda))
    p.check_result(want)
    assert (want[2] == k).any() and (want[2] < k).any()
    mine = p.st.result()
    written = (sd.counts > 0)[:, None]
    assert torch.equal(mine[2], sd.counts)
    assert torch.equal(mine[0] * written, sd.keys * written) and torch.equal(mine[1] * written, sd.hashes * written)


def test_hash_edges_across_a_cut(cuda, oracle):
    """k = 64.  Identity keys planted at exact scrambled hashes, MIN, MIN + 1, MAX - 1 and MAX among them, cut in
    the middle; at the end a key at MIN + 2 evicts the root (MAX), and MAX itself, arriving again, is refused by
    the new root MAX - 1.  Precomputed: a second key at MAX arrives in the second launch and is refused (MAX < MAX fails), then
    a smaller hash evicts the first; and k + 1 keys at MIN split over two launches: the last one is refused."""
    k, seed = 64, 31
    rng = np.random.default_rng(1)
    below = [MIN, MIN + 1, -1, 0, MAX - 1] + [int(x) for x in rng.integers(-2**62, 2**62, size=k - 6)]
    ra = r01(oracle, seed)
    ident = plant(*ra, below + [MAX])
    ident = ident[rng.permutation(k)]
    assert np.unique(ident).size == k
    ident = np.r_[ident[:40], ident[5:30], ident[40:], ident[::3], plant(*ra, [MIN + 2, MAX])]
    p = Pair(cuda, oracle, 1, k, seed, hash="identity")
    offs = np.array([0, ident.size], dtype=np.int64)
    for pk, po in _pieces(ident, offs, [[50]]):
        p.update(pk, po)
    want = _oracle_rows(oracle, ident, offs, k, seed, kind=oracle.HASH_IDENTITY)
    assert want[1][0, 0] == MIN and want[1][0, 1] == MIN + 1 and want[1][0, 2] == MIN + 2 and want[2][0] == k
    assert want[1][0, k - 1] == MAX - 1  # MAX was the root and left
    p.check_result(want)

    seed = 41
    r = [r01(oracle, seed + s) for s in range(2)]
    key0 = np.r_[np.arange(100, 100 + k - 1), 9000, 8000, np.arange(100, 120), 7000].astype(np.int64)
    h0 = plant(*r[0], below + [MAX, MAX] + below[:20] + [5])
    key1 = rng.permutation(k + 1).astype(np.int64)
    h1 = plant(*r[1], [MIN] * (k + 1))
    keys, hashed = np.r_[key0, key1], np.r_[h0, h1]
    offs = np.array([0, key0.size, key0.size + key1.size], dtype=np.int64)
    q = Pair(cuda, oracle, 2, k, seed, hash="precomputed")
    launches = list(_pieces(keys, offs, [[k], [k // 2]], hashed))
    q.update(launches[0][0], launches[0][1], hashes=launches[0][2])
    root = q.state()
    assert root[1][0, 0] == MAX and root[0][0, 0] == 9000 and root[2].tolist() == [k, k // 2]
    q.update(launches[1][0], launches[1][1], hashes=launches[1][2])
    got = q.result()
    assert 8000 not in got[0][0] and 9000 not in got[0][0] and 7000 in got[0][0]
    assert got[2].tolist() == [k, k] and (got[1][1] == MIN).all()
    assert sorted(got[0][1].tolist()) == sorted(key1[:k].tolist())
    q.check_result(_oracle_rows(oracle, keys, offs, k, seed, hashes=hashed))


def _small(S, k, seed=5):
    """S streams of up to 4 keys per Long.hashCode (case 1's recipe), 6k elements each."""
    rng = np.random.default_rng(seed)
    segs = []
    for s in range(S):
        n = 6 * k
        lo, hi = rng.integers(0, k + 3, n), rng.integers(0, 4, n)
        segs.append((hi.astype(np.int64) << 32) | (lo ^ hi).astype(np.int64))
    return segs


def test_stream_ids_and_rows_left_alone(cuda, oracle):
    """A subset of the rows in a shuffled order; an id outside [0, S) with check_ids=False is skipped; rows not
    named and rows with an empty segment are byte-identical before and after (Pair.check compares every byte)."""
    S, k = 9, 5
    segs = _small(S, k)  # 30 elements each
    p = Pair(cuda, oracle, S, k, 21, base=2)
    fed = [np.zeros(0, np.int64) for _ in range(S)]

    def go(ids, parts, **kw):
        offs = np.r_[0, np.cumsum([x.size for x in parts])].astype(np.int64)
        p.update(np.concatenate(parts), offs, ids=np.array(ids, dtype=np.int64), **kw)
        for r, x in zip(ids, parts):
            if 0 <= r < S:
                fed[r] = np.r_[fed[r], x]

    go([6, 1, 8, 3, 0], [segs[6][:20], segs[1][:0], segs[8][:13], segs[3][:0], segs[0][:25]], what="subset")
    assert [int(c > 0) for c in p.exp[2]] == [1, 0, 0, 0, 0, 0, 1, 0, 1]
    assert (p.state()[0][[1, 2, 3, 4, 5, 7]] == FILL).all()
    # the second pieces, other rows and another order; one id behind the state, one negative
    go([3, S, 6, -1, 8, 2], [segs[3][:11], segs[0][:9], segs[6][20:], segs[1][:4], segs[8][:0], segs[2][:3]],
       check_ids=False, what="outside")
    assert [int(c > 0) for c in p.exp[2]] == [1, 0, 1, 1, 0, 0, 1, 0, 1]
    assert (p.state()[0][[1, 4, 5, 7]] == FILL).all()
    woffs = np.r_[0, np.cumsum([x.size for x in fed])].astype(np.int64)
    p.check_result(_oracle_rows(oracle, np.concatenate(fed), woffs, k, 21, 2, kind=oracle.HASH_JAVA_LONG))


def test_a_row_that_admits_nothing_is_not_written(cuda, oracle):
    """A partial row with sentinels beyond its count, fed only repeats of its members: the sentinels survive.
    When it then admits one new key, zeros follow its count.  A full row fed what it refuses is not written either."""
    S, k = 3, 8
    p = Pair(cuda, oracle, S, k, 3)
    first = np.array([11, 12, 13], dtype=np.int64)
    full = np.arange(100, 100 + 40, dtype=np.int64)
    p.update(np.r_[first, full], np.array([0, 3, 3, 43], dtype=np.int64))
    assert p.exp[2].tolist() == [3, 0, k] and not p.exp[0][0, 3:].any()
    p.st.keys[0, 3:] = -99
    p.st.hashes[0, 3:] = -98
    p.exp[0][0, 3:], p.exp[1][0, 3:] = -99, -98
    refused = np.array([x for x in range(100, 140) if x not in set(p.exp[0][2].tolist())][:5], dtype=np.int64)
    before = [x.copy() for x in p.exp]
    p.update(np.r_[first[::-1], first, refused, p.exp[0][2]],
             np.array([0, 6, 6, 6 + 5 + k], dtype=np.int64), what="repeats")
    assert all(np.array_equal(a, b) for a, b in zip(before, p.exp))  # the model admitted nothing: nothing may move
    assert (p.state()[0][0, 3:] == -99).all() and (p.state()[1][0, 3:] == -98).all()
    p.update(np.array([12, 14], dtype=np.int64), np.array([0, 2], dtype=np.int64), what="one new key")
    assert p.exp[2][0] == 4 and not p.state()[0][0, 4:].any() and not p.state()[1][0, 4:].any()


def test_counts_are_clamped(cuda, oracle):
    """counts[r] = k + 7 behaves as a row of k entries, counts[r] = -3 as the empty row (on rows other than the
    last: a missing clamp would still read inside the allocation)."""
    import torch

    S, k = 4, 64
    segs = _small(S, k, seed=9)
    p = Pair(cuda, oracle, S, k, 15)
    keys = np.concatenate([x[:3 * k] for x in segs])
    offs = np.arange(0, S * 3 * k + 1, 3 * k, dtype=np.int64)
    p.update(keys, offs)
    assert p.exp[2].tolist() == [k] * S
    p.st.counts[0] = k + 7
    p.st.counts[1] = -3
    torch.cuda.synchronize()
    p.exp[2][0], p.exp[2][1] = k + 7, -3
    r0, r1 = p.model.r0, p.model.r1
    p.model.rv[1] = H.HeapModel(1, k, r0[1:2], r1[1:2]).rv[0]  # the empty sampler
    keys2 = np.concatenate([x[3 * k:] for x in segs])
    offs2 = np.r_[0, np.cumsum([x.size - 3 * k for x in segs])].astype(np.int64)
    p.update(keys2, offs2, what="clamped")
    assert p.exp[2].tolist() == [k] * S  # both rows admitted something and were written, with their true counts
    want = _oracle_rows(oracle, np.concatenate([segs[0], segs[1][3 * k:], segs[2], segs[3]]),
                        np.r_[0, np.cumsum([segs[0].size, segs[1].size - 3 * k, segs[2].size, segs[3].size])].astype(np.int64),
                        k, 15, kind=oracle.HASH_JAVA_LONG)
    # (row 1's oracle is seeded 15 + 1 like the row, fed only the second piece)
    p.check_result(want)


def test_one_ordered_handle_per_stream(cuda, oracle):
    import torch

    from reservoir_amd import Sampler

    k, seed, S = 64, 77, 16
    keys, offs = _case1(k, S)
    p = Pair(cuda, oracle, S, k, seed, hash="java_long")
    handles = [Sampler.distinct(k, seed=seed + s, order="ordered")(hash="java_long") for s in range(S)]
    for pk, po in _pieces(keys, offs, [[n // 3, (2 * n) // 3] for n in np.diff(offs)]):
        p.update(pk, po)
        for s, d in enumerate(handles):
            d.sample_all(torch.from_numpy(pk[po[s]:po[s + 1]]).to(cuda))
    gk, gh, gc = p.result()
    assert np.array_equal(gk, _oracle_rows(oracle, keys, offs, k, seed, kind=oracle.HASH_JAVA_LONG)[0])
    for s, d in enumerate(handles):
        assert np.array_equal(np.sort(d.result()), np.sort(gk[s, :gc[s]])), s


def test_grid_stride_over_many_rows(cuda, oracle):
    """20 011 rows of 8 elements at k = 2, 3 hash codes x 4 keys, as two launches of 4 elements each."""
    S, k = 20_011, 2
    rng = np.random.default_rng(20_011)
    lo, hi = rng.integers(0, 3, 8 * S), rng.integers(0, 4, 8 * S)
    keys = (hi.astype(np.int64) << 32) | (lo ^ hi).astype(np.int64)
    offs = np.arange(0, 8 * S + 1, 8, dtype=np.int64)
    want = _oracle_rows(oracle, keys, offs, k, 3, kind=oracle.HASH_JAVA_LONG)
    p = Pair(cuda, oracle, S, k, 3)
    for pk, po in _pieces(keys, offs, [[4]] * S):
        p.update(pk, po)
    p.check_result(want)


def test_side_stream_and_the_same_launch_again(cuda, oracle):
    """update() on a non-default torch stream; the same launch on a copy of the state gives the same state."""
    import torch

    k = 64
    keys, offs, want = _case1_ref(cuda, oracle, k)
    S = offs.size - 1
    p = Pair(cuda, oracle, S, k, 77)
    launches = list(_pieces(keys, offs, [[n // 2] for n in np.diff(offs)]))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        p.update(*launches[0])
        copy = [x.clone() for x in (p.st.keys, p.st.hashes, p.st.counts)]
        p.update(*launches[1])
        after = [x.clone() for x in (p.st.keys, p.st.hashes, p.st.counts)]
        p.st.keys, p.st.hashes, p.st.counts = copy
        p.launch(*launches[1])
    st.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(after, (p.st.keys, p.st.hashes, p.st.counts)))
    p.check()
    p.check_result(want)


def test_offsets_past_zero(cuda, oracle):
    k = 64
    keys, offs, want = _case1_ref(cuda, oracle, k)
    p = Pair(cuda, oracle, offs.size - 1, k, 77)
    for pk, po in _pieces(keys, offs, [[n // 2] for n in np.diff(offs)]):
        junk = np.array([1, 2, 3], dtype=np.int64)
        p.launch(np.r_[junk, pk], po + 3)
        p.expect(pk, po)
        p.check()
    p.check_result(want)


def test_no_segments_and_no_rows(cuda, oracle):
    import torch

    p = Pair(cuda, oracle, 3, 4, 1)
    p.update(np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64))  # num_segments == 0
    p.update(np.zeros(0, dtype=np.int64), np.zeros(4, dtype=np.int64))  # three empty segments
    assert not p.exp[2].any()
    z = Pair(cuda, oracle, 0, 4, 1)  # S == 0
    z.update(np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64))
    z.update(np.arange(6, dtype=np.int64), np.array([0, 2, 6], dtype=np.int64), ids=np.array([0, 1], dtype=np.int64),
             check_ids=False)
    r = z.st.result()
    assert r[0].shape == (0, 4) and r[1].shape == (0, 4) and r[2].shape == (0,)
    torch.cuda.synchronize()


def test_bad_arguments_raise_what_the_set_state_raises(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch
    from reservoir_amd import _native as N

    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinctOrdered(4, 0, 1, device=cuda)
    with pytest.raises(ReservoirError, match="4096"):
        batch.SegmentedDistinctOrdered(4, 4097, 1, device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinctOrdered(4, 4, 1, hash="md5", device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinctOrdered(-1, 4, 1, device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinctOrdered(4, 4, 1, dtype=torch.float32, device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinctOrdered(4, 4, 1, device="cpu")
    sd = batch.SegmentedDistinctOrdered(2, 4, 1, device=cuda)
    ref = batch.SegmentedDistinct(2, 4, 1, device=cuda)
    keys = torch.arange(10, dtype=torch.int64, device=cuda)
    offs = torch.tensor([0, 3, 6, 10], dtype=torch.int64, device=cuda)
    ids = lambda *a: torch.tensor(a, dtype=torch.int64, device=cuda)  # noqa: E731
    calls = [
        (IllegalArgumentException, lambda s: s.update(keys.cpu(), offs)),
        (IllegalArgumentException, lambda s: s.update(keys.to(torch.int32), offs)),
        (IllegalArgumentException, lambda s: s.update(keys, offs)),  # three segments, two rows, no ids
        (IllegalArgumentException, lambda s: s.update(keys, offs[:3], hashes=keys[:6])),
        (IllegalArgumentException, lambda s: s.update(keys, offs, stream_ids=ids(0, 1, 0))),
        (IllegalArgumentException, lambda s: s.update(keys, offs, stream_ids=ids(0, 1, 2))),
        (IllegalArgumentException, lambda s: s.update(keys, offs, stream_ids=ids(0, -1, 1))),
        (IllegalArgumentException, lambda s: s.update(keys, offs, stream_ids=ids(0, 1))),
    ]
    for exc, call in calls:
        msgs = []
        for s in (sd, ref):
            with pytest.raises(exc) as e:
                call(s)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    with pytest.raises(NullPointerException):
        batch.SegmentedDistinctOrdered(2, 4, 1, hash="precomputed", device=cuda).update(keys, offs[:3])
    torch.cuda.synchronize()
    assert not sd.counts.any().item()
    vp = C.c_void_p
    with pytest.raises(NullPointerException, match="state_hashes_dev"):
        N.check(N.load().rsv_distinct_segmented_ordered_update(
            vp(keys.data_ptr()), None, vp(offs.data_ptr()), None, 1, 2, 8, 4, N.HASH_IDENTITY, 1, 0,
            vp(sd.keys.data_ptr()), None, vp(sd.counts.data_ptr()), None))


def test_merge_raises(cuda):
    from reservoir_amd import ReservoirError, batch

    sd = batch.SegmentedDistinctOrdered(2, 4, 1, device=cuda)
    with pytest.raises(ReservoirError, match="SegmentedDistinct.merge"):
        sd.merge(sd)
    with pytest.raises(ReservoirError, match="SegmentedDistinct.merge"):
        sd.merge(sd.keys, sd.hashes, sd.counts)
