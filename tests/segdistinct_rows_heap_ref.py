"""The model of the resumed ordered segmented distinct over byte keys (rsv_distinct_segmented_rows_ordered_update):
one reservoir_amd.values.RandomValues per stream over row.tobytes(), fed (row, scrambled hash) in pieces, plus the
slot rule: an admission that grows the heap from n to n + 1 entries takes storage slot n, an admission into a
full heap takes the slot of the root it evicts.

RowsHeapModel is what the GPU state is compared with, stream by stream, after every launch.  rebuilt_from_sorted()
is the plausible wrong state (the heap rebuilt at a cut from the set sorted by (h, words)); layout_decides() says,
from the CPU models alone, that an input can tell the two apart.  The tests at the end (CPU only;
tests/test_segdistinct_rows_heap_ref.py collects them) pin the model to oracle.DistinctRows and state the slot
invariants.
"""
import numpy as np
import pytest
from segdistinct_ref import _r01, _scramble
from segdistinct_rows_ref import U64, uuid_hashcode_np

from reservoir_amd.values import RandomValues


def _words(row_bytes):
    """A row's sort key behind its hash: its little-endian 64-bit words as unsigned values, word 0 first."""
    return tuple(np.frombuffer(row_bytes, dtype=U64).tolist())


class RowsHeapModel:
    """S RandomValues over rows of W bytes; stream s scrambles with (r0[s], r1[s]).  slot[s] maps a member's
    bytes to its storage slot."""

    def __init__(self, S, k, W, r0, r1):
        self.k, self.W = k, W
        self.r0, self.r1 = np.asarray(r0, dtype=np.int64), np.asarray(r1, dtype=np.int64)
        self.rv = [RandomValues(k) for _ in range(S)]
        self.slot = [{} for _ in range(S)]

    def feed(self, s, rows, hashed):
        """rows (n, W) uint8 and their hash values (before the scramble) into stream s, in order.  Returns the
        members admitted by this call that are still members at its end: {bytes: slot}."""
        rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1, self.W)
        hashed = np.asarray(hashed, dtype=np.int64)
        if rows.shape[0] == 0:
            return {}
        h = _scramble(np.full(hashed.size, self.r0[s]), np.full(hashed.size, self.r1[s]), hashed)
        rv, slot = self.rv[s], self.slot[s]
        new = {}
        for row, hh in zip(rows, h.tolist()):
            b = row.tobytes()
            if not rv.admits(b, hh):
                continue
            if rv.size < self.k:
                sl = rv.size
            else:
                root = rv.heap()[0][0]
                sl = slot.pop(root)
                new.pop(root, None)
            rv.sample(b, hh)
            assert b in rv
            slot[b] = new[b] = sl
        return new

    def arrays(self, s):
        """Stream s in array order: (rows (n, W) uint8, hashes [n], slots [n])."""
        e, h = self.rv[s].heap()
        rows = np.frombuffer(b"".join(e), dtype=np.uint8).reshape(len(e), self.W)
        return rows, np.array(h, dtype=np.int64), np.array([self.slot[s][b] for b in e], dtype=np.int64)

    def state(self, s):
        """Everything the engine holds of stream s, zeros where the model has nothing: (storage (k, W) with every
        member's row in its slot, hashes [k], slots [k], count)."""
        rows, h, sl = self.arrays(s)
        n = h.size
        store, oh, os_ = np.zeros((self.k, self.W), np.uint8), np.zeros(self.k, np.int64), np.zeros(self.k, np.int64)
        store[sl], oh[:n], os_[:n] = rows, h, sl
        return store, oh, os_, n

    def sorted_rows(self, s):
        """Stream s ascending by (h, words): distinct_segmented_rows_ordered's layout without the zeros."""
        rows, h, _ = self.arrays(s)
        o = sorted(range(h.size), key=lambda i: (int(h[i]), _words(rows[i].tobytes())))
        return rows[o], h[o]


def rebuilt_from_sorted(rv: RandomValues, k: int) -> RandomValues:
    """A sampler holding rv's set, its heap rebuilt by enqueueing the set ascending by (h, words)."""
    e, h = rv.heap()
    out = RandomValues(k)
    for hh, _, b in sorted((hh, _words(b), b) for hh, b in zip(h, e)):
        out.sample(b, hh)
    return out


def cut_points(n):
    """The cuts of the layout argument: 1/3, 1/2 and 2/3 of a stream's length."""
    return [n // 3, n // 2, (2 * n) // 3]


def layout_decides(rows, offs, k, r0, r1, hashed):
    """The (stream, cut) pairs whose final set differs from the uncut run when the heap is rebuilt from the sorted
    set at the cut: [(s, cut, uncut set, rebuilt set)], sets as sorted lists of row bytes."""
    W = rows.shape[1]
    out = []
    for s in range(offs.size - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        whole = RowsHeapModel(1, k, W, r0[s:s + 1], r1[s:s + 1])
        whole.feed(0, rows[a:b], hashed[a:b])
        want = sorted(whole.rv[0].heap()[0])
        for c in cut_points(b - a):
            m = RowsHeapModel(1, k, W, r0[s:s + 1], r1[s:s + 1])
            m.feed(0, rows[a:a + c], hashed[a:a + c])
            m.rv[0] = rebuilt_from_sorted(m.rv[0], k)
            m.slot[0] = {x: j for j, x in enumerate(m.rv[0].heap()[0])}
            m.feed(0, rows[a + c:b], hashed[a + c:b])
            got = sorted(m.rv[0].heap()[0])
            if got != want:
                out.append((s, c, want, got))
    return out


def feed_cuts(n, k):
    """The piece boundaries of the GPU test's six-launch feed of a stream of n rows: an empty first piece, then
    k - 1 rows, k rows, 1/2, and a last piece of 1 row."""
    return sorted([0, min(k - 1, n), min(k, n), max(n // 2, min(k, n)), max(n - 1, 0)])


def _bounds(n, cuts):
    b = [0] + list(cuts) + [n]
    return list(zip(b[:-1], b[1:]))


# ---- CPU tests (collected by tests/test_segdistinct_rows_heap_ref.py) ----

SEED = 77
KS = [1, 2, 5, 63, 64, 65]


def _case(oracle, k, precomputed):
    from test_gpu_segmented_distinct_rows_ordered import _case1

    rows, offs = _case1(k)
    hashed = uuid_hashcode_np(rows)
    if precomputed:  # the same buckets under other values: what the engine takes as hashes=
        hashed = hashed * 7 - 3
    r0, r1 = _r01(oracle, k, SEED, 0, offs.size - 1)
    return rows, offs, hashed, r0, r1


def _oracle_sorted(oracle, k, seed, seg, hs, precomputed):
    d = oracle.DistinctRows(k, seed, seg.shape[1], "precomputed" if precomputed else "uuid")
    d.sample_all(seg, hs if precomputed else None)
    return d.result()


@pytest.mark.parametrize("precomputed", [False, True])
@pytest.mark.parametrize("k", KS)
def test_model_is_the_oracle_and_its_state_ignores_the_cuts(oracle, k, precomputed):
    """Uncut and cut at 1/3, 1/2, 2/3 and at [0, k - 1, k, n // 2, n - 1]: the set sorted by (h, words) is
    oracle.DistinctRows' result(), the slots are {0..n-1} (a permutation at k), and the whole state -- storage,
    hashes, slots, count -- is the uncut run's."""
    rows, offs, hashed, r0, r1 = _case(oracle, k, precomputed)
    W = rows.shape[1]
    for s in range(offs.size - 1):
        seg, hs = rows[offs[s]:offs[s + 1]], hashed[offs[s]:offs[s + 1]]
        n = seg.shape[0]
        wr, wh = _oracle_sorted(oracle, k, SEED + s, seg, hs, precomputed)
        feeds = [_bounds(n, [])] + [_bounds(n, [c]) for c in cut_points(n)] + [_bounds(n, feed_cuts(n, k))]
        uncut = None
        for bounds in feeds:
            m = RowsHeapModel(1, k, W, r0[s:s + 1], r1[s:s + 1])
            for a, b in bounds:
                m.feed(0, seg[a:b], hs[a:b])
                _, h, sl = m.arrays(0)
                assert sorted(sl.tolist()) == list(range(h.size)), (s, bounds)  # {0..n-1}; a permutation at k
            mr, mh = m.sorted_rows(0)
            assert np.array_equal(mr, wr) and np.array_equal(mh, wh), (s, bounds)
            e, h = m.rv[0].heap()
            assert all(h[(j - 1) // 2] >= h[j] for j in range(1, len(h))) and h[0] == m.rv[0].max_hash
            st = m.state(0)
            if uncut is None:
                uncut = st
            assert all(np.array_equal(x, y) for x, y in zip(st, uncut)), (s, bounds)


@pytest.mark.parametrize("k", KS)
def test_layout_decides_for_rows(oracle, k):
    """With the heap rebuilt from the sorted set at a cut, some (stream, cut) pair ends in another set than the
    uncut oracle's, for every k >= 5 (none at k = 1, 2: a heap of one or two entries has one layout)."""
    rows, offs, hashed, r0, r1 = _case(oracle, k, False)
    pairs = layout_decides(rows, offs, k, r0, r1, hashed)
    if k < 5:
        assert not pairs
        return
    assert pairs, "no (stream, cut) pair tells a heap-array state from a sorted one"
    for s, c, want, got in pairs:
        seg = rows[offs[s]:offs[s + 1]]
        wr, _ = _oracle_sorted(oracle, k, SEED + s, seg, None, False)
        assert sorted(x.tobytes() for x in wr) == want and got != want and len(got) == len(want)


def test_slot_rule_by_hand():
    """k = 3, scramble switched off by feeding RandomValues' hashes through the model's own path: rows a..e with
    hashes 5, 7, 6, 1, 5(a again): a, b, c take slots 0, 1, 2; d evicts the root b and takes slot 1."""
    m = RowsHeapModel(1, 3, 16, [0], [0])
    rows = np.arange(5 * 16, dtype=np.uint8).reshape(5, 16)
    rv = m.rv[0]
    # (fed by hand: the model's feed scrambles, and the scramble of (0, 0) is not the identity)
    for i, h in [(0, 5), (1, 7), (2, 6)]:
        b = rows[i].tobytes()
        m.slot[0][b] = rv.size
        rv.sample(b, h)
    assert m.arrays(0)[2].tolist() == [1, 0, 2] and m.arrays(0)[1].tolist() == [7, 5, 6]
    root = rv.heap()[0][0]
    assert root == rows[1].tobytes()
    sl = m.slot[0].pop(root)
    rv.sample(rows[3].tobytes(), 1)
    m.slot[0][rows[3].tobytes()] = sl
    assert m.arrays(0)[1].tolist() == [6, 5, 1] and m.arrays(0)[2].tolist() == [2, 0, 1]
    store = m.state(0)[0]
    assert np.array_equal(store, rows[[0, 3, 2]])
