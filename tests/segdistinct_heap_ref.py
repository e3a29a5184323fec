"""The model of the resumed ordered segmented distinct (rsv_distinct_segmented_ordered_update): one
reservoir_amd.values.RandomValues per stream, fed (key, scrambled hash) in pieces, its state read through heap():
the queue's array order is the state's layout.

HeapModel is what the GPU state is compared with, row by row, after every launch.  rebuilt_from_sorted() is the
plausible wrong state (the heap rebuilt at a cut from the sorted set); layout_decides() says, from the CPU models
alone, that an input can tell the two apart.
"""
import numpy as np
from segdistinct_ref import _hash_np, _scramble

from reservoir_amd.values import RandomValues


class HeapModel:
    """S RandomValues; stream s scrambles with (r0[s], r1[s])."""

    def __init__(self, S, k, r0, r1):
        self.k = k
        self.r0, self.r1 = np.asarray(r0, dtype=np.int64), np.asarray(r1, dtype=np.int64)
        self.rv = [RandomValues(k) for _ in range(S)]

    def feed(self, s, keys, hashed):
        """keys and their hash values (before the scramble) into stream s, in order."""
        keys = np.asarray(keys).astype(np.int64)
        hashed = np.asarray(hashed, dtype=np.int64)
        if keys.size == 0:
            return
        h = _scramble(np.full(keys.size, self.r0[s]), np.full(keys.size, self.r1[s]), hashed)
        rv = self.rv[s]
        for key, hh in zip(keys.tolist(), h.tolist()):
            rv.sample(key, hh)

    def feed_all(self, keys, offs, hashed, ids=None):
        """Segment b of (keys, offs) into stream ids[b] (None: b)."""
        for b in range(offs.size - 1):
            s = b if ids is None else int(ids[b])
            if 0 <= s < len(self.rv):
                self.feed(s, keys[offs[b]:offs[b + 1]], hashed[offs[b]:offs[b + 1]])

    def rows(self):
        """(keys, hashes, counts) in array order, zeros beyond the count: the state as the engine holds it once
        every row has been written."""
        S, k = len(self.rv), self.k
        ok, oh, oc = np.zeros((S, k), np.int64), np.zeros((S, k), np.int64), np.zeros(S, np.int64)
        for s, rv in enumerate(self.rv):
            e, h = rv.heap()
            ok[s, :len(e)], oh[s, :len(e)], oc[s] = e, h, len(e)
        return ok, oh, oc

    def sorted_rows(self):
        """The rows ascending by (h, key): distinct_segmented_ordered's layout."""
        return sort_rows(*self.rows())


def sort_rows(keys, hashes, counts):
    ok, oh = np.zeros_like(keys), np.zeros_like(hashes)
    for s in range(keys.shape[0]):
        n = int(counts[s])
        o = np.lexsort((keys[s, :n], hashes[s, :n]))
        ok[s, :n], oh[s, :n] = keys[s, :n][o], hashes[s, :n][o]
    return ok, oh, counts.copy()


def rebuilt_from_sorted(rv: RandomValues, k: int) -> RandomValues:
    """A sampler holding rv's set, its heap rebuilt by enqueueing the set ascending by (h, key)."""
    e, h = rv.heap()
    out = RandomValues(k)
    for hh, key in sorted(zip(h, e)):
        out.sample(key, hh)
    return out


def cut_points(n):
    """The cuts of the layout argument: 1/3, 1/2 and 2/3 of a stream's length."""
    return [n // 3, n // 2, (2 * n) // 3]


def layout_decides(keys, offs, k, r0, r1, kind="java_long"):
    """The (stream, cut) pairs whose final set differs from the uncut run when the heap is rebuilt from the
    sorted set at the cut: [(s, cut, uncut set, rebuilt set)], sets as sorted lists of keys."""
    hashed = _hash_np(keys, kind)
    out = []
    for s in range(offs.size - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        whole = HeapModel(1, k, r0[s:s + 1], r1[s:s + 1])
        whole.feed(0, keys[a:b], hashed[a:b])
        want = sorted(whole.rv[0].heap()[0])
        for c in cut_points(b - a):
            m = HeapModel(1, k, r0[s:s + 1], r1[s:s + 1])
            m.feed(0, keys[a:a + c], hashed[a:a + c])
            m.rv[0] = rebuilt_from_sorted(m.rv[0], k)
            m.feed(0, keys[a + c:b], hashed[a + c:b])
            got = sorted(m.rv[0].heap()[0])
            if got != want:
                out.append((s, c, want, got))
    return out
