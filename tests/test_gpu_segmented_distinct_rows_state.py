"""Resumed segmented Sampler.distinct over byte keys (rsv_distinct_segmented_rows_update / _merge,
batch.SegmentedDistinctRows): S long-lived distinct samplers over rows of W bytes, advanced by one
launch per batch and combined across launches, their rows moved inside the caller-held state.

Bottom-k by (scrambled hash, row words) over distinct rows is a function of the row set alone, so
however a stream is cut into updates or split into merged parts, its state row must equal -- exactly:
rows, hashes, counts, zeros beyond the count -- segdistinct_rows_ref.expected_rows over the
CONCATENATED stream (itself pinned to oracle.DistinctRows on the CPU) and one
batch.distinct_segmented_rows launch over it.  The constructor zero-fills the counts only and an
update leaves a row without input alone, so a row that never received a row is compared by its count
(0) alone.
"""
import ctypes as C

import hash_targets as HT
import numpy as np
import pytest
from segdistinct_ref import _r01, _scramble
from segdistinct_rows_ref import U64, expected_rows, hashes_of, ragged_ids, rows_of, uuid_hashcode_np

pytestmark = pytest.mark.gpu


def _offs(lens):
    return np.r_[0, np.cumsum(lens)].astype(np.int64)


def _cuts(rng, lens, B):
    """Random cut positions: cuts[s] = 0 <= c_1 <= ... <= c_{B-1} <= len_s, as an (S, B + 1) array."""
    S = lens.size
    c = np.sort(rng.integers(0, lens[:, None] + 1, size=(S, B - 1)), axis=1)
    return np.concatenate([np.zeros((S, 1), dtype=np.int64), c, lens[:, None]], axis=1).astype(np.int64)


def _piece(offs, cuts, t, *arrays):
    """Batch t of the cut streams: (its offsets, the flat pieces of every array)."""
    ln = cuts[:, t + 1] - cuts[:, t]
    po = _offs(ln)
    idx = np.repeat(offs[:-1] + cuts[:, t] - po[:-1], ln) + np.arange(int(po[-1]))
    return (po,) + tuple(a[idx] for a in arrays)


def _stateless(cuda, rows, offs, k, seed, base, hashes=None):
    import torch

    from reservoir_amd import batch

    kw = {} if hashes is None else dict(hashes=torch.from_numpy(hashes).to(cuda))
    return batch.distinct_segmented_rows(torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                         seed=seed, stream_base=base, **kw)


def _new(cuda, S, k, W, seed, base, hash="precomputed"):
    from reservoir_amd import batch

    return batch.SegmentedDistinctRows(S, k, W, seed, stream_base=base, hash=hash, device=cuda)


def _feed(sd, cuda, po, rows, hashes=None, ids=None, **kw):
    import torch

    return sd.update(torch.from_numpy(np.ascontiguousarray(rows)).to(cuda), torch.from_numpy(po).to(cuda),
                     stream_ids=None if ids is None else torch.from_numpy(ids).to(cuda),
                     hashes=None if hashes is None else torch.from_numpy(np.ascontiguousarray(hashes)).to(cuda), **kw)


def _state(sd):
    return tuple(t.cpu().numpy().copy() for t in (sd.rows, sd.hashes, sd.counts))


def _check(got, want, touched=None):
    gr, gh, gc = got
    wr, wh, wc = (w.cpu().numpy() if hasattr(w, "cpu") else w for w in want)
    assert gr.dtype == np.uint8 and gr.shape == wr.shape
    assert np.array_equal(gc, wc)
    gr, gh = gr.copy(), gh.copy()
    if touched is not None:  # rows that never received a row: the count says empty, the slots are not the engine's
        assert not gc[~touched].any()
        gr[~touched] = 0
        gh[~touched] = 0
    assert np.array_equal(gh, wh)
    assert np.array_equal(gr, wr)  # rows and hashes beyond the count are 0 on both sides


def _first_with_distinct(seg, d):
    """The shortest prefix length of seg holding exactly d distinct ids."""
    _, first = np.unique(seg, return_index=True)
    first = np.sort(first)
    assert first.size > d
    return int(first[d])  # the position of the (d+1)-th new id: the prefix before it has d


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("k", [1, 2, 64, 65, 256, 257, 1024, 1025, 4096])
def test_batch_split_invariance(cuda, oracle, k, B):
    """B update launches over randomly cut ragged streams = numpy = one stateless launch = the oracle."""
    rng = np.random.default_rng(k * 10 + B)
    big = k >= 1024
    S = 12 if big else 60
    top = 4 * k + 5000 if big else 5000
    lens = rng.integers(0, top, size=S)
    lens[:8] = [0, 1, top, top, top, k, 4096, 3]
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    cuts = _cuts(rng, lens, B)
    cuts[6, 1:B] = 1                              # a 1-row piece, then empty pieces (B = 5), then the rest
    cuts[5, 1:B] = 0                              # empty pieces first
    for s, d in ((2, k - 1), (3, k), (4, k + 1)):  # the first piece holds exactly k - 1, k, k + 1 distinct rows
        c = _first_with_distinct(ids[offs[s]:offs[s + 1]], d)
        cuts[s, 1:B] = np.maximum(np.sort(cuts[s, 1:B]), c)
        cuts[s, 1] = c
        assert np.unique(rows[offs[s]:offs[s] + c], axis=0).shape[0] == d
    assert (np.diff(cuts, axis=1) >= 0).all()
    assert (np.diff(cuts, axis=1) % 256 != 0).any() and (np.diff(cuts, axis=1) == 0).any()
    seed, base = 77, 1000
    r0, r1 = _r01(oracle, k, seed, base, S)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    sd = _new(cuda, S, k, 16, seed, base)
    for t in range(B):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        assert _feed(sd, cuda, po, pr, ph) is sd
    got = _state(sd)
    _check(got, want, lens > 0)
    _check(got, _stateless(cuda, rows, offs, k, seed, base, hashes=hashed), lens > 0)
    for s in range(6):  # the oracle's RandomValues per stream (injective hash: the same set)
        ref = oracle.DistinctRows(k, seed + base + s, 16, "precomputed")
        ref.sample_all(rows[offs[s]:offs[s + 1]], hashed[offs[s]:offs[s + 1]])
        rr, rh = ref.result()
        m = int(got[2][s])
        assert m == rr.shape[0], s
        assert np.array_equal(got[0][s, :m], rr) and np.array_equal(got[1][s, :m], rh), s


@pytest.mark.parametrize("k", [5, 300])
@pytest.mark.parametrize("width", [24, 64, 256])
def test_widths(cuda, oracle, width, k):
    rng = np.random.default_rng(width + k)
    lens = rng.integers(0, 2500, size=60)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, width), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 5, 0, lens.size)
    cuts = _cuts(rng, lens, 3)
    sd = _new(cuda, lens.size, k, width, 5, 0)
    for t in range(3):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        _feed(sd, cuda, po, pr, ph)
    assert tuple(sd.rows.shape) == (lens.size, k, width)
    _check(_state(sd), expected_rows(rows, hashed, offs, k, r0, r1), lens > 0)
    _check(_state(sd), _stateless(cuda, rows, offs, k, 5, 0, hashes=hashed), lens > 0)


class _Universe:
    """S streams of n distinct rows each, and per stream its rows' positions in the expected order
    (scrambled hash, words): column j of `asc` is the flat index of the row at position j."""

    def __init__(self, oracle, S, n, k, W, seed, base):
        self.S, self.n, self.k, self.W = S, n, k, W
        ids = np.arange(S * n)
        self.rows, self.hashed = rows_of(ids, W), hashes_of(ids)
        self.r0, self.r1 = _r01(oracle, k, seed, base, S)
        sid = np.repeat(np.arange(S), n)
        w = self.rows.view(U64).reshape(S * n, W // 8)
        h = _scramble(self.r0[sid], self.r1[sid], self.hashed)
        self.asc = np.lexsort(tuple(w[:, j] for j in range(W // 8 - 1, -1, -1)) + (h, sid)).reshape(S, n)

    def at(self, pos):
        """(offsets, rows, hashes) of the rows at positions `pos` of every stream, `pos` in the given order."""
        idx = self.asc[:, pos].reshape(-1)
        return np.arange(0, idx.size + 1, len(pos), dtype=np.int64), self.rows[idx], self.hashed[idx]

    def want(self, pos):
        po, pr, ph = self.at(sorted(pos))
        got = expected_rows(pr, ph, po, self.k, self.r0, self.r1)
        keep = sorted(pos)[:self.k]  # the reference itself places position j before position j + 1
        assert np.array_equal(got[0][:, :len(keep)], self.rows[self.asc[:, keep].reshape(-1)].reshape(self.S, -1, self.W))
        return got


@pytest.mark.parametrize("width", [16, 256])
@pytest.mark.parametrize("k", [64, 257, 1024, 4096])
def test_rows_move_in_place(cuda, oracle, k, width):
    """A full row holding every second position of [2k, 4k), then single updates checked one by one:
    rows above the last entry (bit-identical), one row just below the first entry (every slot moves up
    by one), one in the middle, one that becomes the new last entry, k rows below the first (full
    replacement), the members twice (bit-identical).  Then the single inserts on a row holding k / 2
    entries: the count grows and nothing is trimmed."""
    import torch

    S = 6
    u = _Universe(oracle, S, 6 * k, k, width, 21, 5)
    rng = np.random.default_rng(k + width)

    def feed(sd, pos):
        po, pr, ph = u.at(list(rng.permutation(pos)))
        return _feed(sd, cuda, po, pr, ph)

    def snap(sd):
        return [t.clone() for t in (sd.rows, sd.hashes, sd.counts)]

    def same(before, sd):
        return all(torch.equal(a, b) for a, b in zip(before, (sd.rows, sd.hashes, sd.counts)))

    sd = _new(cuda, S, k, width, 21, 5)
    held = set(range(2 * k, 4 * k, 2))
    feed(sd, sorted(held) + list(range(4 * k, 4 * k + 7)))
    _check(_state(sd), u.want(held))
    before = snap(sd)
    feed(sd, list(range(4 * k - 1, 6 * k)))  # (a) every (h, row) above the row's last entry
    assert same(before, sd)
    old = _state(sd)
    feed(sd, [2 * k - 1])  # (b) just below the first entry
    held = set(sorted(held | {2 * k - 1})[:k])
    new = _state(sd)
    _check(new, u.want(held))
    assert np.array_equal(new[0][:, 1:], old[0][:, :-1]) and np.array_equal(new[1][:, 1:], old[1][:, :-1])
    mid = 2 * k + 2 * (k // 2) + 1
    assert mid not in held and min(held) < mid < max(held)
    feed(sd, [mid])  # (c) in the middle
    held = set(sorted(held | {mid})[:k])
    _check(_state(sd), u.want(held))
    top2, top1 = sorted(held)[-2:]
    assert top1 - top2 == 2
    old = _state(sd)
    feed(sd, [top1 - 1])  # (d) between the last two entries: it replaces the last one, nothing else moves
    held = set(sorted(held | {top1 - 1})[:k])
    assert max(held) == top1 - 1
    new = _state(sd)
    _check(new, u.want(held))
    assert np.array_equal(new[0][:, :-1], old[0][:, :-1]) and not np.array_equal(new[0][:, -1], old[0][:, -1])
    feed(sd, list(range(k)))  # (e) k rows below the first entry
    held = set(range(k))
    _check(_state(sd), u.want(held))
    before = snap(sd)
    feed(sd, sorted(held) * 2)  # (f) current members only
    assert same(before, sd)

    sd = _new(cuda, S, k, width, 21, 5)
    held = set(range(2 * k, 2 * k + 2 * (k // 2), 2))
    feed(sd, sorted(held))
    _check(_state(sd), u.want(held))
    for pos in (2 * k - 1, 2 * k + 2 * (k // 4) + 1, max(held) + 5):  # below the first, in the middle, the new last
        feed(sd, [pos])
        held |= {pos}
        assert len(held) <= k
        _check(_state(sd), u.want(held))
    assert int(sd.counts[0]) == k // 2 + 3


def _colliding_rows(ids, variant):
    if variant == "plain":
        return rows_of(ids, 16)
    if variant == "word0_equal":  # the compare must reach word 1
        w = rows_of(ids, 16).view(U64).reshape(-1, 2)
        w[:, 0] = 0x1234
        return w.view(np.uint8).reshape(-1, 16)
    if variant == "last_word":  # W = 64, rows that differ in their last word only
        w = np.full((ids.size, 8), 0xABCDEF0123456789, dtype=U64)
        w[:, 7] = rows_of(ids, 8).view(U64).reshape(-1)
        return w.view(np.uint8).reshape(-1, 64)
    if variant == "top_bit":  # signed and unsigned order of word 0 differ
        w = rows_of(ids, 16).view(U64).reshape(-1, 2)
        w[:, 0] = ((ids.astype(U64) & U64(1)) << U64(63)) | (ids.astype(U64) % U64(5))
        return w.view(np.uint8).reshape(-1, 16)
    raise ValueError(variant)


@pytest.mark.parametrize("k", [5, 64, 512])
@pytest.mark.parametrize("variant", ["plain", "word0_equal", "last_word", "top_bit"])
def test_ties_across_batches(cuda, oracle, k, variant):
    """hashes = id % 37, split in three: after the first batch T's row lives in the state and every
    admission is a tie on h, decided by a row compare against it."""
    rng = np.random.default_rng(k * 7 + len(variant))
    lens = rng.integers(0, 3000, size=60)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = _colliding_rows(ids, variant), ids % 37
    W = rows.shape[1]
    if variant == "top_bit":
        w0 = rows.view(np.int64).reshape(-1, 2)[:, 0]
        assert (w0 < 0).any() and (w0 > 0).any()
    cuts = _cuts(rng, lens, 3)
    # the tie population: streams whose first piece already holds more than 37 distinct ids, k or more
    first = [np.unique(ids[offs[s]:offs[s] + cuts[s, 1]]).size for s in range(lens.size)]
    assert sum(f > max(37, k) for f in first) >= 5
    r0, r1 = _r01(oracle, k, 4, 50, lens.size)
    sd = _new(cuda, lens.size, k, W, 4, 50)
    for t in range(3):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        _feed(sd, cuda, po, pr, ph)
    _check(_state(sd), expected_rows(rows, hashed, offs, k, r0, r1), lens > 0)
    _check(_state(sd), _stateless(cuda, rows, offs, k, 4, 50, hashes=hashed), lens > 0)


@pytest.mark.parametrize("k", [5, 300])
def test_uuid_twins_in_different_batches(cuda, oracle, k):
    """hash="default": UUID.hashCode on the device.  Every stream is its rows followed by the twins
    [lsb | msb] of every fourth id -- other UUIDs with the same hashCode -- and the cut between the
    last two batches falls between them: the twin ties on h with a row the state already holds."""
    rng = np.random.default_rng(k)
    lens = rng.integers(0, 2500, size=100)
    ids, offs = ragged_ids(rng, lens)
    base_rows = rows_of(ids, 16)
    parts, cut2 = [], []
    for s in range(lens.size):
        a = base_rows[offs[s]:offs[s + 1]]
        tw = a[ids[offs[s]:offs[s + 1]] % 4 == 0].reshape(-1, 2, 8)[:, ::-1].reshape(-1, 16)
        parts += [a, tw]
        cut2.append((a.shape[0], a.shape[0] + tw.shape[0]))
    rows = np.concatenate(parts)
    lens2 = np.array([c[1] for c in cut2])
    offs2 = _offs(lens2)
    cuts = _cuts(rng, lens2, 3)
    cuts[:, 2] = [c[0] for c in cut2]
    cuts[:, 1] = np.minimum(cuts[:, 1], cuts[:, 2])
    hashed = uuid_hashcode_np(rows)
    assert (lens2 > lens).sum() > 50 and np.unique(rows, axis=0).shape[0] > np.unique(base_rows, axis=0).shape[0]
    r0, r1 = _r01(oracle, k, 19, 3, lens.size)
    sd = _new(cuda, lens.size, k, 16, 19, 3, hash="default")
    for t in range(3):
        po, pr = _piece(offs2, cuts, t, rows)
        _feed(sd, cuda, po, pr)
    _check(_state(sd), expected_rows(rows, hashed, offs2, k, r0, r1), lens2 > 0)
    _check(_state(sd), _stateless(cuda, rows, offs2, k, 19, 3), lens2 > 0)


@pytest.mark.parametrize("k", [1, 64, 300])
def test_max_hash_rows_beside_the_pads(cuda, oracle, k):
    """Precomputed hashes planted so that every row's scrambled h is exactly INT64_MAX, the h of the
    sort's pads, on more than k distinct rows in the long streams; split in two."""
    rng = np.random.default_rng(k)
    lens = np.array([0, 1, k + 9, 777, 1500, 2049, 4097, 5001])
    ids, offs = ragged_ids(rng, lens)
    seed, base = 15, 2
    r0, r1 = _r01(oracle, k, seed, base, lens.size)
    rows, hashed = rows_of(ids, 16), hashes_of(ids).copy()
    cuts = _cuts(rng, lens, 2)
    for s in range(lens.size):
        a, b = int(offs[s]), int(offs[s + 1])
        hashed[a:b] = HT.unscramble(int(r0[s]), int(r1[s]), HT.MAX)
        assert (_scramble(np.full(b - a, r0[s]), np.full(b - a, r1[s]), hashed[a:b]) == HT.MAX).all()
        if b - a >= 4097:  # more than k distinct planted rows, in the stream and in its first piece
            cuts[s, 1] = max(cuts[s, 1], 3000)
            assert np.unique(ids[a:a + cuts[s, 1]]).size > k
    sd = _new(cuda, lens.size, k, 16, seed, base)
    for t in range(2):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        _feed(sd, cuda, po, pr, ph)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    assert (want[1][want[2] > 0, 0] == HT.MAX).all()
    _check(_state(sd), want, lens > 0)


def test_stream_ids_permutation_and_subset(cuda, oracle):
    """Segments in a random order of all rows; then a third of the rows, the others pre-filled with a
    sentinel pattern in rows, hashes and counts that must come back unchanged."""
    import torch

    rng = np.random.default_rng(5)
    k, S, W = 50, 120, 16
    lens = rng.integers(0, 2000, size=S)
    lens[:2] = [0, 1]
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, W), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 3, 10, S)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    cuts = _cuts(rng, lens, 2)

    def in_order(order):
        sel = np.concatenate([np.arange(offs[s], offs[s + 1]) for s in order]).astype(np.int64)
        return _offs(lens[order]), rows[sel], hashed[sel]

    sd = _new(cuda, S, k, W, 3, 10)
    for t in range(2):
        perm = rng.permutation(S)  # segment b of the launch belongs to row perm[b]
        poffs, prows, phashed = in_order(perm)
        po, pr, ph = _piece(poffs, cuts[perm], t, prows, phashed)
        _feed(sd, cuda, po, pr, ph, ids=perm.astype(np.int64))
    _check(_state(sd), want, lens > 0)

    named = np.sort(rng.permutation(S)[:S // 3])
    mask = np.zeros(S, dtype=bool)
    mask[named] = True
    sd = _new(cuda, S, k, W, 3, 10)
    sent_r = (torch.arange(S * k * W, dtype=torch.int64, device=cuda) * 7 % 251).to(torch.uint8).reshape(S, k, W)
    sent_h = -torch.arange(S * k, dtype=torch.int64, device=cuda).reshape(S, k) * 7 - 3
    sent_c = torch.arange(S, dtype=torch.int64, device=cuda) % (k + 1)
    sd.rows.copy_(sent_r)
    sd.hashes.copy_(sent_h)
    sd.counts.copy_(sent_c)
    sd.counts[torch.from_numpy(named).to(cuda)] = 0
    noffs, nrows, nhashed = in_order(named)
    for t in range(2):
        po, pr, ph = _piece(noffs, cuts[named], t, nrows, nhashed)
        _feed(sd, cuda, po, pr, ph, ids=named.astype(np.int64))
    gr, gh, gc = _state(sd)
    assert np.array_equal(gr[~mask], sent_r.cpu().numpy()[~mask])
    assert np.array_equal(gh[~mask], sent_h.cpu().numpy()[~mask])
    assert np.array_equal(gc[~mask], sent_c.cpu().numpy()[~mask])
    live = mask & (lens > 0)
    assert np.array_equal(gr[live], want[0][live]) and np.array_equal(gh[live], want[1][live])
    assert np.array_equal(gc[mask], want[2][mask])


def test_reversed_ids_grid_stride(cuda, oracle):
    """S = 100,003 short segments in reversed row order, two updates: more rows than the grid holds."""
    rng = np.random.default_rng(100_003)
    S, k = 100_003, 8
    lens = rng.integers(0, 41, size=S)
    offs = _offs(lens)
    ids = rng.integers(0, 60, size=int(offs[-1]))
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    base = 2**63 - 50_000  # the seed wraps past INT64_MAX inside the launch
    r0, r1 = _r01(oracle, k, 12, base, S)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    cuts = _cuts(rng, lens, 2)
    rev = np.arange(S - 1, -1, -1, dtype=np.int64)
    sid = np.repeat(np.arange(S), lens)
    order = np.lexsort((np.arange(sid.size), -sid))  # the streams reversed, each in its own order
    rrows, rhashed, roffs = rows[order], hashed[order], _offs(lens[rev])
    sd = _new(cuda, S, k, 16, 12, base)
    for t in range(2):
        po, pr, ph = _piece(roffs, cuts[rev], t, rrows, rhashed)
        _feed(sd, cuda, po, pr, ph, ids=rev)
    _check(_state(sd), want, lens > 0)


def test_check_ids_raises_before_any_launch(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException

    sd = _new(cuda, 10, 4, 16, 1, 0, hash="default")
    sd.rows.fill_(0xEE)
    sd.hashes.fill_(-2)
    rows = torch.arange(12 * 16, dtype=torch.int64, device=cuda).to(torch.uint8).reshape(12, 16)
    offs = torch.tensor([0, 4, 8, 12], dtype=torch.int64, device=cuda)
    for ids in ([1, 5, 1], [0, 10, 2], [-1, 3, 4]):
        with pytest.raises(IllegalArgumentException):
            sd.update(rows, offs, stream_ids=torch.tensor(ids, dtype=torch.int64, device=cuda))
    torch.cuda.synchronize()
    assert not sd.counts.any() and (sd.rows == 0xEE).all() and (sd.hashes == -2).all()
    with pytest.raises(IllegalArgumentException):  # one id per segment
        sd.update(rows, offs, stream_ids=torch.tensor([1, 2], dtype=torch.int64, device=cuda))
    sd.update(rows, offs, stream_ids=torch.tensor([9, 0, 4], dtype=torch.int64, device=cuda))
    assert sd.counts.cpu().tolist() == [4, 0, 0, 0, 4, 0, 0, 0, 0, 4]


@pytest.mark.parametrize("P", [1, 2, 8])
@pytest.mark.parametrize("k", [5, 256, 257, 1024, 1025])
def test_merge(cuda, oracle, k, P):
    """Streams split by index into P parts, each sampled by the stateless call, stacked and merged:
    into an empty state and into a non-empty one; then the merged row is resumed by one more update."""
    import torch

    rng = np.random.default_rng(k * 100 + P)
    big = k >= 1024
    S = 12 if big else 60
    top = 4 * k + 5000 if big else 5000
    lens = rng.integers(0, top, size=S)
    lens[:5] = [0, 1, top, k, 3 * k + 50]
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    seed, base = 31, 400
    r0, r1 = _r01(oracle, k, seed, base, S)
    cuts = _cuts(rng, lens, P + 2)  # piece 0 seeds the non-empty state, 1..P are the parts, P + 1 resumes
    c1 = min(k + 10, top)
    cuts[2, 1:3] = [c1, top - 5]     # stream 2: part 1 holds nearly the whole stream, more than k distinct rows
    cuts[2, 3:P + 2] = top - 5
    cuts[3, 2:P + 1] = cuts[3, 1]    # stream 3: empty parts (count 0) beside a non-empty one
    cuts[1, 1], cuts[1, 2:] = 0, 1   # stream 1: its one row is part 1 (a partial count for k > 1)
    if P >= 3:  # stream 4: part 1 empty, part 2 a few rows, part 3 more than k distinct rows, the others empty
        cuts[4, 1:3] = 10
        cuts[4, 3] = 10 + max(1, k // 2)
        cuts[4, 4:P + 2] = 3 * k + 40
    assert (np.diff(cuts, axis=1) >= 0).all()
    assert np.unique(ids[offs[2] + c1:offs[2] + top - 5]).size > k
    parts = []
    for p in range(1, P + 1):
        po, pr, ph = _piece(offs, cuts, p, rows, hashed)
        parts.append(_stateless(cuda, pr, po, k, seed, base, hashes=ph))
    pr_, ph_, pc_ = (torch.stack([x[i] for x in parts]) for i in range(3))
    pc = pc_.cpu().numpy()
    assert (pc == 0).any() and ((pc > 0) & (pc < k)).any() and (pc == k).any()
    if P >= 3:  # count 0, a partial count and a full count in one row
        assert pc[0, 4] == 0 and 0 < pc[1, 4] < k and pc[2, 4] == k

    def want_of(a, b):  # the stateless value over pieces [a, b) of every stream
        sub = np.stack([cuts[:, a], cuts[:, b]], axis=1)
        po, pr, ph = _piece(offs, sub, 0, rows, hashed)
        return po, pr, ph, expected_rows(pr, ph, po, k, r0, r1)

    # into an empty state
    sd = _new(cuda, S, k, 16, seed, base)
    assert sd.merge(pr_, ph_, pc_) is sd
    po, pr, ph, want = want_of(1, P + 1)
    _check(_state(sd), want, np.diff(po) > 0)
    _check(_state(sd), _stateless(cuda, pr, po, k, seed, base, hashes=ph), np.diff(po) > 0)

    # into a non-empty state, then one more update on the merged rows
    sd = _new(cuda, S, k, 16, seed, base)
    po, pr, ph = _piece(offs, cuts, 0, rows, hashed)
    _feed(sd, cuda, po, pr, ph)
    sd.merge(pr_, ph_, pc_)
    po, pr, ph, want = want_of(0, P + 1)
    _check(_state(sd), want, np.diff(po) > 0)
    po, pr, ph = _piece(offs, cuts, P + 1, rows, hashed)
    _feed(sd, cuda, po, pr, ph)
    _check(_state(sd), expected_rows(rows, hashed, offs, k, r0, r1), lens > 0)
    _check(_state(sd), _stateless(cuda, rows, offs, k, seed, base, hashes=hashed), lens > 0)


def test_merge_of_state_objects(cuda, oracle):
    """merge(other) and merge(a, b): the index-split recipe with SegmentedDistinctRows objects, W = 24."""
    from reservoir_amd import IllegalArgumentException

    rng = np.random.default_rng(17)
    k, S, W = 40, 50, 24
    lens = rng.integers(0, 1500, size=S)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, W), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 2, 0, S)
    cuts = _cuts(rng, lens, 3)
    sds = []
    for t in range(3):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        sds.append(_feed(_new(cuda, S, k, W, 2, 0), cuda, po, pr, ph))
    a = _new(cuda, S, k, W, 2, 0).merge(sds[0]).merge(sds[1], sds[2])
    _check(_state(a), expected_rows(rows, hashed, offs, k, r0, r1), lens > 0)
    with pytest.raises(IllegalArgumentException):
        a.merge(_new(cuda, S, k, W, 3, 0))  # another seed: its hashes mean something else
    with pytest.raises(IllegalArgumentException):
        a.merge(_new(cuda, S, k, 32, 2, 0))  # another width
    with pytest.raises(IllegalArgumentException):
        a.merge(a.rows[:1], a.hashes[:1], a.counts[:1])


def test_raw_abi(cuda, oracle):
    """The C ABI through ctypes: two updates with stream_ids_dev = NULL and rows_dev at 8 mod 16 (a UUID is
    two 8-byte loads), UUID.hashCode on the device; the row without input keeps its fill; then a merge of
    the state into a second one."""
    import torch

    from reservoir_amd import _native as N

    rng = np.random.default_rng(9)
    k, S = 100, 200
    lens = rng.integers(0, 3000, size=S)
    lens[0] = 0
    ids, offs = ragged_ids(rng, lens)
    rows = rows_of(ids, 16)
    hashed = uuid_hashcode_np(rows)
    r0, r1 = _r01(oracle, k, 6, 2, S)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    cuts = _cuts(rng, lens, 2)
    L = N.load()
    vp = C.c_void_p
    stream = vp(torch.cuda.current_stream(cuda).cuda_stream)

    def state():
        return (torch.full((S, k, 16), 0xFF, dtype=torch.uint8, device=cuda),
                torch.full((S, k), -1, dtype=torch.int64, device=cuda), torch.zeros(S, dtype=torch.int64, device=cuda))

    sr, sh, sc = state()
    for t in range(2):
        po, pr = _piece(offs, cuts, t, rows)
        words = torch.from_numpy(np.ascontiguousarray(pr).view(np.int64).reshape(-1))
        shifted = torch.empty(words.numel() + 1, dtype=torch.int64, device=cuda)
        shifted[1:] = words.to(cuda)
        assert shifted[1:].data_ptr() % 16 == 8
        od = torch.from_numpy(po).to(cuda)
        N.check(L.rsv_distinct_segmented_rows_update(
            vp(shifted[1:].data_ptr()), None, vp(od.data_ptr()), None, S, S, 16, k, N.HASH_DEFAULT, 6, 2,
            vp(sr.data_ptr()), vp(sh.data_ptr()), vp(sc.data_ptr()), stream))
        torch.cuda.synchronize()
    got = (sr.cpu().numpy(), sh.cpu().numpy(), sc.cpu().numpy())
    assert (got[0][0] == 0xFF).all() and (got[1][0] == -1).all()  # the row without input was not written
    _check(got, want, lens > 0)
    mr, mh, mc = state()
    N.check(L.rsv_distinct_segmented_rows_merge(vp(sr.data_ptr()), vp(sh.data_ptr()), vp(sc.data_ptr()), 1, S, 16, k,
                                                vp(mr.data_ptr()), vp(mh.data_ptr()), vp(mc.data_ptr()), stream))
    torch.cuda.synchronize()
    got = (mr.cpu().numpy(), mh.cpu().numpy(), mc.cpu().numpy())
    assert (got[0][0] == 0xFF).all() and (got[1][0] == -1).all()
    _check(got, want, lens > 0)


@pytest.mark.parametrize("k", [10, 700])
def test_handle_equivalence(cuda, oracle, k):
    """One Sampler.distinct(k, key_type="bytes16", seed=seed+base+s, order="set") handle per stream, fed
    the same batches."""
    import torch

    from reservoir_amd import Sampler

    rng = np.random.default_rng(k)
    S, B = 6, 4
    lens = rng.integers(0, 6000, size=S)
    lens[1] = k // 2
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    cuts = _cuts(rng, lens, B)
    sd = _new(cuda, S, k, 16, 40, 7)
    handles = [Sampler.distinct(k, key_type="bytes16", seed=40 + 7 + s, order="set")(hash=lambda b: 0) for s in range(S)]
    for t in range(B):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        _feed(sd, cuda, po, pr, ph)
        for s in range(S):
            if po[s + 1] > po[s]:
                handles[s].sample_all(torch.from_numpy(np.ascontiguousarray(pr[po[s]:po[s + 1]])).to(cuda),
                                      hashes=torch.from_numpy(np.ascontiguousarray(ph[po[s]:po[s + 1]])).to(cuda))
    gr, _, gc = _state(sd)
    for s in range(S):
        held = np.asarray(handles[s].result()).reshape(-1, 16)
        m = int(gc[s])
        assert held.shape[0] == m, s
        assert sorted(bytes(r) for r in held) == sorted(bytes(r) for r in gr[s, :m]), s


def test_stream_order_and_repeatability(cuda, oracle):
    """4 updates queued back to back on a non-default torch stream with check_ids=False, no host wait
    between them, one synchronize; two identical runs are bit-identical."""
    import torch

    rng = np.random.default_rng(8)
    k, S, B = 100, 200, 4
    lens = rng.integers(0, 3000, size=S)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 6, 0, S)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    cuts = _cuts(rng, lens, B)
    sids = torch.arange(S, dtype=torch.int64, device=cuda)
    dev = []
    for t in range(B):
        po, pr, ph = _piece(offs, cuts, t, rows, hashed)
        dev.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (pr, po, ph)))
    runs = [_new(cuda, S, k, 16, 6, 0), _new(cuda, S, k, 16, 6, 0)]
    for sd in runs:  # equal starting bytes, so that the rows no input reaches compare equal too
        sd.rows.zero_()
        sd.hashes.zero_()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        for sd in runs:
            for pr, po, ph in dev:
                sd.update(pr, po, stream_ids=sids, hashes=ph, check_ids=False)
    st.synchronize()
    _check(_state(runs[0]), want)
    assert all(torch.equal(x, y) for x, y in zip(*[(sd.rows, sd.hashes, sd.counts) for sd in runs]))


def test_bad_arguments_raise(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch

    new = batch.SegmentedDistinctRows
    with pytest.raises(IllegalArgumentException):
        new(4, 0, 16, 1, device=cuda)
    with pytest.raises(ReservoirError, match="4096"):
        new(4, 4097, 16, 1, device=cuda)
    with pytest.raises(IllegalArgumentException):
        new(4, 4, 16, 1, hash="md5", device=cuda)
    with pytest.raises(IllegalArgumentException):
        new(4, 4, 12, 1, hash="precomputed", device=cuda)
    with pytest.raises(ReservoirError, match="SegmentedDistinct "):
        new(4, 4, 8, 1, hash="precomputed", device=cuda)
    with pytest.raises(ReservoirError):
        new(4, 4, 24, 1, device=cuda)  # UUID.hashCode of 24 bytes
    sd = new(2, 4, 16, 1, device=cuda)
    assert sd.rows.dtype == torch.uint8 and tuple(sd.rows.shape) == (2, 4, 16) and not sd.counts.any()
    rows = torch.zeros((10, 16), dtype=torch.uint8, device=cuda)
    offs = torch.tensor([0, 3, 6, 10], dtype=torch.int64, device=cuda)
    hs = torch.zeros(10, dtype=torch.int64, device=cuda)
    with pytest.raises(IllegalArgumentException):
        sd.update(rows.cpu(), offs)
    with pytest.raises(IllegalArgumentException):
        sd.update(rows.view(-1), offs)  # not 2-D
    with pytest.raises(IllegalArgumentException):
        sd.update(torch.zeros((10, 24), dtype=torch.uint8, device=cuda), offs[:3])  # another width
    with pytest.raises(IllegalArgumentException):  # three segments, two rows, no ids
        sd.update(rows, offs)
    with pytest.raises(IllegalArgumentException):
        sd.update(rows, offs[:3], hashes=hs)  # hashes without hash="precomputed"
    pre = new(2, 4, 16, 1, hash="precomputed", device=cuda)
    with pytest.raises(NullPointerException):
        pre.update(rows, offs[:3])
    with pytest.raises(IllegalArgumentException):
        pre.update(rows, offs[:3], hashes=hs[:9])  # one hash per row
    with pytest.raises(IllegalArgumentException):
        sd.merge(sd.rows[:1], sd.hashes[:1], sd.counts[:1])
    with pytest.raises(IllegalArgumentException):
        sd.merge(pre)  # another hash
    assert not sd.counts.any() and not pre.counts.any()
    sd.update(rows.view(torch.int64), offs[:3])  # int64 (n, W / 8) is the same memory
    assert sd.counts.cpu().tolist() == [1, 1]
