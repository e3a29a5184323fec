"""Resumed ordered segmented Sampler.distinct over byte keys (rsv_distinct_segmented_rows_ordered_update,
batch.SegmentedDistinctRowsOrdered): the state is RandomValues' heap array holding references -- hashes and slots in
array order, the rows in their slots -- and every comparison is bit for bit.

  the state   rows, hashes, slots and counts equal the model (tests/segdistinct_rows_heap_ref.py: one
              reservoir_amd.values.RandomValues per stream over row.tobytes(), plus the slot rule) after EVERY launch.
              The expectation is kept for the whole tensors, which start filled with a pattern: when a launch admits
              something into a row, its hashes and slots become the model's arrays (zeros beyond the count), the
              rows it admitted that are still members land in their slots, and the slots beyond the count are
              zeroed if the row was empty before or its count was clamped; every other byte stands.  So "not
              touched", "not written when nothing was admitted", "zeros beyond the count" and "only admitted
              survivors' slots are written" are all the same comparison.
  the refs    rows[s, slots[s, p]] is the model's element at position p.
  result()    equals the oracle's rows (oracle.DistinctRows, uncut, ascending by (h, words)),
              batch.distinct_segmented_rows_ordered over the whole streams and one ordered handle per stream.
"""
import ctypes as C

import numpy as np
import pytest
import segdistinct_rows_heap_ref as H
from hash_targets import MAX, MIN, plant, r01
from segdistinct_ref import _r01
from segdistinct_rows_ref import rows_of, uuid_hashcode_np
from test_gpu_segmented_distinct_ordered_state import _feed_cuts, _pieces
from test_gpu_segmented_distinct_rows_ordered import _case1, _differs, _id_rows, _oracle_rows, _reorder, _uuids

pytestmark = pytest.mark.gpu

FILL = -7  # what hashes and slots hold before the engine writes them
FILL_B = 0xA5  # and every byte of the row blocks


class Pair:
    """A SegmentedDistinctRowsOrdered, the model of its streams, and the expected bytes of its four tensors."""

    def __init__(self, cuda, oracle, S, k, W, seed, base=0, hash="default"):
        import torch

        from reservoir_amd import batch

        self.torch, self.cuda, self.k, self.S, self.W, self.hash = torch, cuda, k, S, W, hash
        self.st = st = batch.SegmentedDistinctRowsOrdered(S, k, W, seed, stream_base=base, hash=hash, device=cuda)
        assert st.rows.shape == (S, k, W) and st.rows.dtype == torch.uint8
        assert st.hashes.shape == (S, k) and st.hashes.dtype == torch.int64
        assert st.slots.shape == (S, k) and st.slots.dtype == torch.int32
        assert st.counts.shape == (S,) and st.counts.dtype == torch.int64 and not st.counts.any().item()
        st.rows.fill_(FILL_B)
        st.hashes.fill_(FILL)
        st.slots.fill_(FILL)
        r0, r1 = _r01(oracle, k, seed, base, S) if S else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        self.model = H.RowsHeapModel(S, k, W, r0, r1)
        self.exp = [np.full((S, k, W), FILL_B, np.uint8), np.full((S, k), FILL, np.int64),
                    np.full((S, k), FILL, np.int64), np.zeros(S, np.int64)]

    def hashed(self, rows, hashes):
        return hashes if hashes is not None else uuid_hashcode_np(rows)

    def expect(self, rows, offs, ids=None, hashes=None):
        """The model takes the launch; a row it admitted something into takes the model's arrays, the admitted
        survivors' rows in their slots, and zeros beyond its count where the engine owes them."""
        hashed = self.hashed(rows, hashes)
        er, eh, es, ec = self.exp
        for b in range(offs.size - 1):
            s = b if ids is None else int(ids[b])
            if not 0 <= s < self.S or offs[b + 1] <= offs[b]:
                continue
            owes_zeros = ec[s] <= 0 or ec[s] > self.k
            new = self.model.feed(s, rows[offs[b]:offs[b + 1]], hashed[offs[b]:offs[b + 1]])
            if not new:
                continue
            _, h, sl, n = self.model.state(s)
            eh[s], es[s], ec[s] = h, sl, n
            for row, slot in new.items():
                er[s, slot] = np.frombuffer(row, dtype=np.uint8)
            if owes_zeros:
                er[s, n:] = 0

    def launch(self, rows, offs, ids=None, hashes=None, check_ids=True):
        t = self.torch
        dev = lambda a: None if a is None else t.from_numpy(np.ascontiguousarray(a)).to(self.cuda)  # noqa: E731
        got = self.st.update(dev(rows), dev(offs), stream_ids=dev(ids), hashes=dev(hashes), check_ids=check_ids)
        assert got is self.st

    def state(self):
        st = self.st
        return [st.rows.cpu().numpy(), st.hashes.cpu().numpy(), st.slots.cpu().numpy().astype(np.int64),
                st.counts.cpu().numpy()]

    def check(self, what=""):
        got = self.state()
        assert np.array_equal(got[3], self.exp[3]), (what, np.flatnonzero(got[3] != self.exp[3])[:10])
        for g, e, name in zip(got, self.exp, ("rows", "hashes", "slots")):
            bad = np.flatnonzero((g != e).any(axis=tuple(range(1, g.ndim))))
            assert bad.size == 0, (what, name, bad[:10], g[bad[0]].reshape(-1)[:16], e[bad[0]].reshape(-1)[:16])
        # the references: the row of the entry at position p lies in slot slots[s, p]
        for s in range(self.S):
            mrows, mh, _ = self.model.arrays(s)
            n = mh.size
            if n and 0 < self.exp[3][s] <= self.k:
                assert np.array_equal(got[0][s][got[2][s, :n]], mrows), (what, "refs", s)

    def update(self, rows, offs, ids=None, hashes=None, check_ids=True, what=""):
        self.launch(rows, offs, ids, hashes, check_ids)
        self.expect(rows, offs, ids, hashes)
        self.check(what)

    def result(self):
        before = self.state()
        r = self.st.result()
        assert r[0].dtype == self.torch.uint8 and r[0].shape == (self.S, self.k, self.W)
        assert r[0].data_ptr() != self.st.rows.data_ptr() and r[1].data_ptr() != self.st.hashes.data_ptr()
        assert all(np.array_equal(a, b) for a, b in zip(before, self.state()))  # the state is left as it is
        return [x.cpu().numpy() for x in r]

    def check_result(self, want, what=""):
        got = self.result()
        for g, w, name in zip(got, want, ("rows", "hashes", "counts")):
            assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).any(axis=tuple(range(1, g.ndim))))[:10])


_REF = {}
_DECIDES = {}


def _case1_ref(cuda, oracle, k):
    """Case 1's input, the uncut oracle rows (equal to the stateless ordered launch), once per k."""
    import torch

    from reservoir_amd import batch

    if k not in _REF:
        rows, offs = _case1(k, 4 if k == 4096 else 12)
        want = _oracle_rows(oracle, rows, offs, k, 77)
        one = batch.distinct_segmented_rows_ordered(torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                                    seed=77, hash="default")
        one = [x.cpu().numpy() for x in one[:3]]
        assert all(np.array_equal(a, b) for a, b in zip(one, want))
        _REF[k] = rows, offs, want
    return _REF[k]


def _layout_decides(oracle, k, rows, offs):
    """From the CPU models alone, once per k: the first (stream, cut) pair at which a heap rebuilt from the sorted
    set ends with another set than the uncut run."""
    if k not in _DECIDES:
        r0, r1 = _r01(oracle, k, 77, 0, offs.size - 1)
        hashed = uuid_hashcode_np(rows)
        found = []
        for s in range(offs.size - 1):
            found = H.layout_decides(rows, offs[s:s + 2], k, r0[s:s + 1], r1[s:s + 1], hashed)
            if found:
                break
        _DECIDES[k] = found
    return _DECIDES[k]


@pytest.mark.parametrize("feed", ["one", "half", "cuts"])
@pytest.mark.parametrize("k", [1, 2, 5, 63, 64, 65, 511, 512, 513, 1024, 4096])
def test_cuts_over_every_size(cuda, oracle, k, feed):
    rows, offs, want = _case1_ref(cuda, oracle, k)
    if k >= 5:
        assert _layout_decides(oracle, k, rows, offs), "the input cannot tell a heap-array state from a sorted one"
    S = offs.size - 1
    lens = np.diff(offs)
    cuts = {"one": [[] for n in lens], "half": [[n // 2] for n in lens], "cuts": [_feed_cuts(int(n), k) for n in lens]}[feed]
    p = Pair(cuda, oracle, S, k, 16, 77)
    for j, (pr, po) in enumerate(_pieces(rows, offs, cuts)):
        p.update(pr, po, what=(feed, j))
    assert np.array_equal(p.exp[3], want[2])
    p.check_result(want, feed)


def test_result_is_the_oracle_the_stateless_launch_and_one_handle_per_stream(cuda, oracle):
    import torch

    from reservoir_amd import Sampler, batch

    k, seed, S = 64, 77, 12
    rows, offs, want = _case1_ref(cuda, oracle, k)
    p = Pair(cuda, oracle, S, k, 16, seed)
    handles = [Sampler.distinct(k, key_type="bytes16", seed=seed + s, order="ordered")() for s in range(S)]
    for pr, po in _pieces(rows, offs, [[n // 3, (2 * n) // 3] for n in np.diff(offs)]):
        p.update(pr, po)
        for s, d in enumerate(handles):
            d.sample_all(torch.from_numpy(pr[po[s]:po[s + 1]]).to(cuda))
    p.check_result(want)  # the uncut oracle
    gr, gh, gc = p.result()
    one = batch.distinct_segmented_rows_ordered(torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda), k, seed=seed)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip((gr, gh, gc), one[:3]))
    assert one[3].any().item()  # tied streams among them
    for s, d in enumerate(handles):
        held = np.asarray(d.result()).reshape(-1, 16)
        assert sorted(bytes(x) for x in held) == sorted(bytes(x) for x in gr[s, :gc[s]]), s


@pytest.mark.parametrize("width,k", [(24, 5), (64, 64), (256, 512)])
def test_wider_rows_precomputed_colliding_hashes(cuda, oracle, width, k):
    """Ids 0 .. 5k under id % (k // 2 + 1): fewer hash values than k, every full stream is tied, and every
    candidate meets members with its hash: rows are compared at words >= 2 between a state slot and an input row.
    The last two streams hold k - 2 and exactly k distinct rows: never tied.  3 pieces."""
    rng = np.random.default_rng(k)
    segs = []
    for s in range(8):
        d = rng.permutation(5 * k + 1) if s < 6 else rng.permutation(5 * k + 1)[:k - 2 if s == 6 else k]
        segs.append(np.r_[d, rng.choice(d, size=max(1, (3 * d.size) // 10))].astype(np.int64))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    ids = np.concatenate(segs)
    rows, hashed = rows_of(ids, width), ids % (k // 2 + 1)
    rows[:, :16] = rows_of(ids % 3, 16)  # the first two words are shared by a third of the rows
    assert np.unique(rows, axis=0).shape[0] == np.unique(ids).size
    want = _oracle_rows(oracle, rows, offs, k, 11, 3, hashes=hashed)
    assert np.array_equal(want[2], [k] * 6 + [k - 2, k])
    p = Pair(cuda, oracle, 8, k, width, 11, base=3, hash="precomputed")
    for pr, po, ph in _pieces(rows, offs, [[n // 3, (2 * n) // 3] for n in np.diff(offs)], hashed):
        p.update(pr, po, hashes=ph)
    p.check_result(want)


def test_repeats_and_equal_hashes(cuda, oracle):
    """k = 4, one stream, hashes planted at exact scrambled values.
    launch 1  A10 B20 C30 A10 D40 A10: a member offered twice in one launch
    launch 2  only members, other indices: nothing is admitted, nothing is written
    launch 3  A (equal bytes, another index); E at 20 -- B's hash, another row -- is admitted and evicts D; D again
              (evicted earlier in this launch) is refused by the new root 30; F at 5 evicts C; C again is refused"""
    k, seed = 4, 19
    ra = r01(oracle, seed)
    A, B, Cc, D, E, F = (_id_rows([i])[0] for i in (1, 2, 3, 4, 5, 6))
    p = Pair(cuda, oracle, 1, k, 16, seed, hash="precomputed")

    def go(rows, targets, what):
        rows = np.stack(rows)
        p.update(rows, np.array([0, rows.shape[0]], dtype=np.int64), hashes=plant(*ra, targets), what=what)

    go([A, B, Cc, A, D, A], [10, 20, 30, 10, 40, 10], "twice in one launch")
    assert p.exp[3][0] == 4 and sorted(p.exp[2][0].tolist()) == [0, 1, 2, 3]
    before = [x.copy() for x in p.exp]
    go([D, A, Cc, B, A], [40, 10, 30, 20, 10], "members only")
    assert all(np.array_equal(a, b) for a, b in zip(before, p.exp))
    slot_d = p.model.slot[0][D.tobytes()]
    slot_c = p.model.slot[0][Cc.tobytes()]
    go([A, E, D, F, Cc], [10, 20, 40, 5, 30], "evicted and offered again")
    held = set(p.model.rv[0].heap()[0])
    assert held == {A.tobytes(), B.tobytes(), E.tobytes(), F.tobytes()}
    assert p.model.slot[0][E.tobytes()] == slot_d and p.model.slot[0][F.tobytes()] == slot_c
    got = p.result()
    assert got[1][0].tolist() == [5, 10, 20, 20] and got[2][0] == 4


@pytest.mark.parametrize("how", ["reversed", "permuted"])
def test_arrival_order_across_a_cut(cuda, oracle, how):
    k = 64
    rows, offs, fwd = _case1_ref(cuda, oracle, k)
    rows = _reorder(rows, offs, how)
    want = _oracle_rows(oracle, rows, offs, k, 77)
    assert _differs(want, fwd).any()  # the order decides the set
    p = Pair(cuda, oracle, offs.size - 1, k, 16, 77)
    for pr, po in _pieces(rows, offs, [[n // 3, (2 * n) // 3] for n in np.diff(offs)]):
        p.update(pr, po)
    p.check_result(want)
    fwd_state = Pair(cuda, oracle, offs.size - 1, k, 16, 77)
    fwd_rows = _case1_ref(cuda, oracle, k)[0]
    fwd_state.expect(fwd_rows, offs)
    assert any(not np.array_equal(a, b) for a, b in zip(fwd_state.exp, p.exp))  # the model's other state


@pytest.mark.parametrize("k", [1, 64])
def test_hash_edges(cuda, oracle, k):
    """Row 0: h = INT64_MIN into an empty row is admitted; at k = 1 the row is then full with the root INT64_MIN,
    admits nothing and is not written; at k = 64 it fills up with INT64_MAX as the root, a second row at INT64_MAX
    is refused and a smaller hash evicts the root.  Row 1: k rows at INT64_MIN, then anything: nothing admitted."""
    seed = 31
    r = [r01(oracle, seed + s) for s in range(2)]
    rng = np.random.default_rng(k)
    p = Pair(cuda, oracle, 2, k, 16, seed, hash="precomputed")

    def go(ids0, t0, ids1, t1, what):
        rows = _id_rows(list(ids0) + list(ids1))
        offs = np.array([0, len(ids0), len(ids0) + len(ids1)], dtype=np.int64)
        p.update(rows, offs, hashes=np.r_[plant(*r[0], t0), plant(*r[1], t1)].astype(np.int64), what=what)

    go([100], [MIN], range(200, 200 + k), [MIN] * k, "MIN into an empty row")
    assert p.exp[3].tolist() == [1, k] and p.exp[1][0, 0] == MIN and (p.exp[1][1] == MIN).all()
    before = [x.copy() for x in p.exp]
    if k == 1:
        go([101, 100, 102], [MIN, MIN, MIN + 1], [300, 200], [MIN, MIN], "a root at MIN admits nothing")
        assert all(np.array_equal(a, b) for a, b in zip(before, p.exp))
        return
    mid = [int(x) for x in rng.integers(-2**62, 2**62, size=k - 3)]
    go(range(101, 100 + k), mid + [MAX - 1, MAX], [300, 301], [MIN, MIN + 1], "fills up, MAX at the root")
    assert p.exp[3].tolist() == [k, k] and p.exp[1][0, 0] == MAX
    assert np.array_equal(before[1][1], p.exp[1][1])  # row 1 was not written
    go([900], [MAX], [], [], "MAX < MAX fails")
    assert p.exp[1][0, 0] == MAX
    go([901, 100 + k - 1], [5, MAX], [], [], "a smaller hash evicts MAX, and MAX is refused again")
    assert p.exp[1][0, 0] == MAX - 1 and p.exp[3][0] == k
    assert 901 in p.result()[0][0].view(np.uint64).reshape(k, 2)[:, 0]


def test_rows_base_at_8_mod_16_and_int64_rows(cuda, oracle):
    """rows_dev one word into an allocation (a UUID is two 8-byte loads), and 16-byte aligned; the rows given as
    int64 (n, width / 8)."""
    import torch

    k = 64
    rows, offs, want = _case1_ref(cuda, oracle, k)
    lens = np.diff(offs)
    for off8 in (1, 0):
        p = Pair(cuda, oracle, offs.size - 1, k, 16, 77)
        for pr, po in _pieces(rows, offs, [[n // 2] for n in lens]):
            words = torch.from_numpy(np.ascontiguousarray(pr).view(np.int64).reshape(-1))
            shifted = torch.empty(words.numel() + 3, dtype=torch.int64, device=cuda)
            base = 1 if (shifted.data_ptr() % 16 == 0) == bool(off8) else 2
            shifted[base:base + words.numel()] = words.to(cuda)
            rd = shifted[base:base + words.numel()].view(-1, 2)  # int64 rows
            assert rd.data_ptr() % 16 == 8 * off8 and rd.dtype == torch.int64
            assert p.st.update(rd, torch.from_numpy(po).to(cuda)) is p.st
            p.expect(pr, po)
            p.check(off8)
        p.check_result(want)


def _small(S, k, seed=5):
    """S streams of up to 4 UUIDs per hashCode (case 1's recipe), 6k rows each."""
    rng = np.random.default_rng(seed)
    return [_uuids(rng.integers(0, 4, 6 * k), rng.integers(0, k + 3, 6 * k), s) for s in range(S)]


def test_stream_ids_and_rows_left_alone(cuda, oracle):
    """A subset of the rows in a shuffled order; an id outside [0, S) with check_ids=False is skipped; rows nobody
    names and rows with an empty segment keep the fill (Pair.check compares every byte)."""
    S, k = 9, 5
    segs = _small(S, k)  # 30 rows each
    p = Pair(cuda, oracle, S, k, 16, 21, base=2)
    fed = [np.zeros((0, 16), np.uint8) for _ in range(S)]

    def go(ids, parts, **kw):
        offs = np.r_[0, np.cumsum([x.shape[0] for x in parts])].astype(np.int64)
        p.update(np.concatenate(parts), offs, ids=np.array(ids, dtype=np.int64), **kw)
        for r, x in zip(ids, parts):
            if 0 <= r < S:
                fed[r] = np.concatenate([fed[r], x])

    go([6, 1, 8, 3, 0], [segs[6][:20], segs[1][:0], segs[8][:13], segs[3][:0], segs[0][:25]], what="subset")
    assert [int(c > 0) for c in p.exp[3]] == [1, 0, 0, 0, 0, 0, 1, 0, 1]
    got = p.state()
    assert (got[0][[1, 2, 3, 4, 5, 7]] == FILL_B).all() and (got[2][[1, 2, 3, 4, 5, 7]] == FILL).all()
    # the second pieces, other rows and another order; one id behind the state, one negative
    go([3, S, 6, -1, 8, 2], [segs[3][:11], segs[0][:9], segs[6][20:], segs[1][:4], segs[8][:0], segs[2][:3]],
       check_ids=False, what="outside")
    assert [int(c > 0) for c in p.exp[3]] == [1, 0, 1, 1, 0, 0, 1, 0, 1]
    assert (p.state()[0][[1, 4, 5, 7]] == FILL_B).all()
    woffs = np.r_[0, np.cumsum([x.shape[0] for x in fed])].astype(np.int64)
    p.check_result(_oracle_rows(oracle, np.concatenate(fed), woffs, k, 21, 2))
    with pytest.raises(Exception) as e:
        p.launch(np.concatenate([segs[0][:2], segs[1][:2]]), np.array([0, 2, 4], dtype=np.int64),
                 ids=np.array([4, 4], dtype=np.int64))
    from reservoir_amd import IllegalArgumentException

    assert isinstance(e.value, IllegalArgumentException)
    p.check("duplicate ids raise before the launch")


def test_no_segments_and_no_rows(cuda, oracle):
    import torch

    p = Pair(cuda, oracle, 3, 4, 16, 1)
    p.update(np.zeros((0, 16), dtype=np.uint8), np.zeros(1, dtype=np.int64))  # num_segments == 0
    p.update(np.zeros((0, 16), dtype=np.uint8), np.zeros(4, dtype=np.int64))  # three empty segments
    assert not p.exp[3].any()
    r = p.result()  # a state fed nothing: all empty
    assert not r[0].any() and not r[1].any() and not r[2].any()
    z = Pair(cuda, oracle, 0, 4, 16, 1)  # S == 0
    z.update(np.zeros((0, 16), dtype=np.uint8), np.zeros(1, dtype=np.int64))
    z.update(_id_rows(range(6)), np.array([0, 2, 6], dtype=np.int64), ids=np.array([0, 1], dtype=np.int64), check_ids=False)
    r = z.st.result()
    assert r[0].shape == (0, 4, 16) and r[1].shape == (0, 4) and r[2].shape == (0,)
    torch.cuda.synchronize()


def test_clamps_never_leave_the_state(cuda, oracle):
    """The four tensors are views into larger buffers with guard bands of k rows / k entries of a pattern on both
    sides.  Counts of -3 and k + 5, slots in [k, 2k), in [-k, -1] and repeated: the launch returns, every guard
    byte stands, the counts end in [0, k]; the two rows with only a bad count behave as the empty row and as a row of
    k entries.  (Unclamped, every planted value would still land inside a guard band or a neighbouring row.)"""
    import torch

    S, k, W = 7, 64, 16
    segs = _small(S, k, seed=9)
    p = Pair(cuda, oracle, S, k, W, 15)
    st = p.st
    guard = {}
    for name, per in (("rows", k * W), ("hashes", k), ("slots", k), ("counts", 1)):
        t = getattr(st, name)
        g = k * W if name == "rows" else k
        big = torch.empty(g + S * per + g, dtype=t.dtype, device=cuda)
        big.fill_(0x5C if name == "rows" else -12345)
        view = big[g:g + S * per].view(t.shape)
        view.copy_(t)
        setattr(st, name, view)
        guard[name] = (big, g, S * per, big.clone())
    assert st.rows.data_ptr() % 8 == 0
    rows1 = np.concatenate([x[:3 * k] for x in segs])
    offs1 = np.arange(0, S * 3 * k + 1, 3 * k, dtype=np.int64)
    p.update(rows1, offs1)
    assert p.exp[3].tolist() == [k] * S
    st.counts[0] = k + 5
    st.counts[1] = -3
    st.slots[2, ::2] += k  # [k, 2k)
    st.slots[3, 1::3] -= k  # [-k, -1]
    st.slots[4] = 0  # repeats
    st.slots[5, :] = torch.arange(k, 2 * k, dtype=torch.int32, device=cuda)
    st.counts[5] = k + 5
    torch.cuda.synchronize()
    rows2 = np.concatenate([x[3 * k:] for x in segs])
    offs2 = np.r_[0, np.cumsum([x.shape[0] - 3 * k for x in segs])].astype(np.int64)
    p.launch(rows2, offs2)
    torch.cuda.synchronize()
    for name, (big, g, n, was) in guard.items():
        assert torch.equal(big[:g], was[:g]) and torch.equal(big[g + n:], was[g + n:]), name
    counts = st.counts.cpu().numpy()
    assert ((counts >= 0) & (counts <= k)).all() and counts[[0, 1, 6]].tolist() == [k, k, k]
    slots = st.slots.cpu().numpy()
    assert ((slots[[0, 1, 6]] >= 0) & (slots[[0, 1, 6]] < k)).all()
    r = [x.cpu().numpy() for x in st.result()]
    torch.cuda.synchronize()
    # row 0 went on as a row of k entries, row 1 as the empty sampler (seeded 15 + 1, fed the second piece only),
    # row 6 was left alone by the planting
    for s, fed in [(0, segs[0]), (1, segs[1][3 * k:]), (6, segs[6])]:
        w = _oracle_rows(oracle, fed, np.array([0, fed.shape[0]], dtype=np.int64), k, 15 + s)
        assert np.array_equal(r[0][s], w[0][0]) and np.array_equal(r[1][s], w[1][0]) and r[2][s] == w[2][0], s
    # row 1 was taken as empty and filled up again: its slots are the rule's permutation from an empty row
    assert sorted(slots[1].tolist()) == list(range(k))


def test_a_row_that_admits_nothing_is_not_written(cuda, oracle):
    """A partial row with sentinels beyond its count in all three per-slot tensors, fed only repeats of its members:
    the sentinels survive.  When it then admits one new row, hashes and slots get zeros beyond the count, and the row
    slots beyond it keep what they had (the row was not empty and its count was in range)."""
    S, k = 2, 8
    p = Pair(cuda, oracle, S, k, 16, 3)
    first = _id_rows([11, 12, 13])
    p.update(first, np.array([0, 3, 3], dtype=np.int64))
    assert p.exp[3].tolist() == [3, 0] and not p.exp[0][0, 3:].any() and not p.exp[1][0, 3:].any()
    p.st.rows[0, 3:] = 0x99
    p.st.hashes[0, 3:] = -98
    p.st.slots[0, 3:] = -97
    p.exp[0][0, 3:], p.exp[1][0, 3:], p.exp[2][0, 3:] = 0x99, -98, -97
    p.update(np.concatenate([first[::-1], first]), np.array([0, 6, 6], dtype=np.int64), what="repeats")
    assert (p.state()[0][0, 3:] == 0x99).all() and (p.state()[1][0, 3:] == -98).all()
    p.update(_id_rows([12, 14]), np.array([0, 2, 2], dtype=np.int64), what="one new row")
    got = p.state()
    assert got[3][0] == 4 and not got[1][0, 4:].any() and not got[2][0, 4:].any()
    assert (got[0][0, 4:] == 0x99).all() and np.array_equal(got[0][0, 3], _id_rows([14])[0])


def test_bad_arguments_raise_what_the_set_state_raises(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch
    from reservoir_amd import _native as N

    new, ref = batch.SegmentedDistinctRowsOrdered, batch.SegmentedDistinctRows
    ctor = [
        (IllegalArgumentException, lambda c: c(4, 0, 16, 1, device=cuda)),
        (ReservoirError, lambda c: c(4, 4097, 16, 1, device=cuda)),
        (IllegalArgumentException, lambda c: c(4, 4, 16, 1, hash="md5", device=cuda)),
        (IllegalArgumentException, lambda c: c(-1, 4, 16, 1, device=cuda)),
        (IllegalArgumentException, lambda c: c(4, 4, 12, 1, device=cuda)),
        (IllegalArgumentException, lambda c: c(4, 4, 264, 1, hash="precomputed", device=cuda)),
        (ReservoirError, lambda c: c(4, 4, 8, 1, device=cuda)),
        (ReservoirError, lambda c: c(4, 4, 24, 1, device=cuda)),  # hash="default" is width 16 only
        (IllegalArgumentException, lambda c: c(4, 4, 16, 1, device="cpu")),
    ]
    for exc, make in ctor:
        msgs = []
        for c in (new, ref):
            with pytest.raises(exc) as e:
                make(c)
            msgs.append(str(e.value).replace(c._NAME, "X").replace(c._LONG, "Y"))
        assert msgs[0] == msgs[1], msgs
    with pytest.raises(ReservoirError, match="SegmentedDistinctRowsOrdered takes byte keys; SegmentedDistinctOrdered takes"):
        new(4, 4, 8, 1, device=cuda)
    sd, rf = new(2, 4, 16, 1, device=cuda), ref(2, 4, 16, 1, device=cuda)
    rows = torch.zeros((10, 16), dtype=torch.uint8, device=cuda)
    offs = torch.tensor([0, 3, 6, 10], dtype=torch.int64, device=cuda)
    ids = lambda *a: torch.tensor(a, dtype=torch.int64, device=cuda)  # noqa: E731
    calls = [
        (IllegalArgumentException, lambda s: s.update(rows.cpu(), offs)),
        (IllegalArgumentException, lambda s: s.update(rows.view(-1), offs)),  # 1-D rows
        (IllegalArgumentException, lambda s: s.update(rows.to(torch.int32), offs)),
        (IllegalArgumentException, lambda s: s.update(torch.zeros((10, 24), dtype=torch.uint8, device=cuda), offs)),
        (IllegalArgumentException, lambda s: s.update(rows, offs.to(torch.int32))),
        (IllegalArgumentException, lambda s: s.update(rows, offs)),  # three segments, two rows, no ids
        (IllegalArgumentException, lambda s: s.update(rows, offs[:3], hashes=torch.zeros(10, dtype=torch.int64, device=cuda))),
        (IllegalArgumentException, lambda s: s.update(rows, offs, stream_ids=ids(0, 1, 0))),
        (IllegalArgumentException, lambda s: s.update(rows, offs, stream_ids=ids(0, 1, 2))),
        (IllegalArgumentException, lambda s: s.update(rows, offs, stream_ids=ids(0, -1, 1))),
        (IllegalArgumentException, lambda s: s.update(rows, offs, stream_ids=ids(0, 1))),
    ]
    for exc, call in calls:
        msgs = []
        for s in (sd, rf):
            with pytest.raises(exc) as e:
                call(s)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    with pytest.raises(NullPointerException):
        new(2, 4, 16, 1, hash="precomputed", device=cuda).update(rows, offs[:3])
    torch.cuda.synchronize()
    assert not sd.counts.any().item()
    vp = C.c_void_p
    with pytest.raises(NullPointerException, match="state_slots_dev"):
        N.check(N.load().rsv_distinct_segmented_rows_ordered_update(
            vp(rows.data_ptr()), None, vp(offs.data_ptr()), None, 1, 2, 16, 4, N.HASH_DEFAULT, 1, 0,
            vp(sd.rows.data_ptr()), vp(sd.hashes.data_ptr()), None, vp(sd.counts.data_ptr()), None))


def test_merge_raises(cuda):
    from reservoir_amd import ReservoirError, batch

    sd = batch.SegmentedDistinctRowsOrdered(2, 4, 16, 1, device=cuda)
    with pytest.raises(ReservoirError, match="SegmentedDistinctRows.merge"):
        sd.merge(sd)
    with pytest.raises(ReservoirError, match="SegmentedDistinctRows.merge"):
        sd.merge(sd.rows, sd.hashes, sd.counts)
