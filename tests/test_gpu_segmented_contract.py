"""What the members of the segmented Sampler.apply family (K2) share, on the smallest shapes that reach
each shared piece: the segment header of the four update kernels (empty segments, ids outside [0, S) and
negative bases are skipped), the stateless slot rule (last writer, else the stream's own element j, else
zero) in both forms, the merge's largest-idx-per-slot pick, and the argument checks the four state
classes of batch.py have in common (K5's two included), with their exception types and message texts.

Long keys (int64) and byte rows of W = 24 (8-byte granules: every other row is off a 16-byte boundary).
Every expected slot comes from oracle.algo_r_last_writers; the merge's from the rule itself (per slot the
largest idx, next the max), computed over the planted tensors with numpy."""
import functools

import numpy as np
import pytest

import test_gpu_segmented_rows as TR  # _rows: every 8-byte word of every row distinct, and _expect

pytestmark = pytest.mark.gpu

SEED, BASE, W = 31, 2**33 + 5, 24
KINDS = ["keys", "rows"]
CAN_K, CAN_I, CAN_N = 0x5A, 2**40 + 3, 2**41 + 9  # canaries: payload byte, idx, next


def _payload(kind, n):
    """n elements: distinct int64 keys, or rows of W bytes"""
    if kind == "rows":
        return TR._rows(n, W)
    return (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)


def _state(batch, kind, S, k, cuda, dtype=None):
    if kind == "rows":
        return batch.SegmentedSamplerRows(S, k, W, SEED, BASE, device=cuda)
    return batch.SegmentedSampler(S, k, SEED, BASE, device=cuda)


def _payload_of(st):
    return st.rows if hasattr(st, "rows") else st.keys


def _bytes(t):
    """a payload tensor as numpy bytes, one row of bytes per slot"""
    a = t.cpu().numpy()
    return a.view(np.uint8).reshape(a.shape[:2] + (-1,)) if a.dtype != np.uint8 else a


# ---- the four update kernels: one segment header ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def _update_case(k):
    """Six segments for S = 6 rows: (id, base, len).  Rows 2 and 5 are fed; 0 (empty segment) and 4
    (negative base) are named but skipped; ids -1 and S name no row; rows 1 and 3 are not named."""
    from oracle import oracle

    S = 6
    segs = [(2, 0, 3 * k + 100), (-1, 0, 20), (0, 0, 0), (S, 0, 20), (4, -1, 20), (5, 7, k + 300)]
    lens = np.array([s[2] for s in segs], dtype=np.int64)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    widx = {r: oracle.algo_r_last_writers(SEED, BASE + r, k, n0, n, 1) for r, n0, n in (segs[0], segs[5])}
    return S, segs, offs, widx


@pytest.mark.parametrize("k", [5, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_update_segment_header(cuda, oracle, kind, k):
    """k = 5: the wave form, k = 512: the workgroup form.  The fed rows end as the oracle says (row 5
    from base 7: above k = 5, inside the fill range of k = 512); every other row keeps its canaries bit
    for bit in all three tensors, and so do the fed rows' slots without a writer."""
    import torch

    from reservoir_amd import batch

    S, segs, offs, widx = _update_case(k)
    data = _payload(kind, int(offs[-1]))
    st = _state(batch, kind, S, k, cuda)
    pay = _payload_of(st)
    pay.view(torch.uint8).fill_(CAN_K)
    fed = sorted(widx)
    rest = [r for r in range(S) if r not in fed]
    st.idx[rest] = CAN_I
    st.next[rest] = CAN_N
    before = (pay.clone(), st.idx.clone(), st.next.clone())
    ids = TR._dev(torch, cuda, np.array([s[0] for s in segs], dtype=np.int64))
    bases = TR._dev(torch, cuda, np.array([s[1] for s in segs], dtype=np.int64))
    assert st.update(TR._dev(torch, cuda, data), TR._dev(torch, cuda, offs), stream_ids=ids, bases=bases,
                     check_ids=False) is st
    got, idx, nxt = _bytes(pay), st.idx.cpu().numpy(), st.next.cpu().numpy()
    was = _bytes(before[0])
    for b, (r, n0, n) in enumerate(segs):
        if r not in widx:
            continue
        w = widx[r]
        assert np.array_equal(idx[r], w), (kind, k, r)
        assert nxt[r] == n0 + n
        src = data[offs[b] + np.where(w >= 0, w - n0, 0)]
        want = np.where((w >= 0)[:, None], np.ascontiguousarray(src).view(np.uint8).reshape(k, -1), CAN_K)
        assert np.array_equal(got[r], want), (kind, k, r)
    assert (widx[5] >= 0).any() and (k < 512 or (widx[5] < 0).any())  # k = 512: a fed row has canary slots
    assert np.array_equal(got[rest], was[rest])
    assert torch.equal(st.idx[rest], before[1][rest]) and torch.equal(st.next[rest], before[2][rest])


# ---- the stateless kernels: one slot rule ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stateless_case(k):
    from oracle import oracle

    lens = np.array([0, 1, max(k - 1, 0), k, k + 1, 3 * k + 1, 3 * k + 17, 2, k // 2 + 1], dtype=np.int64)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    widx = TR.LK._last_writers(oracle, SEED, BASE, k, lens)
    for a in (lens, offs, widx):
        a.setflags(write=False)
    return lens, offs, widx


@pytest.mark.parametrize("k", [1, 64, 65, 511, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_stateless_slot_rule(cuda, oracle, kind, k):
    """S = 9 streams of 0, 1, k - 1, k, k + 1 and about 3k elements: slots no draw hit hold the stream's
    own element j, slots at and beyond the count are zero; k = 64 | 65 and 511 | 512 are the borders of
    the deferred gather and of the workgroup form."""
    import torch

    from reservoir_amd import batch

    lens, offs, widx = _stateless_case(k)
    data = _payload(kind, int(offs[-1]))
    fn = batch.sample_segmented_rows if kind == "rows" else batch.sample_segmented
    out, cnt = fn(TR._dev(torch, cuda, data), TR._dev(torch, cuda, offs), k, SEED, BASE)
    assert np.array_equal(cnt.cpu().numpy(), np.minimum(lens, k))
    want = TR._expect(np.ascontiguousarray(data).view(np.uint8).reshape(data.shape[0], -1), offs, widx)
    assert np.array_equal(_bytes(out), want), (kind, k)
    assert not _bytes(out)[widx < 0].any()


# ---- merge: one pick -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_merge_pick(cuda, kind):
    """P = 3 parts of S = 4 rows, k = 7.  Row 0 plants a slot the state wins, one per part, and one that
    is empty everywhere; the other slots hold distinct random indices.  A winning part moves its payload
    and idx, a losing one nothing; next becomes the max; merging the result into itself changes nothing."""
    import torch

    from reservoir_amd import batch

    P, S, k = 3, 4, 7
    rng = np.random.default_rng(77)
    allidx = rng.permutation(10_000)[:(P + 1) * S * k].reshape(P + 1, S, k).astype(np.int64)
    allidx[:, 0, 0] = [100, 3, -1, 50]   # the state wins
    allidx[:, 0, 1] = [5, 900, 7, -1]    # part 0
    allidx[:, 0, 2] = [-1, 1, 901, 2]    # part 1
    allidx[:, 0, 3] = [8, 9, 10, 902]    # part 2
    allidx[:, 0, 4] = -1                 # empty everywhere
    allnext = rng.integers(0, 20_000, size=(P + 1, S)).astype(np.int64)
    allnext[:, 1] = [700, 3, 5, 9]       # the state's next is the largest
    data = _payload(kind, (P + 1) * S * k)
    allpay = np.ascontiguousarray(data).view(np.uint8).reshape(P + 1, S, k, -1)
    win = allidx.argmax(0)               # the indices are distinct, or all -1 (argmax: the state)
    want_pay = np.take_along_axis(allpay, win[None, :, :, None], 0)[0]
    st = _state(batch, kind, S, k, cuda)
    pay = _payload_of(st)
    pay.view(torch.uint8).copy_(TR._dev(torch, cuda, allpay[0]).view(pay.view(torch.uint8).shape))
    st.idx.copy_(TR._dev(torch, cuda, allidx[0]))
    st.next.copy_(TR._dev(torch, cuda, allnext[0]))
    parts = TR._dev(torch, cuda, allpay[1:]).view(pay.dtype).view((P,) + tuple(pay.shape))
    assert st.merge(parts, TR._dev(torch, cuda, allidx[1:]), TR._dev(torch, cuda, allnext[1:])) is st
    assert win[0, :5].tolist() == [0, 1, 2, 3, 0]
    assert np.array_equal(st.idx.cpu().numpy(), allidx.max(0))
    assert np.array_equal(st.next.cpu().numpy(), allnext.max(0))
    assert np.array_equal(_bytes(pay), want_pay), kind
    snap = (pay.clone(), st.idx.clone(), st.next.clone())
    assert st.merge(st) is st
    for now, was in zip((pay, st.idx, st.next), snap):
        assert torch.equal(now, was)


# ---- the four state classes: one set of argument checks --------------------------------------------

CLASSES = {  # name: (extra constructor arguments after k, k's cap, payload, side tensors, merge's identity)
    "SegmentedDistinct": ((), 4096, "keys", "hashes and counts", "seed, stream_base and hash"),
    "SegmentedDistinctRows": ((16,), 4096, "rows", "hashes and counts", "width, seed, stream_base and hash"),
    "SegmentedSampler": ((), 15104, "keys", "idx and next", "seed and stream_base"),
    "SegmentedSamplerRows": ((16,), 15104, "rows", "idx and next", "width, seed and stream_base"),
}
MSG_OFFSETS_DTYPE = {
    "SegmentedDistinct": "keys must have the state's dtype and offsets must be int64",
    "SegmentedDistinctRows": "rows must be 2-D (one key per row) and offsets int64",
    "SegmentedSampler": "keys must have the state's dtype and offsets must be int64",
    "SegmentedSamplerRows": "rows must be 2-D uint8 or int64 (one key per row) and offsets int64",
}
MSG_PART_DTYPE = {
    "SegmentedDistinct": "part keys must have the state's dtype, hashes and counts must be int64",
    "SegmentedDistinctRows": "part rows must be uint8, hashes and counts int64",
    "SegmentedSampler": "part keys must have the state's dtype, idx and next must be int64",
    "SegmentedSamplerRows": "part rows must be uint8, idx and next int64",
}
MSG_IDS = "stream_ids must be an int64 device tensor, one per segment"


def _raises(exc, msg, fn, *a, **kw):
    with pytest.raises(exc) as e:
        fn(*a, **kw)
    assert type(e.value) is exc and str(e.value) == msg


def _class_case(torch, batch, name, cuda, seed=1):
    """a 4 x 8 state of the class, and an update's (payload, offsets): two segments of 4 and 6 elements"""
    extra = CLASSES[name][0]
    st = getattr(batch, name)(4, 8, *extra, seed, device=cuda)
    offs = torch.tensor([0, 4, 10], device=cuda)
    if extra:
        return st, torch.arange(160, device=cuda).to(torch.uint8).view(10, 16), offs
    return st, torch.arange(10, device=cuda), offs


@pytest.mark.parametrize("name", list(CLASSES))
def test_state_class_arguments(cuda, name):
    import torch

    from reservoir_amd import batch
    from reservoir_amd import _native as N

    cls = getattr(batch, name)
    extra, cap, payload, sides, ident = CLASSES[name]
    IAE = N.IllegalArgumentException
    _raises(IAE, "negative stream count", cls, -1, 8, *extra, 1, device=cuda)
    _raises(IAE, "k out of range", cls, 4, 0, *extra, 1, device=cuda)
    _raises(N.ReservoirError, f"{name} holds k <= {cap} per stream; use separate handles beyond",
            cls, 4, cap + 1, *extra, 1, device=cuda)
    _raises(IAE, "the state lives on the device", cls, 4, 8, *extra, 1, device="cpu")
    st, data, offs = _class_case(torch, batch, name, cuda)
    _raises(IAE, f"{payload} and offsets must be device tensors", st.update, data.cpu(), offs)
    _raises(IAE, MSG_OFFSETS_DTYPE[name], st.update, data, offs.to(torch.int32))
    _raises(IAE, MSG_IDS, st.update, data, offs, stream_ids=torch.tensor([0, 1], dtype=torch.int32, device=cuda))
    _raises(IAE, MSG_IDS, st.update, data, offs, stream_ids=torch.tensor([0], device=cuda))
    _raises(IAE, MSG_IDS, st.update, data, offs, stream_ids=torch.tensor([0, 1]))
    _raises(IAE, "stream_ids repeat a row within one update", st.update, data, offs,
            stream_ids=torch.tensor([1, 1], device=cuda))
    _raises(IAE, "stream_ids outside [0, 4)", st.update, data, offs, stream_ids=torch.tensor([0, 4], device=cuda))
    three = [getattr(st, payload)] + [getattr(st, n) for n in sides.split(" and ")]
    _raises(N.NullPointerException, f"merge needs part_{payload}, part_{sides.replace(' and ', ' and part_')}",
            st.merge, three[0])
    _raises(IAE, f"merge needs states of the same shape, {ident}", st.merge,
            _class_case(torch, batch, name, cuda, seed=2)[0])
    shape = "(P, 4, 8, 16), (P, 4, 8), (P, 4)" if extra else "(P, 4, 8), (P, 4, 8), (P, 4)"
    _raises(IAE, f"parts must be shaped {shape}", st.merge, three[0][:, :4], three[1][:, :4], three[2])
    _raises(IAE, f"parts must be shaped {shape}", st.merge, three[0], three[1], three[2][:3])
    _raises(IAE, MSG_PART_DTYPE[name], st.merge, three[0], three[1].to(torch.int32), three[2])
    # and the calls that pass: no segment, one part as tensors, itself as an object
    assert st.update(data[:0], offs[:1]) is st
    assert st.update(data, offs, stream_ids=torch.tensor([3, 1], device=cuda)) is st
    assert st.merge(*three) is st and st.merge(st) is st
    assert st.counts.tolist() == [0, 6, 0, 4]


@pytest.mark.parametrize("name", list(CLASSES))
def test_state_class_other_device(cuda, name):
    import torch

    from reservoir_amd import batch
    from reservoir_amd import _native as N

    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    st, data, offs = _class_case(torch, batch, name, cuda)
    other = torch.device("cuda", 1)
    payload = CLASSES[name][2]
    _raises(N.IllegalArgumentException, f"{payload} and offsets must live on the state's device", st.update,
            data.to(other), offs.to(other))
    three = [getattr(st, payload).to(other)] + [getattr(st, n).to(other) for n in CLASSES[name][3].split(" and ")]
    _raises(N.IllegalArgumentException, "parts must live on the state's device", st.merge, *three)
