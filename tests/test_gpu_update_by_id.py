"""update_by_id of the caller-held states: ids in arrival order in, the states advanced, no host grouping.

A feed is three micro-batches of about 5000 interleaved elements over S = 37 or S = 5000 rows with gaps (rows the
feed never names), skewed so that the busiest row sees more than 512 elements, with a few ids outside [0, S) that
are dropped.  The element samplers are compared after EVERY batch with a second state fed the same batch grouped on
the host (numpy stable sort, compact offsets + stream_ids, the existing update), bit for bit over keys / rows, idx and
next, and after the last batch with the oracle's last writers over each row's whole stream.  The distinct states are
compared with the existing update on host-grouped input; the ordered one, under a colliding hash, with
values.RandomValues fed each row's elements in arrival order, in array order -- the check an unstable grouping fails.
"""
import ctypes as C

import numpy as np
import pytest
import segdistinct_heap_ref as H
from segdistinct_ref import _r01

pytestmark = pytest.mark.gpu

FILL = -7
SEED, BASE = 0xC0FFEE, 5
_FEEDS = {}


def _feed(S):
    """Three batches of ids (int64, arrival order) over S rows: half the rows never named, a skewed choice among
    the others, and some ids outside [0, S).  Once per S."""
    if S not in _FEEDS:
        rng = np.random.default_rng(S)
        present = np.sort(rng.choice(S, size=max(2, S // 2), replace=False))
        w = 1.0 / (1.0 + np.arange(present.size)) ** 1.1
        w[0] += 0.35 * w.sum()  # the busiest row: more than 512 elements over the feed
        batches = []
        for b, n in enumerate((5003, 4999, 5120)):
            ids = present[rng.choice(present.size, size=n, p=w / w.sum())].astype(np.int64)
            bad = rng.choice(n, size=40, replace=False)
            ids[bad] = rng.choice(np.array([-1, S, S + 7, np.iinfo(np.int64).min, np.iinfo(np.int64).max]), size=40)
            batches.append(ids)
        _FEEDS[S] = present, batches
    return _FEEDS[S]


def _host_group(ids, S):
    """The batch grouped on the host: (positions in grouped order, compact offsets, the rows present)."""
    keep = np.flatnonzero((ids >= 0) & (ids < S))
    pos = keep[np.argsort(ids[keep], kind="stable")]
    rows, counts = np.unique(ids[pos], return_counts=True)
    return pos, np.r_[0, np.cumsum(counts)].astype(np.int64), rows.astype(np.int64)


def _dev(cuda, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(a, b, what):
    for x, y, name in zip(a._state(), b._state(), a._TENSORS):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(x, y), (what, name, np.argwhere(x != y)[:5])


def _streams(ids_batches, payload_batches, S):
    """Each row's whole stream, in arrival order."""
    ids, payload = np.concatenate(ids_batches), np.concatenate(payload_batches)
    return {int(r): payload[ids == r] for r in np.unique(ids) if 0 <= r < S}


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
@pytest.mark.parametrize("k", [1, 64, 512])
@pytest.mark.parametrize("S", [37, 5000])
def test_sampler_by_id(cuda, oracle, S, k, dtype):
    import torch

    from reservoir_amd import batch

    present, batches = _feed(S)
    rng = np.random.default_rng(k)
    info = np.iinfo(dtype)
    tdt = torch.int32 if dtype == np.int32 else torch.int64
    got = batch.SegmentedSampler(S, k, SEED, stream_base=BASE, dtype=tdt, device=cuda)
    ref = batch.SegmentedSampler(S, k, SEED, stream_base=BASE, dtype=tdt, device=cuda)
    got.keys.fill_(FILL)
    ref.keys.fill_(FILL)
    fed = []
    for b, ids in enumerate(batches):
        keys = rng.integers(info.min, info.max, size=ids.size, dtype=dtype)
        fed.append(keys)
        ids_dev = _dev(cuda, ids if b != 1 else ids.clip(-2**31, 2**31 - 1).astype(np.int32))  # int32 ids too
        assert got.update_by_id(_dev(cuda, keys), ids_dev) is got
        pos, offs, rows = _host_group(ids, S)
        ref.update(_dev(cuda, keys[pos]), _dev(cuda, offs), stream_ids=_dev(cuda, rows))
        _same(got, ref, b)
    streams = _streams(batches, fed, S)
    keys_out, idx, nxt = (t.cpu().numpy() for t in got._state())
    assert len(streams[int(present[0])]) > 512
    for r in range(S):
        st = streams.get(r)
        if st is None:  # a gap: never touched
            assert nxt[r] == 0 and (idx[r] == -1).all() and (keys_out[r] == FILL).all(), r
            continue
        lw = oracle.algo_r_last_writers(SEED, BASE + r, k, 0, st.size)
        assert nxt[r] == st.size and np.array_equal(idx[r], lw), r
        assert np.array_equal(keys_out[r][lw >= 0], st[lw[lw >= 0]]), r


@pytest.mark.parametrize("width", [16, 24])
@pytest.mark.parametrize("k", [1, 64, 512])
@pytest.mark.parametrize("S", [37, 5000])
def test_sampler_rows_by_id(cuda, oracle, S, k, width):
    from reservoir_amd import batch

    present, batches = _feed(S)
    rng = np.random.default_rng(k + width)
    got = batch.SegmentedSamplerRows(S, k, width, SEED, stream_base=BASE, device=cuda)
    ref = batch.SegmentedSamplerRows(S, k, width, SEED, stream_base=BASE, device=cuda)
    got.rows.fill_(0xA5)
    ref.rows.fill_(0xA5)
    fed = []
    for b, ids in enumerate(batches):
        rows = rng.integers(0, 256, size=(ids.size, width), dtype=np.uint8)
        fed.append(rows)
        rows_dev = _dev(cuda, rows) if b != 1 else _dev(cuda, rows.view(np.int64))  # both documented layouts
        assert got.update_by_id(rows_dev, _dev(cuda, ids)) is got
        pos, offs, present_rows = _host_group(ids, S)
        ref.update(_dev(cuda, rows[pos]), _dev(cuda, offs), stream_ids=_dev(cuda, present_rows))
        _same(got, ref, b)
    streams = _streams(batches, fed, S)
    rows_out, idx, nxt = (t.cpu().numpy() for t in got._state())
    for r in range(S):
        st = streams.get(r)
        if st is None:
            assert nxt[r] == 0 and (idx[r] == -1).all() and (rows_out[r] == 0xA5).all(), r
            continue
        lw = oracle.algo_r_last_writers(SEED, BASE + r, k, 0, st.shape[0])
        assert nxt[r] == st.shape[0] and np.array_equal(idx[r], lw), r
        assert np.array_equal(rows_out[r][lw >= 0], st[lw[lw >= 0]]), r


@pytest.mark.parametrize("S", [37, 5000])
def test_distinct_by_id(cuda, S):
    from reservoir_amd import batch

    _, batches = _feed(S)
    rng = np.random.default_rng(S + 1)
    got = batch.SegmentedDistinct(S, 64, 9, stream_base=2, device=cuda)
    ref = batch.SegmentedDistinct(S, 64, 9, stream_base=2, device=cuda)
    for t in got._state()[:2] + ref._state()[:2]:
        t.fill_(FILL)
    for b, ids in enumerate(batches):
        keys = rng.integers(0, 3000, size=ids.size).astype(np.int64) * 0x1E3779B97F4A7 - 7  # 3000 values: repeats
        assert got.update_by_id(_dev(cuda, keys), _dev(cuda, ids)) is got
        pos, offs, rows = _host_group(ids, S)
        ref.update(_dev(cuda, keys[pos]), _dev(cuda, offs), stream_ids=_dev(cuda, rows))
        _same(got, ref, b)
    assert got.counts.max().item() == 64


@pytest.mark.parametrize("S", [37, 5000])
def test_distinct_rows_by_id(cuda, S):
    from reservoir_amd import batch

    _, batches = _feed(S)
    rng = np.random.default_rng(S + 2)
    got = batch.SegmentedDistinctRows(S, 64, 16, 9, stream_base=2, device=cuda)
    ref = batch.SegmentedDistinctRows(S, 64, 16, 9, stream_base=2, device=cuda)
    for t in got._state()[:2] + ref._state()[:2]:
        t.fill_(3)
    pool = rng.integers(0, 256, size=(3000, 16), dtype=np.uint8)
    for b, ids in enumerate(batches):
        rows = pool[rng.integers(0, pool.shape[0], size=ids.size)]
        assert got.update_by_id(_dev(cuda, rows), _dev(cuda, ids)) is got
        pos, offs, present_rows = _host_group(ids, S)
        ref.update(_dev(cuda, rows[pos]), _dev(cuda, offs), stream_ids=_dev(cuda, present_rows))
        _same(got, ref, b)


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("S", [37, 5000])
def test_ordered_distinct_by_id_keeps_arrival_order(cuda, oracle, S, k):
    """A colliding hash (key % (k // 2 + 1): fewer values than k, every full row tied): which keys a row holds, and
    where in the heap array, depends on the order its elements arrived in."""
    from reservoir_amd import batch

    _, batches = _feed(S)
    rng = np.random.default_rng(S + k)
    got = batch.SegmentedDistinctOrdered(S, k, 11, stream_base=3, hash="precomputed", device=cuda)
    r0, r1 = _r01(oracle, k, 11, 3, S)
    model = H.HeapModel(S, k, r0, r1)
    for b, ids in enumerate(batches):
        keys = rng.integers(0, 5 * k + 1, size=ids.size).astype(np.int64)
        hashed = keys % (k // 2 + 1)
        assert got.update_by_id(_dev(cuda, keys), _dev(cuda, ids), hashes=_dev(cuda, hashed)) is got
        for r in np.unique(ids):
            if 0 <= r < S:
                model.feed(int(r), keys[ids == r], hashed[ids == r])
        wk, wh, wc = model.rows()
        gk, gh, gc = (t.cpu().numpy() for t in got._state())
        assert np.array_equal(gc, wc), (b, np.flatnonzero(gc != wc)[:8])
        live = np.arange(k)[None, :] < wc[:, None]
        assert np.array_equal(gk[live], wk[live]), (b, np.argwhere((gk != wk) & live)[:5])
        assert np.array_equal(gh[live], wh[live]), (b, np.argwhere((gh != wh) & live)[:5])
    assert (wc == k).sum() >= 1


@pytest.mark.parametrize("k,n", [(64, 700), (512, 3000)])
def test_indirect_update_skips_bad_order_entries(cuda, oracle, k, n):
    """rsv_sample_segmented_update_indirect with one order entry >= n_keys and one negative one, both at winning
    positions: the call completes, every other slot is right, and those two keep their key and idx."""
    import torch

    from reservoir_amd import _native as N

    L = N.load()
    rng = np.random.default_rng(k)
    keys = rng.integers(-2**62, 2**62, size=n)
    perm = rng.permutation(n).astype(np.int32)  # the segment's p-th element is keys[perm[p]]
    lw = oracle.algo_r_last_writers(SEED, BASE, k, 0, n)
    assert (lw >= 0).all()
    j_hi, j_neg = 3, k - 1  # a replaced slot's winner and another one's
    order = perm.copy()
    order[lw[j_hi]] = n
    order[lw[j_neg]] = -5
    keys_dev, order_dev = _dev(cuda, keys), _dev(cuda, order)
    offs = _dev(cuda, np.array([0, n], np.int64))
    sk = torch.full((1, k), FILL, dtype=torch.int64, device=cuda)
    si = torch.full((1, k), -1, dtype=torch.int64, device=cuda)
    sn = torch.zeros(1, dtype=torch.int64, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    N.check(L.rsv_sample_segmented_update_indirect(p(keys_dev), n, p(order_dev), p(offs), None, None, 1, 1, 8, k, SEED,
                                                   BASE, p(sk), p(si), p(sn),
                                                   C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
    torch.cuda.synchronize()
    sk, si, sn = sk.cpu().numpy()[0], si.cpu().numpy()[0], sn.cpu().numpy()
    ok = np.ones(k, bool)
    ok[[j_hi, j_neg]] = False
    assert sn[0] == n
    assert np.array_equal(si[ok], lw[ok]) and np.array_equal(sk[ok], keys[perm[lw[ok]]])
    assert (si[~ok] == -1).all() and (sk[~ok] == FILL).all()


def test_argument_checks(cuda):
    import torch

    from reservoir_amd import batch
    from reservoir_amd._native import IllegalArgumentException

    st = batch.SegmentedSampler(4, 2, 1, device=cuda)
    keys = torch.zeros(6, dtype=torch.int64, device=cuda)
    ids = torch.zeros(6, dtype=torch.int64, device=cuda)
    with pytest.raises(IllegalArgumentException, match="device tensors"):
        st.update_by_id(keys.cpu(), ids)
    with pytest.raises(IllegalArgumentException, match="state's dtype"):
        st.update_by_id(keys.to(torch.int32), ids)
    with pytest.raises(IllegalArgumentException, match="int64/int32"):
        st.update_by_id(keys, ids.to(torch.int16))
    with pytest.raises(IllegalArgumentException, match="one id per"):
        st.update_by_id(keys, ids[:5])
    rs = batch.SegmentedSamplerRows(4, 2, 16, 1, device=cuda)
    with pytest.raises(IllegalArgumentException, match="16 bytes"):
        rs.update_by_id(torch.zeros((6, 24), dtype=torch.uint8, device=cuda), ids)
    ds = batch.SegmentedDistinct(4, 2, 1, device=cuda)
    with pytest.raises(IllegalArgumentException, match="one id per"):
        ds.update_by_id(keys, ids[:5])
    assert st.update_by_id(keys[:0], ids[:0]) is st and st.next.sum().item() == 0
