"""Ordered segmented Sampler.distinct over byte keys (rsv_distinct_segmented_rows_ordered,
batch.distinct_segmented_rows_ordered): S independent RandomValues over rows of W bytes per launch, exact for
any hash, the boundary hash bucket included -- UUID.hashCode's 32 bits above all.

Stream s is seeded with java.util.Random(seed + stream_base + s) and must hold exactly the rows
oracle.DistinctRows (the oracle's RandomValues restatement over byte keys: heap order, arrival order) holds
after the stream's rows in order.  Its result() is sorted by (h, words), which is how the launch writes, so
rows, hashes, counts and the zeros beyond the count are compared bit for bit.  tied is compared with its
definition stated in numpy: the bottom-(k + 1) by (h, row) is full and its last two entries share their hash
(= some distinct row outside the bottom-k by (h, row) has the set's maximum hash).

Every case that claims ties first asserts, from the oracle and numpy alone, that the oracle's set differs from
the bottom-k in some stream and only in tied ones: a set-order implementation fails here.
"""
import ctypes as C

import numpy as np
import pytest
from hash_targets import MAX, MIN, plant, r01
from segdistinct_ref import _r01
from segdistinct_rows_ref import U64, expected_rows, hashes_of, ragged_ids, rows_of, uuid_hashcode_np

pytestmark = pytest.mark.gpu


def _run(cuda, rows, offs, k, seed, stream_base=0, hashes=None, **kw):
    import torch

    from reservoir_amd import batch

    if hashes is not None:
        kw["hashes"] = torch.from_numpy(hashes).to(cuda)
    got = batch.distinct_segmented_rows_ordered(torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                                seed=seed, stream_base=stream_base, **kw)
    assert got[0].dtype == torch.uint8 and got[3].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in got)


def _oracle_rows(oracle, rows, offs, k, seed, base=0, hashes=None):
    """Per stream the oracle's set, ascending by (h, words), zeros beyond the count: (rows, hashes, counts)."""
    S, W = offs.size - 1, rows.shape[1]
    orow, oh, oc = np.zeros((S, k, W), np.uint8), np.zeros((S, k), np.int64), np.zeros(S, np.int64)
    for s in range(S):
        ref = oracle.DistinctRows(k, seed + base + s, W, "uuid" if hashes is None else "precomputed")
        ref.sample_all(rows[offs[s]:offs[s + 1]], None if hashes is None else hashes[offs[s]:offs[s + 1]])
        rr, rh = ref.result()
        m = rr.shape[0]
        orow[s, :m], oh[s, :m], oc[s] = rr, rh, m
    return orow, oh, oc


def _tied_np(rows, hashed, offs, k, r0, r1):
    """The definition: k + 1 distinct rows exist and the (k+1)-th by (h, row) carries the k-th's hash."""
    _, wh, wc = expected_rows(rows, hashed, offs, k + 1, r0, r1)
    return ((wc == k + 1) & (wh[:, k] == wh[:, k - 1])).astype(np.int32)


def _differs(a, b):
    """Streams whose sets differ (row blocks are sorted: equal sets are equal blocks)."""
    return (a[0] != b[0]).any(axis=(1, 2))


def _check(got, want, tied):
    gr, gh, gc, gt = got
    assert gr.shape == want[0].shape
    assert np.array_equal(gc, want[2])
    bad = np.flatnonzero((gr != want[0]).any(axis=(1, 2)) | (gh != want[1]).any(axis=1))
    assert bad.size == 0, (bad[:10], gt[bad[:10]], tied[bad[:10]])
    assert np.array_equal(gt, tied), np.flatnonzero(gt != tied)[:10]


def _uuids(v, c, s):
    """msb = splitmix of (v, c, s), lsb = msb ^ (v << 32 | c ^ v): equal (v, c) of a stream are one row and
    UUID.hashCode = (v ^ (c ^ v)) = c."""
    v, c = v.astype(U64), c.astype(U64)
    msb = rows_of((U64(s) << U64(40)) | (v << U64(32)) | c, 8, salt=5).view(U64).reshape(-1)
    return np.stack([msb, msb ^ ((v << U64(32)) | (c ^ v))], axis=1).view(np.uint8).reshape(-1, 16)


def _case1(k, S=12):
    """Up to 4 UUIDs per hashCode, k + 3 hashCodes: the boundary bucket is oversubscribed."""
    segs = []
    for s in range(S):
        rng = np.random.default_rng(1000 * k + s)
        n = int(rng.integers(5 * k + 8, 7 * k + 16))
        c = rng.integers(0, k + 3, n)
        v = rng.integers(0, 4, n)
        segs.append(_uuids(v, c, s))
    offs = np.r_[0, np.cumsum([x.shape[0] for x in segs])].astype(np.int64)
    return np.concatenate(segs), offs


def _reorder(rows, offs, how):
    out = rows.copy()
    for s in range(offs.size - 1):
        seg = rows[offs[s]:offs[s + 1]]
        out[offs[s]:offs[s + 1]] = seg[::-1] if how == "reversed" else seg[np.random.default_rng(5).permutation(seg.shape[0])]
    return out


_CASE1 = {}


def _case1_ref(oracle, k):
    """Case 1's input, (r0, r1), oracle rows, bottom-k rows and tied, computed once per k and left unchanged."""
    if k not in _CASE1:
        rows, offs = _case1(k)
        S = offs.size - 1
        r0, r1 = _r01(oracle, k, 77, 0, S)
        hashed = uuid_hashcode_np(rows)
        assert hashed.min() == 0 and hashed.max() == k + 2
        _CASE1[k] = (rows, offs, r0, r1, _oracle_rows(oracle, rows, offs, k, 77),
                     expected_rows(rows, hashed, offs, k, r0, r1), _tied_np(rows, hashed, offs, k, r0, r1))
    return _CASE1[k]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 256, 257, 1024, 1025, 4096])
def test_tied_parity_over_every_form(cuda, oracle, k):
    rows, offs, r0, r1, want, bottom, tied = _case1_ref(oracle, k)
    # from the oracle alone: the reference's set is not the bottom-k by (h, row) in some stream, and only in tied ones
    diff = _differs(want, bottom)
    assert diff.any() and np.array_equal(want[2], bottom[2]) and not (diff & (tied == 0)).any()
    _check(_run(cuda, rows, offs, k, 77, hash="default"), want, tied)


@pytest.mark.parametrize("k", [64, 1024])
@pytest.mark.parametrize("how", ["reversed", "permuted"])
def test_arrival_order_is_followed(cuda, oracle, k, how):
    rows, offs, r0, r1, fwd, _, _ = _case1_ref(oracle, k)
    rows = _reorder(rows, offs, how)
    want = _oracle_rows(oracle, rows, offs, k, 77)
    assert _differs(want, fwd).any()  # the order decides the set
    _check(_run(cuda, rows, offs, k, 77), want, _tied_np(rows, uuid_hashcode_np(rows), offs, k, r0, r1))


@pytest.mark.parametrize("width,k", [(24, 5), (64, 64), (256, 512)])
def test_precomputed_hashes_wider_rows(cuda, oracle, width, k):
    """Ids 0 .. 5k under id % (k // 2 + 1): fewer hash values than k, every full stream is tied.  The last two
    streams hold k - 2 and exactly k distinct rows: never tied."""
    rng = np.random.default_rng(k)
    segs = []
    for s in range(8):
        d = rng.permutation(5 * k + 1) if s < 6 else rng.permutation(5 * k + 1)[:k - 2 if s == 6 else k]
        segs.append(np.r_[d, rng.choice(d, size=max(1, (3 * d.size) // 10))].astype(np.int64))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    ids = np.concatenate(segs)
    rows, hashed = rows_of(ids, width), ids % (k // 2 + 1)
    r0, r1 = _r01(oracle, k, 11, 3, 8)
    tied = _tied_np(rows, hashed, offs, k, r0, r1)
    assert np.array_equal(tied, [1] * 6 + [0, 0])
    want = _oracle_rows(oracle, rows, offs, k, 11, 3, hashes=hashed)
    assert np.array_equal(want[2], [k] * 6 + [k - 2, k])
    diff = _differs(want, expected_rows(rows, hashed, offs, k, r0, r1))
    assert np.array_equal(diff, [True] * 6 + [False, False])
    _check(_run(cuda, rows, offs, k, 11, 3, hashes=hashed), want, tied)


@pytest.mark.parametrize("k", [17, 600])
def test_injective_hashes_are_the_set_launch(cuda, oracle, k):
    import torch

    from reservoir_amd import batch

    rng = np.random.default_rng(k)
    lens = rng.integers(0, 3000, size=100)
    lens[:4] = [0, 1, k, k + 1]
    ids, offs = ragged_ids(rng, lens)
    rd = torch.from_numpy(rows_of(ids, 16)).to(cuda)
    hd, od = torch.from_numpy(hashes_of(ids)).to(cuda), torch.from_numpy(offs).to(cuda)
    a = batch.distinct_segmented_rows_ordered(rd, od, k, seed=9, stream_base=4, hashes=hd)
    b = batch.distinct_segmented_rows(rd, od, k, seed=9, stream_base=4, hashes=hd)
    assert not a[3].any().item()
    assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a[:3], b))
    assert (b[2] == k).any().item() and (b[2] < k).any().item()


def _id_rows(ids):
    """16-byte rows [id | 7]: the order of the rows is the order of the ids."""
    w = np.full((len(ids), 2), 7, dtype=U64)
    w[:, 0] = np.asarray(ids, dtype=U64)
    return w.view(np.uint8).reshape(-1, 16)


def test_hash_edges(cuda, oracle):
    """k = 64, W = 16, one stream per case, hashes planted at exact scrambled values:
    0  k - 1 rows below and one at MAX (the sort's pad hash), with repeats: full, nothing outside
    1  the same plus a second row at MAX, the larger row first: tied, and the first to arrive stays
    2  k - 2 rows at MIN, then three at MIN + 1: the boundary bucket holds two of the three
    3  k + 1 rows at MIN: maxHash = MIN admits nothing once the heap is full"""
    k, seed = 64, 31
    rng = np.random.default_rng(1)
    below = [MIN, MIN + 1, -1, 0, MAX - 1] + [int(x) for x in rng.integers(-2**62, 2**62, size=k - 6)]
    r = [r01(oracle, seed + s) for s in range(4)]
    id0 = np.arange(100, 100 + k)
    segs = [np.r_[id0, id0[::3]]]
    h0 = plant(*r[0], below + [MAX])
    hs = [np.r_[h0, h0[::3]]]
    segs.append(np.r_[np.arange(100, 100 + k - 1), 9000, 8000, np.arange(100, 120)])
    hs.append(plant(*r[1], below + [MAX, MAX] + below[:20]))
    segs.append(np.r_[np.arange(k - 2), 702, 701, 700, np.arange(10)])
    hs.append(plant(*r[2], [MIN] * (k - 2) + [MIN + 1] * 3 + [MIN] * 10))
    segs.append(rng.permutation(k + 1))
    hs.append(plant(*r[3], [MIN] * (k + 1)))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    ids, hashed = np.concatenate(segs), np.concatenate(hs)
    rows = _id_rows(ids)
    r0 = np.array([x[0] for x in r], dtype=np.int64)
    r1 = np.array([x[1] for x in r], dtype=np.int64)
    tied = _tied_np(rows, hashed, offs, k, r0, r1)
    assert np.array_equal(tied, [0, 1, 1, 1])
    want = _oracle_rows(oracle, rows, offs, k, seed, hashes=hashed)
    assert np.array_equal(want[2], [k] * 4)
    held1 = want[0][1].view(U64).reshape(k, 2)[:, 0]
    assert want[1][0, k - 1] == MAX and want[1][1, k - 1] == MAX and 9000 in held1 and 8000 not in held1
    assert want[1][2, k - 1] == MIN + 1 and want[1][3, k - 1] == MIN
    diff = _differs(want, expected_rows(rows, hashed, offs, k, r0, r1))
    assert diff[1] and not diff[0]
    _check(_run(cuda, rows, offs, k, seed, hashes=hashed), want, tied)


@pytest.mark.parametrize("k", [3, 70])
def test_repeats_of_a_member_in_the_boundary_bucket_are_no_tie(cuda, oracle, k):
    """k distinct rows, the last two sharing the maximum hash M, then repeats of the smaller of the two: the
    merge leaves those repeats behind position k, below T's own position, with h = M and a row that is not
    T's.  They are members, so stream 0 is untied; stream 1 adds one larger row at M and is tied; stream 2
    adds a smaller one instead (the bottom-k changes, the reference keeps the first to arrive)."""
    seed = 12
    r = [r01(oracle, seed + s) for s in range(3)]
    base = np.arange(10, 10 + k)
    below = [int(x) for x in np.random.default_rng(k).integers(-2**62, 2**62, size=k - 2)]
    m = MAX - 5
    reps = 3 * k + 150  # more than a merge's buffer at either k
    segs = [np.r_[base, np.full(reps, base[-2])],
            np.r_[base, np.full(reps, base[-2]), 9000, np.full(reps, base[-2])],
            np.r_[base, np.full(reps, base[-2]), 5, np.full(reps, base[-2])]]
    hs = [plant(*r[0], below + [m, m] + [m] * reps),
          plant(*r[1], below + [m, m] + [m] * reps + [m] + [m] * reps),
          plant(*r[2], below + [m, m] + [m] * reps + [m] + [m] * reps)]
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    ids, hashed = np.concatenate(segs), np.concatenate(hs)
    rows = _id_rows(ids)
    r0 = np.array([x[0] for x in r], dtype=np.int64)
    r1 = np.array([x[1] for x in r], dtype=np.int64)
    tied = _tied_np(rows, hashed, offs, k, r0, r1)
    assert np.array_equal(tied, [0, 1, 1])
    want = _oracle_rows(oracle, rows, offs, k, seed, hashes=hashed)
    diff = _differs(want, expected_rows(rows, hashed, offs, k, r0, r1))
    assert np.array_equal(diff, [False, False, True])
    _check(_run(cuda, rows, offs, k, seed, hashes=hashed), want, tied)


def test_rows_base_at_8_mod_16(cuda, oracle):
    """rows_dev one word into an allocation: a UUID is two 8-byte loads in both kernels; and 16-byte aligned."""
    import torch

    from reservoir_amd import batch

    k = 64
    rows, offs, r0, r1, want, _, tied = _case1_ref(oracle, k)
    assert tied.any()
    words = torch.from_numpy(rows.view(np.int64).reshape(-1))
    shifted = torch.empty(words.numel() + 1, dtype=torch.int64, device=cuda)
    shifted[1:] = words.to(cuda)
    od = torch.from_numpy(offs).to(cuda)
    for off8 in (1, 0):
        rd = (shifted[1:] if off8 else shifted[1:].clone()).view(-1, 2)  # int64 rows: the same memory
        assert rd.data_ptr() % 16 == 8 * off8
        got = batch.distinct_segmented_rows_ordered(rd, od, k, seed=77)
        _check(tuple(t.cpu().numpy() for t in got), want, tied)


def test_offsets_past_zero_and_empty_streams(cuda, oracle):
    k = 64
    rows, offs = _case1(k)
    S = 2 * (offs.size - 1) + 1
    lens = np.zeros(S, dtype=np.int64)
    lens[1::2] = np.diff(offs)  # an empty stream before, between and behind the tied ones
    offs2 = (3 + np.r_[0, np.cumsum(lens)]).astype(np.int64)
    rows2 = np.concatenate([rows_of(np.arange(3), 16), rows])
    r0, r1 = _r01(oracle, k, 5, 100, S)
    tied = _tied_np(rows2, uuid_hashcode_np(rows2), offs2, k, r0, r1)
    assert tied[1::2].sum() >= 3 and not tied[::2].any()
    want = _oracle_rows(oracle, rows2, offs2, k, 5, 100)
    _check(_run(cuda, rows2, offs2, k, 5, 100), want, tied)


def test_side_stream_same_buffers_and_null_hashes(cuda, oracle):
    """A non-default torch stream, the call repeated into the same buffers; out_hashes_dev = NULL."""
    import torch

    from reservoir_amd import _native as N

    k = 64
    rows, offs, r0, r1, want, _, tied = _case1_ref(oracle, k)
    S = offs.size - 1
    rd, od = torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda)
    out = torch.full((S, k, 16), 0xFF, dtype=torch.uint8, device=cuda)
    oh = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    cnt = torch.full((S,), -1, dtype=torch.int64, device=cuda)
    td = torch.full((S,), -1, dtype=torch.int32, device=cuda)
    vp = C.c_void_p

    def call(hashes_out, stream):
        N.check(N.load().rsv_distinct_segmented_rows_ordered(
            vp(rd.data_ptr()), None, vp(od.data_ptr()), S, 16, k, N.HASH_DEFAULT, 77, 0, vp(out.data_ptr()),
            vp(hashes_out.data_ptr()) if hashes_out is not None else None, vp(cnt.data_ptr()), vp(td.data_ptr()),
            vp(stream.cuda_stream)))

    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        call(oh, st)
        first = [t.clone() for t in (out, oh, cnt, td)]
        call(oh, st)
    st.synchronize()
    _check([t.cpu().numpy() for t in (out, oh, cnt, td)], want, tied)
    assert all(torch.equal(x, y) for x, y in zip(first, (out, oh, cnt, td)))
    out.fill_(0xFF)
    oh.fill_(-1)
    torch.cuda.synchronize()
    call(None, torch.cuda.current_stream(cuda))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[0]) and (oh == -1).all().item()
    assert np.array_equal(td.cpu().numpy(), tied)


def test_grid_stride_with_many_tied_streams(cuda, oracle):
    """20 011 streams of 8 rows at k = 2, 3 hashCodes x 4 UUIDs: both kernels stride, the replay groups the tied
    words, hundreds of streams are tied."""
    S, k = 20_011, 2
    rng = np.random.default_rng(20_011)
    c, v = rng.integers(0, 3, 8 * S), rng.integers(0, 4, 8 * S)
    rows = _uuids(v, c, 0)
    offs = np.arange(0, 8 * S + 1, 8, dtype=np.int64)
    r0, r1 = _r01(oracle, k, 3, 0, S)
    hashed = uuid_hashcode_np(rows)
    want = _oracle_rows(oracle, rows, offs, k, 3)
    tied = _tied_np(rows, hashed, offs, k, r0, r1)
    diff = _differs(want, expected_rows(rows, hashed, offs, k, r0, r1))
    assert tied.sum() > 100 and diff.sum() > 100 and not (diff & (tied == 0)).any()
    _check(_run(cuda, rows, offs, k, 3, hash="default"), want, tied)


def test_one_ordered_handle_per_stream(cuda, oracle):
    import torch

    from reservoir_amd import Sampler

    k, seed = 64, 77
    rows, offs, r0, r1, want, _, tied = _case1_ref(oracle, k)
    gr, gh, gc, gt = _run(cuda, rows, offs, k, seed)
    assert gt[:8].any()
    for s in range(8):
        d = Sampler.distinct(k, key_type="bytes16", seed=seed + s, order="ordered")()
        d.sample_all(torch.from_numpy(rows[offs[s]:offs[s + 1]]).to(cuda))
        held = np.asarray(d.result()).reshape(-1, 16)
        assert sorted(bytes(x) for x in held) == sorted(bytes(x) for x in gr[s, :gc[s]]), s


def test_bad_arguments_raise_as_the_set_launch(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch

    rows = torch.zeros((10, 16), dtype=torch.uint8, device=cuda)
    offs = torch.tensor([0, 10], dtype=torch.int64, device=cuda)
    cases = [
        (IllegalArgumentException, lambda f: f(rows.view(-1), offs, 4, seed=1)),  # 1-D rows
        (IllegalArgumentException, lambda f: f(rows.cpu(), offs, 4, seed=1)),  # host tensors
        (ReservoirError, lambda f: f(torch.zeros((10, 24), dtype=torch.uint8, device=cuda), offs, 4, seed=1)),
        (NullPointerException, lambda f: f(rows, offs, 4, seed=1, hash="precomputed")),
    ]
    for exc, call in cases:
        for f in (batch.distinct_segmented_rows, batch.distinct_segmented_rows_ordered):
            with pytest.raises(exc):
                call(f)
