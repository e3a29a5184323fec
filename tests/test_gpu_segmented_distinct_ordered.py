"""Ordered segmented Sampler.distinct (rsv_distinct_segmented_ordered): S independent RandomValues per launch,
exact for any hash, the boundary hash bucket included.

Stream s is seeded with java.util.Random(seed + stream_base + s) and must hold exactly the set
oracle.Distinct (the oracle's RandomValues restatement: heap order, arrival order) holds after the stream's
keys in order.  The reference's result order is a HashSet's; the launch writes ascending by (h, key), zeros
beyond the count, so every row is compared exactly with the oracle's (keys, hashes) sorted that way.  tied
is compared with the definition stated in numpy: the set is full and the (k+1)-th distinct key by (h, key)
has the k-th's hash (= some distinct key outside the bottom-k by (h, key) has the set's maximum hash).
"""
import ctypes as C

import numpy as np
import pytest
from hash_targets import MAX, MIN, plant, r01
from segdistinct_ref import _expected, _hash_np, _r01, _scramble, _with_repeats

pytestmark = pytest.mark.gpu


def _run(cuda, keys, offs, k, seed, stream_base=0, **kw):
    import torch

    from reservoir_amd import batch

    if "hashes" in kw:
        kw["hashes"] = torch.from_numpy(kw["hashes"]).to(cuda)
    got = batch.distinct_segmented_ordered(torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                           seed=seed, stream_base=stream_base, **kw)
    assert got[3].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in got)


def _oracle_rows(oracle, keys, offs, k, seed, base=0, kind=None, hashes=None):
    """Per stream the oracle's set as rows ascending by (h, key), zeros beyond the count: (keys, hashes, counts)."""
    S = offs.size - 1
    ok, oh, oc = np.zeros((S, k), np.int64), np.zeros((S, k), np.int64), np.zeros(S, np.int64)
    for s in range(S):
        seg = np.ascontiguousarray(keys[offs[s]:offs[s + 1]]).astype(np.int64)
        if hashes is None:
            ref = oracle.Distinct(k, seed + base + s, kind)
            ref.sample_all(seg)
            rk, rh = ref.result()
        else:
            ref = oracle.DistinctRows(k, seed + base + s, 8)
            ref.sample_all(seg.view(np.uint8).reshape(-1, 8), hashes[offs[s]:offs[s + 1]])
            rr, rh = ref.result()
            rk = np.ascontiguousarray(rr).view(np.int64).reshape(-1)
        o = np.lexsort((rk, rh))
        ok[s, :rk.size], oh[s, :rk.size], oc[s] = rk[o], rh[o], rk.size
    return ok, oh, oc


def _tied_np(keys, hashed, offs, k, r0, r1):
    """The definition: counts == k and the (k+1)-th distinct key by (h, key) carries the k-th's hash."""
    wk, wh, wc = _expected(keys, hashed, offs, k + 1, r0, r1)
    return ((wc == k + 1) & (wh[:, k] == wh[:, k - 1])).astype(np.int32)


def _differs(a, b):
    """Streams whose sets differ (rows are sorted: equal sets are equal rows)."""
    return (a[0] != b[0]).any(axis=1)


def _check(got, want, tied):
    gk, gh, gc, gt = got
    assert np.array_equal(gc, want[2])
    bad = np.flatnonzero((gk.astype(np.int64) != want[0]).any(axis=1) | (gh != want[1]).any(axis=1))
    assert bad.size == 0, (bad[:10], gt[bad[:10]], tied[bad[:10]])
    assert np.array_equal(gt, tied), np.flatnonzero(gt != tied)[:10]


def _case1(k, S=12):
    """Up to 4 keys per Long.hashCode, k + 3 hash codes: the boundary bucket is oversubscribed."""
    segs = []
    for s in range(S):
        rng = np.random.default_rng(1000 * k + s)
        n = int(rng.integers(5 * k + 8, 7 * k + 16))
        lo = rng.integers(0, k + 3, n)
        hi = rng.integers(0, 4, n)
        segs.append((hi.astype(np.int64) << 32) | (lo ^ hi).astype(np.int64))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    return np.concatenate(segs), offs


def _reorder(keys, offs, how):
    out = keys.copy()
    for s in range(offs.size - 1):
        seg = keys[offs[s]:offs[s + 1]]
        out[offs[s]:offs[s + 1]] = seg[::-1] if how == "reversed" else seg[np.random.default_rng(5).permutation(seg.size)]
    return out


_CASE1 = {}


def _case1_ref(oracle, k):
    """Case 1's input, (r0, r1), oracle rows, bottom-k rows and tied, computed once per k."""
    if k not in _CASE1:
        keys, offs = _case1(k)
        S = offs.size - 1
        r0, r1 = _r01(oracle, k, 77, 0, S)
        hashed = _hash_np(keys, "java_long")
        want = _oracle_rows(oracle, keys, offs, k, 77, kind=oracle.HASH_JAVA_LONG)
        _CASE1[k] = (keys, offs, r0, r1, hashed, want, _expected(keys, hashed, offs, k, r0, r1),
                     _tied_np(keys, hashed, offs, k, r0, r1))
    return _CASE1[k]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 256, 257, 1024, 1025, 4096])
def test_tied_parity_over_every_form(cuda, oracle, k):
    keys, offs, r0, r1, hashed, want, bottom, tied = _case1_ref(oracle, k)
    # from the oracle alone: the reference's set is not the bottom-k by (h, key) in some stream, and only in tied ones
    diff = _differs(want, bottom)
    assert diff.any() and np.array_equal(want[2], bottom[2]) and not (diff & (tied == 0)).any()
    _check(_run(cuda, keys, offs, k, 77, hash="default"), want, tied)


@pytest.mark.parametrize("k", [64, 1024])
@pytest.mark.parametrize("how", ["reversed", "permuted"])
def test_arrival_order_is_followed(cuda, oracle, k, how):
    keys, offs, r0, r1, hashed, fwd, _, _ = _case1_ref(oracle, k)
    keys = _reorder(keys, offs, how)
    hashed = _hash_np(keys, "java_long")
    want = _oracle_rows(oracle, keys, offs, k, 77, kind=oracle.HASH_JAVA_LONG)
    assert _differs(want, fwd).any()  # the order decides the set
    _check(_run(cuda, keys, offs, k, 77, hash="java_long"), want, _tied_np(keys, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("k", [5, 64, 512])
def test_precomputed_hashes(cuda, oracle, k):
    """Keys 0 .. 5k under key % (k // 2 + 1): fewer hash values than k, every full stream is tied.  The last
    two streams hold fewer than k and exactly k distinct keys: never tied."""
    rng = np.random.default_rng(k)
    segs = []
    for s in range(8):
        d = rng.permutation(5 * k + 1) if s < 6 else rng.permutation(5 * k + 1)[:k - 2 if s == 6 else k]
        segs.append(np.r_[d, rng.choice(d, size=max(1, (3 * d.size) // 10))].astype(np.int64))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    keys = np.concatenate(segs)
    hashed = keys % (k // 2 + 1)
    r0, r1 = _r01(oracle, k, 11, 3, 8)
    tied = _tied_np(keys, hashed, offs, k, r0, r1)
    assert np.array_equal(tied, [1] * 6 + [0, 0])
    want = _oracle_rows(oracle, keys, offs, k, 11, 3, hashes=hashed)
    assert np.array_equal(want[2], [k] * 6 + [k - 2, k])
    _check(_run(cuda, keys, offs, k, 11, 3, hashes=hashed), want, tied)


@pytest.mark.parametrize("k", [17, 600])
@pytest.mark.parametrize("kind", ["identity", "java_int"])
def test_injective_hashes_are_the_set_launch(cuda, oracle, k, kind):
    import torch

    from reservoir_amd import batch

    rng = np.random.default_rng(k)
    lens = rng.integers(0, 3000, size=100)
    lens[:4] = [0, 1, k, k + 1]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n = int(offs[-1])
    if kind == "identity":
        keys = _with_repeats(rng, oracle.splitmix_keys(k, n), offs)
    else:
        keys = np.where(rng.random(n) < 0.5, rng.integers(-2**31, 2**31, size=n), rng.integers(-700, 700, size=n))
        keys = keys.astype(np.int32)
    kd, od = torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda)
    a = batch.distinct_segmented_ordered(kd, od, k, seed=9, stream_base=4, hash=kind)
    b = batch.distinct_segmented(kd, od, k, seed=9, stream_base=4, hash=kind)
    assert not a[3].any().item()
    assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a[:3], b))
    assert (b[2] == k).any().item() and (b[2] < k).any().item()


def test_hash_edges(cuda, oracle):
    """k = 64, one stream per case, hashes planted at exact scrambled values:
    0  identity keys: k - 1 below and one at MAX (the sort's pad value), with repeats: full, nothing outside
    1  the same plus a second key at MAX, the larger key first: tied, and the first to arrive stays
    2  k - 2 keys at MIN, then three at MIN + 1: the boundary bucket holds two of the three
    3  k + 1 keys at MIN: maxHash = MIN admits nothing once the heap is full"""
    k, seed = 64, 31
    rng = np.random.default_rng(1)
    below = [MIN, MIN + 1, -1, 0, MAX - 1] + [int(x) for x in rng.integers(-2**62, 2**62, size=k - 6)]
    r = [r01(oracle, seed + s) for s in range(4)]
    ident = plant(*r[0], below + [MAX])
    assert np.unique(ident).size == k
    ident = np.r_[ident, ident[::3]]
    segs = [ident]
    hs = [ident]
    key1 = np.r_[np.arange(100, 100 + k - 1), 9000, 8000, np.arange(100, 120)].astype(np.int64)
    segs.append(key1)
    hs.append(plant(*r[1], below + [MAX, MAX] + below[:20]))
    key2 = np.r_[np.arange(k - 2), 702, 701, 700, np.arange(10)].astype(np.int64)
    segs.append(key2)
    hs.append(plant(*r[2], [MIN] * (k - 2) + [MIN + 1] * 3 + [MIN] * 10))
    segs.append(rng.permutation(k + 1).astype(np.int64))
    hs.append(plant(*r[3], [MIN] * (k + 1)))
    offs = np.r_[0, np.cumsum([x.size for x in segs])].astype(np.int64)
    keys, hashed = np.concatenate(segs), np.concatenate(hs)
    r0 = np.array([x[0] for x in r], dtype=np.int64)
    r1 = np.array([x[1] for x in r], dtype=np.int64)
    tied = _tied_np(keys, hashed, offs, k, r0, r1)
    assert np.array_equal(tied, [0, 1, 1, 1])
    want = _oracle_rows(oracle, keys, offs, k, seed, hashes=hashed)
    assert want[1][0, k - 1] == MAX and want[1][1, k - 1] == MAX and 9000 in want[0][1] and 8000 not in want[0][1]
    assert want[1][2, k - 1] == MIN + 1 and want[1][3, k - 1] == MIN
    got = _run(cuda, keys, offs, k, seed, hashes=hashed)
    _check(got, want, tied)
    # case 0 through the identity hash itself (a Long key is its own hash value)
    one = _run(cuda, ident, np.array([0, ident.size], dtype=np.int64), k, seed, hash="identity")
    _check(one, tuple(w[:1] for w in want), tied[:1])


def test_offsets_past_zero_and_empty_streams(cuda, oracle):
    k = 64
    keys, offs = _case1(k)
    S = 2 * (offs.size - 1) + 1
    lens = np.zeros(S, dtype=np.int64)
    lens[1::2] = np.diff(offs)  # an empty stream before, between and behind the tied ones
    offs2 = (3 + np.r_[0, np.cumsum(lens)]).astype(np.int64)
    keys2 = np.r_[np.array([1, 2, 3], dtype=np.int64), keys]
    r0, r1 = _r01(oracle, k, 5, 100, S)
    hashed = _hash_np(keys2, "java_long")
    tied = _tied_np(keys2, hashed, offs2, k, r0, r1)
    assert tied[1::2].sum() >= 3 and not tied[::2].any()
    want = _oracle_rows(oracle, keys2, offs2, k, 5, 100, kind=oracle.HASH_JAVA_LONG)
    _check(_run(cuda, keys2, offs2, k, 5, 100, hash="java_long"), want, tied)


def test_all_empty_launch(cuda):
    for k in (8, 2000):
        gk, gh, gc, gt = _run(cuda, np.zeros(0, dtype=np.int64), np.zeros(51, dtype=np.int64), k, 1)
        assert gk.shape == (50, k) and gt.shape == (50,)
        assert not gk.any() and not gh.any() and not gc.any() and not gt.any()
    gk, gh, gc, gt = _run(cuda, np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), 8, 1)
    assert gk.shape == (0, 8) and gt.shape == (0,)


def test_side_stream_same_buffers_and_null_hashes(cuda, oracle):
    """A non-default torch stream, the call repeated into the same buffers; out_hashes_dev = NULL."""
    import torch

    from reservoir_amd import _native as N

    k = 64
    keys, offs, r0, r1, hashed, want, _, tied = _case1_ref(oracle, k)
    S = offs.size - 1
    kd, od = torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda)
    out = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    oh = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    cnt = torch.full((S,), -1, dtype=torch.int64, device=cuda)
    td = torch.full((S,), -1, dtype=torch.int32, device=cuda)
    vp = C.c_void_p

    def call(hashes_out, stream):
        N.check(N.load().rsv_distinct_segmented_ordered(
            vp(kd.data_ptr()), None, vp(od.data_ptr()), S, 8, k, N.HASH_DEFAULT, 77, 0, vp(out.data_ptr()),
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
    out.fill_(-1)
    oh.fill_(-1)
    torch.cuda.synchronize()
    call(None, torch.cuda.current_stream(cuda))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[0]) and (oh == -1).all().item()
    assert np.array_equal(td.cpu().numpy(), tied)


def test_grid_stride_with_many_tied_streams(cuda, oracle):
    """20 011 streams of 8 elements at k = 2, 3 hash codes x 4 keys: both kernels stride, hundreds of streams tied."""
    S, k = 20_011, 2
    rng = np.random.default_rng(20_011)
    lo, hi = rng.integers(0, 3, 8 * S), rng.integers(0, 4, 8 * S)
    keys = (hi.astype(np.int64) << 32) | (lo ^ hi).astype(np.int64)
    offs = np.arange(0, 8 * S + 1, 8, dtype=np.int64)
    r0, r1 = _r01(oracle, k, 3, 0, S)
    hashed = _hash_np(keys, "java_long")
    want = _oracle_rows(oracle, keys, offs, k, 3, kind=oracle.HASH_JAVA_LONG)
    tied = _tied_np(keys, hashed, offs, k, r0, r1)
    assert tied.sum() > 100 and _differs(want, _expected(keys, hashed, offs, k, r0, r1)).sum() > 100
    _check(_run(cuda, keys, offs, k, 3, hash="default"), want, tied)


def test_one_ordered_handle_per_stream(cuda, oracle):
    import torch

    from reservoir_amd import Sampler

    k, seed = 64, 77
    segs = [_case1(k, 16)]
    keys, offs = segs[0]
    gk, gh, gc, gt = _run(cuda, keys, offs, k, seed, hash="java_long")
    assert gt.any()
    for s in range(16):
        d = Sampler.distinct(k, seed=seed + s, order="ordered")(hash="java_long")
        d.sample_all(torch.from_numpy(keys[offs[s]:offs[s + 1]]).to(cuda))
        assert np.array_equal(np.sort(d.result()), np.sort(gk[s, :gc[s]])), s


def test_bad_arguments_raise(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch
    from reservoir_amd import _native as N

    keys = torch.arange(10, dtype=torch.int64, device=cuda)
    offs = torch.tensor([0, 10], dtype=torch.int64, device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented_ordered(keys, offs, 0, seed=1)
    with pytest.raises(ReservoirError, match="4096"):
        batch.distinct_segmented_ordered(keys, offs, 4097, seed=1)
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented_ordered(keys, offs, 4, seed=1, hash="md5")
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented_ordered(keys.cpu(), offs, 4, seed=1)
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented_ordered(keys, offs, 4, seed=1, hashes=keys[:3])
    vp = C.c_void_p
    with pytest.raises(NullPointerException, match="tied_dev"):
        N.check(N.load().rsv_distinct_segmented_ordered(vp(keys.data_ptr()), None, vp(offs.data_ptr()), 1, 8, 4,
                                                        N.HASH_IDENTITY, 1, 0, vp(keys.data_ptr()), None,
                                                        vp(offs.data_ptr()), None, None))
