"""Segmented Sampler.distinct over fixed-width byte keys (rsv_distinct_segmented_rows,
batch.distinct_segmented_rows): S independent distinct samplers over rows of W bytes per launch.

Stream s is seeded with java.util.Random(seed + stream_base + s) and holds the min(k, D_s) distinct
rows with the smallest (scrambled hash, row words as unsigned 64-bit values, word 0 first), ascending.
Every comparison is exact -- rows, hashes, counts, zeros beyond the count -- against the numpy
reference of segdistinct_rows_ref.py (itself pinned to oracle.DistinctRows on the CPU).  Forms as for
Long keys: one wave per stream up to k = 256, a 256-thread workgroup up to k = 1024, a 1024-thread
workgroup up to k = 4096.
"""
import ctypes as C

import hash_targets as HT
import numpy as np
import pytest
from segdistinct_ref import WAVE_MAX_K, _r01, _scramble
from segdistinct_rows_ref import U64, expected_rows, hashes_of, ragged_ids, rows_of, uuid_hashcode_np

pytestmark = pytest.mark.gpu


def _run(cuda, rows, offs, k, seed, stream_base=0, hashes=None, **kw):
    import torch

    from reservoir_amd import batch

    if hashes is not None:
        kw["hashes"] = torch.from_numpy(hashes).to(cuda)
    out = batch.distinct_segmented_rows(torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                        seed=seed, stream_base=stream_base, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _check(got, want):
    gr, gh, gc = got
    wr, wh, wc = want
    assert gr.dtype == np.uint8 and gr.shape == wr.shape
    assert np.array_equal(gc, wc)
    assert np.array_equal(gh, wh)
    assert np.array_equal(gr, wr)  # rows beyond the count are zero on both sides


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, WAVE_MAX_K, WAVE_MAX_K + 1, 1024, 1025, 4096])
def test_ragged_parity(cuda, oracle, k):
    """Each form and both sides of each crossover; lengths from 0 to a few times 4k, ~50 % repeats."""
    rng = np.random.default_rng(k)
    big = k >= 1024
    lens = rng.integers(0, 4 * k + 5000 if big else 5000, size=12 if big else 200)
    lens[:6] = [0, 1, k - 1, k, k + 1, 4097]
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    seed, base = 77, 1000
    r0, r1 = _r01(oracle, k, seed, base, lens.size)
    _check(_run(cuda, rows, offs, k, seed, base, hashes=hashed), expected_rows(rows, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("k", [5, 300])
@pytest.mark.parametrize("width", [24, 64, 256])
def test_widths(cuda, oracle, width, k):
    rng = np.random.default_rng(width + k)
    lens = rng.integers(0, 2500, size=60)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, width), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 5, 0, lens.size)
    _check(_run(cuda, rows, offs, k, 5, hashes=hashed), expected_rows(rows, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("k", [5, 300])
def test_uuid_default_hash(cuda, oracle, k):
    """hash="default": UUID.hashCode on the device.  Every fourth id also arrives as its twin
    [lsb | msb]: another UUID with the same hashCode, so the two tie on h and the words decide."""
    rng = np.random.default_rng(k)
    lens = rng.integers(0, 2500, size=100)
    ids, offs = ragged_ids(rng, lens)
    rows = rows_of(ids, 16)
    twin = (ids % 4 == 0) & (rng.random(ids.size) < 0.5)
    rows[twin] = rows[twin].reshape(-1, 2, 8)[:, ::-1].reshape(-1, 16)
    hashed = uuid_hashcode_np(rows)
    r0, r1 = _r01(oracle, k, 19, 3, lens.size)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    _check(_run(cuda, rows, offs, k, 19, 3), want)
    _check(_run(cuda, rows, offs, k, 19, 3, hash="default"), want)


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
def test_colliding_hashes(cuda, oracle, k, variant):
    """hashes = id % 37: fewer hash values than k = 64, every admission is a tie on h and the rows
    read from global memory carry the result."""
    rng = np.random.default_rng(k * 7 + len(variant))
    lens = rng.integers(0, 3000, size=60)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = _colliding_rows(ids, variant), ids % 37
    if variant == "top_bit":
        w0 = rows.view(np.int64).reshape(-1, 2)[:, 0]
        assert (w0 < 0).any() and (w0 > 0).any()
    r0, r1 = _r01(oracle, k, 4, 50, lens.size)
    _check(_run(cuda, rows, offs, k, 4, 50, hashes=hashed), expected_rows(rows, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("k", [1, 64, 300])
@pytest.mark.parametrize("edge", ["max", "min", "threshold"])
def test_hash_edges(cuda, oracle, k, edge):
    """Precomputed hashes planted so that the scrambled h of more than k distinct rows per stream is
    exactly INT64_MAX (every row: real entries beside the sort's pads, which carry the same h),
    INT64_MIN (beside random ones: T's h is the smallest value there is), or the h of the stream's
    own k-th smallest (the planted rows tie with T and with each other).  Lengths are no powers of two."""
    rng = np.random.default_rng(k + len(edge))
    lens = np.array([0, 1, k + 9, 777, 1500, 2049, 4097, 5001])
    ids, offs = ragged_ids(rng, lens)
    seed, base = 15, 2
    r0, r1 = _r01(oracle, k, seed, base, lens.size)
    rows, hashed = rows_of(ids, 16), hashes_of(ids).copy()
    for s in range(lens.size):
        a, b = int(offs[s]), int(offs[s + 1])
        if b - a < 2:
            continue
        if edge == "max":
            target, planted = HT.MAX, np.ones(b - a, dtype=bool)
        else:
            h = np.sort(_scramble(np.full(b - a, r0[s]), np.full(b - a, r1[s]), hashed[a:b]))
            target = HT.MIN if edge == "min" else int(h[min(k // 2, h.size - 1)])
            planted = ids[a:b] % 3 == 0  # by id: equal rows keep equal hashes
        hashed[a:b][planted] = HT.unscramble(int(r0[s]), int(r1[s]), target)
        got_h = _scramble(np.full(b - a, r0[s]), np.full(b - a, r1[s]), hashed[a:b])
        assert (got_h[planted] == target).all()
        if b - a >= 4097:  # the long streams hold more than k distinct planted rows
            assert np.unique(ids[a:b][planted]).size > k
    _check(_run(cuda, rows, offs, k, seed, base, hashes=hashed), expected_rows(rows, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("k", [64, 1024])
def test_worst_case_arrival(cuda, oracle, k):
    """Descending (h, row) under the stream's own (r0, r1): every element is admitted; ascending:
    nothing after the first k; one row repeated: one member."""
    S, n = 8, 20_000
    offs = np.arange(0, S * n + 1, n, dtype=np.int64)
    ids = np.arange(S * n)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 21, 5, S)
    sid = np.repeat(np.arange(S), n)
    w = rows.view(U64).reshape(-1, 2)
    asc = np.lexsort((w[:, 1], w[:, 0], _scramble(r0[sid], r1[sid], hashed), sid))
    desc = asc.reshape(S, n)[:, ::-1].reshape(-1)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    assert np.array_equal(want[0], rows[asc].reshape(S, n, 16)[:, :k])
    _check(_run(cuda, rows[desc], offs, k, 21, 5, hashes=hashed[desc]), want)
    _check(_run(cuda, rows[asc], offs, k, 21, 5, hashes=hashed[asc]), want)
    same = np.repeat(np.arange(S), n)
    got = _run(cuda, rows[same], offs, k, 21, 5, hashes=hashed[same])
    assert np.array_equal(got[2], np.ones(S, dtype=np.int64))
    _check(got, expected_rows(rows[same], hashed[same], offs, k, r0, r1))


@pytest.mark.parametrize("width", [16, 24])
def test_offsets_start_past_zero(cuda, oracle, width):
    """offsets[0] = 3: the rows before it are not read, and the entries' indices are absolute."""
    rng = np.random.default_rng(width)
    for k in (8, 300):
        lens = rng.integers(0, 2000, size=40)
        ids, offs = ragged_ids(rng, np.r_[3, lens])
        offs = offs[1:]
        rows, hashed = rows_of(ids, width), hashes_of(ids)
        r0, r1 = _r01(oracle, k, 1, 0, lens.size)
        _check(_run(cuda, rows, offs, k, 1, hashes=hashed), expected_rows(rows, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("width,uuid", [(16, True), (16, False), (24, False)])
def test_rows_base_at_8_mod_16(cuda, oracle, width, uuid):
    """Any 8-byte-aligned base is right: rows that start one word into an allocation (a UUID is then
    two 8-byte loads instead of one 16-byte load), and the same rows 16-byte aligned."""
    import torch

    from reservoir_amd import batch

    rng = np.random.default_rng(width)
    k = 70
    lens = rng.integers(0, 2000, size=50)
    ids, offs = ragged_ids(rng, lens)
    rows = rows_of(ids, width)
    hashed = uuid_hashcode_np(rows) if uuid else hashes_of(ids)
    r0, r1 = _r01(oracle, k, 8, 0, lens.size)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    words = torch.from_numpy(rows.view(np.int64).reshape(-1))
    shifted = torch.empty(words.numel() + 1, dtype=torch.int64, device=cuda)
    shifted[1:] = words.to(cuda)
    od = torch.from_numpy(offs).to(cuda)
    kw = {} if uuid else dict(hashes=torch.from_numpy(hashed).to(cuda))
    for off8 in (1, 0):
        rd = (shifted[1:] if off8 else shifted[1:].clone()).view(-1, width // 8)  # int64 rows: the same memory
        assert rd.data_ptr() % 16 == 8 * off8
        _check(tuple(t.cpu().numpy() for t in batch.distinct_segmented_rows(rd, od, k, seed=8, **kw)), want)


@pytest.mark.parametrize("S", [1, 2, 100_003])
def test_short_streams_and_grid_stride(cuda, oracle, S):
    rng = np.random.default_rng(S)
    lens = rng.integers(0, 21, size=S)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    ids = rng.integers(0, 30, size=int(offs[-1]))
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    r0, r1 = _r01(oracle, 8, 12, 2**63 - 50_000, S)  # the seed wraps past INT64_MAX inside the launch
    _check(_run(cuda, rows, offs, 8, 12, 2**63 - 50_000, hashes=hashed), expected_rows(rows, hashed, offs, 8, r0, r1))


def test_all_empty_launch(cuda):
    none = np.zeros((0, 16), dtype=np.uint8)
    for k in (8, 2000):
        gr, gh, gc = _run(cuda, none, np.zeros(51, dtype=np.int64), k, 1)
        assert gr.shape == (50, k, 16) and not gr.any() and not gh.any() and not gc.any()
    gr, gh, gc = _run(cuda, np.zeros((0, 24), dtype=np.uint8), np.zeros(4, dtype=np.int64), 8, 1,
                      hashes=np.zeros(0, dtype=np.int64))
    assert gr.shape == (3, 8, 24) and not gr.any() and not gh.any() and not gc.any()


def test_torch_stream_repeat_and_null_hashes(cuda, oracle):
    """A non-default torch stream; two runs bit-identical; out_hashes_dev = NULL through ctypes."""
    import torch

    from reservoir_amd import _native as N
    from reservoir_amd import batch

    rng = np.random.default_rng(8)
    k, S = 100, 100
    lens = rng.integers(0, 3000, size=S)
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    r0, r1 = _r01(oracle, k, 6, 0, S)
    want = expected_rows(rows, hashed, offs, k, r0, r1)
    rd, hd, od = (torch.from_numpy(a).to(cuda) for a in (rows, hashed, offs))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        a = batch.distinct_segmented_rows(rd, od, k, seed=6, hashes=hd)
        b = batch.distinct_segmented_rows(rd, od, k, seed=6, hash="precomputed", hashes=hd)
    st.synchronize()
    _check([t.cpu().numpy() for t in a], want)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    out = torch.full((S, k, 16), 0xFF, dtype=torch.uint8, device=cuda)
    cnt = torch.full((S,), -1, dtype=torch.int64, device=cuda)
    torch.cuda.synchronize()
    N.check(N.load().rsv_distinct_segmented_rows(
        C.c_void_p(rd.data_ptr()), C.c_void_p(hd.data_ptr()), C.c_void_p(od.data_ptr()), S, 16, k,
        N.HASH_PRECOMPUTED, 6, 0, C.c_void_p(out.data_ptr()), None, C.c_void_p(cnt.data_ptr()),
        C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(cnt.cpu().numpy(), want[2])


@pytest.mark.parametrize("k", [10, 700])
def test_single_handles_and_arrival_order(cuda, oracle, k):
    """Stream s is what one Sampler.distinct(k, key_type="bytes16", seed=seed_s, order="set") handle
    holds after the same rows, and shuffling each stream leaves the output unchanged."""
    import torch

    from reservoir_amd import Sampler

    rng = np.random.default_rng(k)
    S = 8
    lens = rng.integers(0, 6000, size=S)
    lens[1] = k // 2
    ids, offs = ragged_ids(rng, lens)
    rows, hashed = rows_of(ids, 16), hashes_of(ids)
    got = _run(cuda, rows, offs, k, 40, 7, hashes=hashed)
    perm = np.arange(ids.size)
    for s in range(S):
        rng.shuffle(perm[offs[s]:offs[s + 1]])
    _check(_run(cuda, rows[perm], offs, k, 40, 7, hashes=hashed[perm]), got)
    for s in range(S):
        a, b = int(offs[s]), int(offs[s + 1])
        d = Sampler.distinct(k, key_type="bytes16", seed=40 + 7 + s, order="set")(hash=lambda b: 0)
        if b > a:
            d.sample_all(torch.from_numpy(rows[a:b]).to(cuda), hashes=torch.from_numpy(hashed[a:b]).to(cuda))
        held = np.asarray(d.result()).reshape(-1, 16)
        m = int(got[2][s])
        assert held.shape[0] == m, s
        assert sorted(bytes(r) for r in held) == sorted(bytes(r) for r in got[0][s, :m]), s


def test_bad_arguments_raise(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch

    rows = torch.zeros((10, 16), dtype=torch.uint8, device=cuda)
    offs = torch.tensor([0, 10], dtype=torch.int64, device=cuda)
    hs = torch.zeros(10, dtype=torch.int64, device=cuda)
    f = batch.distinct_segmented_rows
    with pytest.raises(IllegalArgumentException):
        f(rows, offs, 0, seed=1)
    with pytest.raises(ReservoirError, match="4096"):
        f(rows, offs, 4097, seed=1)
    with pytest.raises(IllegalArgumentException):
        f(rows, offs, 4, seed=1, hash="md5")
    with pytest.raises(IllegalArgumentException):
        f(rows.cpu(), offs, 4, seed=1)
    with pytest.raises(IllegalArgumentException):
        f(rows.view(-1), offs, 4, seed=1)  # not 2-D
    with pytest.raises(IllegalArgumentException):
        f(rows, offs.to(torch.int32), 4, seed=1)
    with pytest.raises(IllegalArgumentException):
        f(rows, offs, 4, seed=1, hashes=hs[:9])  # one hash per row
    with pytest.raises(IllegalArgumentException):
        f(rows[:, :12], offs, 4, seed=1, hashes=hs)  # 12-byte rows
    with pytest.raises(NullPointerException):
        f(rows, offs, 4, seed=1, hash="precomputed")
    with pytest.raises(ReservoirError):
        f(torch.zeros((10, 24), dtype=torch.uint8, device=cuda), offs, 4, seed=1)  # UUID.hashCode of 24 bytes
    with pytest.raises(ReservoirError, match="rsv_distinct_segmented"):
        f(torch.zeros((10, 8), dtype=torch.uint8, device=cuda), offs, 4, seed=1, hashes=hs)
