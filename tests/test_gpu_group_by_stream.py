"""batch.group_by_stream (rsv_group_by_stream) against numpy on the host, bit for bit, for int64 and int32 ids:

    order   == np.argsort(ids mapped, kind="stable"), ids outside [0, S) mapped to S
    offsets == np.searchsorted(sorted mapped ids, arange(S + 1))

The shapes are those at which a radix partition goes wrong: around a wave (64), a tile (4096) and several tiles; S
around every change of the pass count (255 | 256: one pass to two, 65535 | 65536: two to three, 2^24 - 1 | 2^24:
three to four) and of the digit width inside a pass count; one run that crosses every wave and tile boundary;
descending ids; every row in every wave; a skewed draw; dropped ids between kept ones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64, I32 = np.iinfo(np.int64), np.iinfo(np.int32)


def _reference(ids, S):
    mapped = np.where((ids >= 0) & (ids < S), ids, S).astype(np.int64)
    order = np.argsort(mapped, kind="stable")
    return np.searchsorted(mapped[order], np.arange(S + 1)).astype(np.int64), order.astype(np.int32)


def _run(cuda, ids, S):
    import torch

    from reservoir_amd import batch

    offsets, order = batch.group_by_stream(torch.from_numpy(ids).to(cuda), S)
    assert offsets.dtype == torch.int64 and offsets.shape == (S + 1,) and offsets.device == cuda
    assert order.dtype == torch.int32 and order.shape == (ids.size,) and order.device == cuda
    return offsets.cpu().numpy(), order.cpu().numpy()


def _check(cuda, ids, S, what=""):
    for dtype in (np.int64, np.int32):
        x = ids.astype(dtype)
        want = _reference(x, S)
        got = _run(cuda, x, S)
        assert np.array_equal(got[0], want[0]), (what, dtype, np.flatnonzero(got[0] != want[0])[:8])
        assert np.array_equal(got[1], want[1]), (what, dtype, np.flatnonzero(got[1] != want[1])[:8])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 100_003])
def test_sizes(cuda, n):
    rng = np.random.default_rng(n)
    _check(cuda, rng.integers(0, 37, size=n), 37, n)


def test_one_row(cuda):
    _check(cuda, np.zeros(5000, np.int64), 1)
    _check(cuda, np.arange(-3, 4997), 1)  # mostly dropped


@pytest.mark.parametrize("S", [2, 127, 128, 255, 256, 257, 511, 512, 65_535, 65_536, 65_537, (1 << 18) - 1, 1 << 18])
def test_row_counts_around_the_digit_boundaries(cuda, S):
    rng = np.random.default_rng(S)
    ids = rng.integers(0, S, size=20_011)
    ids[:4] = [S - 1, 0, S - 1, S - 2 if S > 1 else 0]  # the top rows are there
    _check(cuda, ids, S, S)


@pytest.mark.parametrize("S", [(1 << 20) + 3, (1 << 24) - 1, 1 << 24])
def test_sparse_over_many_rows(cuda, S):
    """5000 elements over millions of rows (the top digit partial): three and four passes."""
    rng = np.random.default_rng(7)
    ids = rng.integers(0, S, size=5000)
    ids[:3] = [S - 1, 0, S - 1]
    _check(cuda, ids, S, S)


def test_all_ids_equal(cuda):
    """One run crosses every wave and tile boundary: positions must come out ascending."""
    for S, r in ((37, 11), (300, 299), (70_000, 65_536)):
        _check(cuda, np.full(20_011, r, np.int64), S, (S, r))


def test_descending_ids(cuda):
    _check(cuda, np.arange(9999, -1, -1), 10_000)
    _check(cuda, np.arange(9999, -1, -1) // 7, 1500)


def test_every_row_in_every_wave(cuda):
    for S in (37, 64, 300):
        _check(cuda, np.arange(30_011) % S, S, S)


def test_zipf_skew(cuda):
    rng = np.random.default_rng(3)
    for S in (37, 5000):
        ids = np.minimum(rng.zipf(1.2, size=50_021) - 1, S - 1)
        _check(cuda, ids, S, S)


@pytest.mark.parametrize("S", [37, 256, 70_000])
def test_out_of_range_ids_between_valid_ones(cuda, S):
    import torch

    from reservoir_amd import batch

    rng = np.random.default_rng(S)
    n = 12_345
    for dtype, info in ((np.int64, I64), (np.int32, I32)):
        ids = rng.integers(0, S, size=n).astype(dtype)
        bad = np.array([-1, S, info.min, info.max, S + 1, -S - 1], dtype=dtype)
        where = rng.choice(n, size=n // 3, replace=False)
        ids[where] = bad[rng.integers(0, bad.size, size=where.size)]
        ids[[0, n - 1]] = [-1, info.max]
        want = _reference(ids, S)
        got = _run(cuda, ids, S)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), dtype
        kept = int(got[0][S])
        assert kept == int(((ids >= 0) & (ids < S)).sum())
        assert np.array_equal(np.sort(got[1]), np.arange(n))  # a permutation
        assert np.array_equal(got[1][kept:], np.flatnonzero((ids < 0) | (ids >= S)))  # the dropped, in arrival order
        # all dropped
        offs, order = batch.group_by_stream(torch.from_numpy(np.full(100, info.min, dtype)).to(cuda), S)
        assert not offs.any().item() and np.array_equal(order.cpu().numpy(), np.arange(100))


def test_empty_batch_writes_every_offset(cuda):
    import torch

    from reservoir_amd import batch

    for dtype in (torch.int64, torch.int32):
        offs, order = batch.group_by_stream(torch.empty(0, dtype=dtype, device=cuda), 1000)
        assert offs.shape == (1001,) and not offs.any().item() and order.numel() == 0


def test_two_calls_give_identical_tensors(cuda):
    import torch

    from reservoir_amd import batch

    rng = np.random.default_rng(11)
    ids = torch.from_numpy(np.minimum(rng.zipf(1.3, size=100_003) - 1, 4999)).to(cuda)
    a = batch.group_by_stream(ids, 5000)
    b = batch.group_by_stream(ids, 5000)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_on_a_side_stream_without_synchronisation(cuda):
    """The call and the work that consumes it on one non-default stream, nothing in between."""
    import torch

    from reservoir_amd import batch

    rng = np.random.default_rng(5)
    ids_np = rng.integers(-5, 305, size=70_001)
    keys_np = rng.integers(I64.min, I64.max, size=ids_np.size)
    ids, keys = torch.from_numpy(ids_np).to(cuda), torch.from_numpy(keys_np).to(cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        spin = torch.ones(1 << 22, device=cuda)
        for _ in range(8):  # queued work ahead of the call
            spin = spin * 1.0001
        offs, order = batch.group_by_stream(ids, 300)
        grouped = keys.index_select(0, order)  # consumes order on the same stream
        sizes = offs[1:] - offs[:-1]
    side.synchronize()
    want_offs, want_order = _reference(ids_np, 300)
    assert np.array_equal(offs.cpu().numpy(), want_offs) and np.array_equal(order.cpu().numpy(), want_order)
    assert np.array_equal(grouped.cpu().numpy(), keys_np[want_order])
    assert np.array_equal(sizes.cpu().numpy(), np.diff(want_offs))


def test_argument_checks(cuda):
    import torch

    from reservoir_amd import batch
    from reservoir_amd._native import IllegalArgumentException

    ids = torch.zeros(4, dtype=torch.int64, device=cuda)
    with pytest.raises(IllegalArgumentException, match="device tensor"):
        batch.group_by_stream(ids.cpu(), 3)
    with pytest.raises(IllegalArgumentException, match="int64/int32"):
        batch.group_by_stream(ids.to(torch.int16), 3)
    with pytest.raises(IllegalArgumentException, match="1-D"):
        batch.group_by_stream(ids.view(2, 2), 3)
    with pytest.raises(IllegalArgumentException, match="num_streams"):
        batch.group_by_stream(ids, 0)
