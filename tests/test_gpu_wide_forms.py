"""The byte-key element sampler (`Sampler(k, key_type="bytesW")`) at every form, width and limit.

A byte-key handle takes its own kernel at every step (rsv_elements.hip): resolve_wide_kernel in its
publishing (one workgroup of 64..1024 threads, k <= 8192 and k * W <= 2^20 bytes) and its grid
launch, the byte loops of resolve_indices_kernel / resolve_indices_publish_kernel / fill_slots_kernel
(host batches), merge_kernel<StridedWideParts>, export_packed_wide_kernel, merge_kernel<PackedWideRows>, the wide
branch of init_slots_kernel and publish_kernel over m * W bytes.  Above either limit result() no
longer waits for a published generation: k > 8192 publishes at result(), k * W > 2^20 copies through a
pinned buffer.

Every key is derived from its global index (wide_rows._rows), so the expected reservoir is the same
derivation applied to the oracle's last writers -- `oracle.algo_r_last_writers` for philox_r,
`oracle.AlgoL(...).sample_all_iota` for java_l -- and W zero bytes where a slot has no writer.
Everything is compared exactly.  The tests do not inspect which kernel ran.
"""
import functools
import math

import numpy as np
import pytest

from test_gpu_staging import _stage_all
from wide_rows import _rows, _rows_at

pytestmark = pytest.mark.gpu

SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03  # all four 32-bit words nonzero and distinct
SEED_L = SEED - 2**64                                # the same 64 bits as a Java long (java_l)
N = 300_000
N_KEYS = 400_000                                     # the shared key table: rows of ids 0 .. N_KEYS - 1


@functools.lru_cache(maxsize=None)
def _writers(k, i0, n):
    from oracle import oracle

    if n <= 0:
        w = np.full(k, -1, dtype=np.int64)
    else:
        w = oracle.algo_r_last_writers(SEED, SID, k, i0, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _algo_l(k, n):
    """The reference's Algorithm L over the indices 0 .. n - 1: the winning index of each slot."""
    from oracle import oracle

    ref = oracle.AlgoL(k, SEED_L)
    ref.sample_all_iota(0, n)
    w = ref.result()
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _host_keys(width):
    keys = _rows(np.arange(N_KEYS, dtype=np.int64), width)
    keys.setflags(write=False)
    return keys


@pytest.fixture(scope="module")
def dev_keys(cuda):
    """width -> the key table as a (N_KEYS, width) uint8 device tensor, built once per width."""
    import torch

    cache = {}

    def get(width):
        if width not in cache:
            cache[width] = torch.from_numpy(_host_keys(width).copy()).to(cuda)
        return cache[width]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _sampler(k, width, **kw):
    from reservoir_amd import Sampler

    return Sampler(k, seed=SEED, stream_id=SID, key_type=f"bytes{width}", **kw)()


def _check_state(torch, cuda, s, want_idx, width, count=None):
    """export_state's idx and rows (empty slots: -1 and zero bytes) and result()'s min(count, k) rows."""
    want = _rows_at(want_idx, width)
    gidx, grows, _, gn = s.export_state(cuda)
    torch.cuda.synchronize()
    assert gn == want_idx.size and tuple(grows.shape) == (want_idx.size, width)
    assert np.array_equal(gidx.cpu().numpy(), want_idx)
    assert np.array_equal(grows.cpu().numpy(), want)
    m = want_idx.size if count is None else min(count, want_idx.size)
    got = s.result()
    assert got.dtype == np.uint8 and got.shape == (m, width)
    assert np.array_equal(got, want[:m])


# ---- 1. every resolve form over device batches -------------------------------------------------------
FORMS = [  # (W, k)
    (16, 1), (16, 63), (16, 64), (16, 65),         # one wave, and 64 -> 128 threads
    (24, 1023), (24, 1024), (24, 1025),            # one 1024-thread workgroup loops from 1025; 6 words per row
    (40, 100), (40, 2049),                         # 10 words per row
    (16, 8192), (16, 8193),                        # slot limit: fused publication, then publish at result()
    (128, 8192),                                   # both limits met exactly (2^20 bytes)
    (256, 4096), (256, 4097),                      # byte limit exactly, then one row over it: pinned D2H copy
    (256, 8192),                                   # inside the slot limit but 2 MiB
]


@pytest.mark.parametrize("reusable", [False, True], ids=["single_use", "reusable"])
@pytest.mark.parametrize("forked", [False, True], ids=["one_stream", "forked"])
@pytest.mark.parametrize("width,k", FORMS)
def test_wide_resolve_forms(cuda, oracle, dev_keys, width, k, forked, reusable):
    """Device batches cut at [0, k // 2, k + 37, 150_000 + k, N, N]: a fresh batch inside the fill
    (m < k rows published), one crossing k, two past k (not fresh: untouched slots are re-published
    from the slot rows), an empty tail.  A reusable handle's result() is read after every batch and
    must be the oracle's reservoir of that prefix; at the end export_state and result_device too.
    forked: the resolve runs on a second stream (set_resolve_stream)."""
    import torch

    from reservoir_amd import IllegalStateException

    kd = dev_keys(width)
    cuts = [0, k // 2, k + 37, 150_000 + k, N, N]
    batches = [kd[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    if width in (24, 40):  # rows that are only 8-byte aligned
        assert any(t.data_ptr() % 16 == 8 for t in batches)
    s = _sampler(k, width, reusable=reusable)
    if forked:
        side = torch.cuda.Stream(device=cuda)
        s.set_stream(torch.cuda.current_stream(cuda).cuda_stream)
        s.set_resolve_stream(side.cuda_stream)
    for t, c in zip(batches, cuts[1:]):
        s.sample_all(t)
        if reusable:  # the published generation of every batch, not only the last
            m = min(c, k)
            got = s.result()
            assert got.shape == (m, width), (c, got.shape)
            assert np.array_equal(got, _rows_at(_writers(k, 0, c), width)[:m]), c
    assert s.count == N
    want_idx = _writers(k, 0, N)
    assert (want_idx >= 0).all()
    want = _rows_at(want_idx, width)
    if reusable:
        _check_state(torch, cuda, s, want_idx, width)
        out = torch.zeros((k, width), dtype=torch.uint8, device=cuda)
        assert s.result_device(out) == k
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        s.close()
    else:
        got = s.result()
        assert got.dtype == np.uint8 and got.shape == (k, width) and np.array_equal(got, want)
        with pytest.raises(IllegalStateException):
            s.sample(_host_keys(width)[0].tobytes())
        s.close()


# ---- 2. a first batch on a recycled slot block -------------------------------------------------------
@pytest.mark.parametrize("feed", ["device", "host"])
@pytest.mark.parametrize("width,k", [(16, 64), (24, 1025), (16, 8193), (256, 4097)])
def test_wide_first_batch_on_recycled_block(cuda, oracle, dev_keys, width, k, feed):
    """Handle A leaves a nonzero row in every slot and is closed: its slot block goes to the
    clean-slot pool (as long as the pool has room for it).  Handle B of the same (k, W) takes the
    block, seeks past the fill and samples one batch: the slots without a writer must read idx -1
    and zero bytes, which only the `fresh` branches of the resolve kernels write."""
    import torch

    kd = dev_keys(width)
    a = _sampler(k, width)
    a.sample_all(kd[: 3 * k])
    first = a.result()
    assert first.shape == (k, width) and np.array_equal(first, _rows_at(_writers(k, 0, 3 * k), width))
    assert first.any(axis=1).all()  # every slot of the block holds a nonzero row
    a.close()
    del a

    i0 = min(40 * k + 3, 100_003)
    n = i0
    want_idx = _writers(k, i0, n)
    written = int((want_idx >= 0).sum())
    assert written > 0 and written < k, "both kinds of slot must exist"
    assert (written, k - written) == {64: (35, 29), 1025: (516, 509), 4097: (2044, 2053), 8193: (4059, 4134)}[k]
    b = _sampler(k, width)
    b.seek(i0)
    b.sample_all(kd[i0: i0 + n] if feed == "device" else _host_keys(width)[i0: i0 + n])
    assert b.count == i0 + n
    _check_state(torch, cuda, b, want_idx, width)
    b.close()


# ---- 3. every way in, mixed, on one handle -----------------------------------------------------------
def _expected_changes(k, base, n):
    """The engine's estimate of the slots a batch of n elements at [base, base + n) changes."""
    fill = min(max(k - base, 0), n)
    lo, hi = max(base, k), base + n
    ev = k * math.log(hi / lo) if hi > lo else 0.0
    return min(fill + ev, min(n, k))


@pytest.mark.parametrize("engine,width,k", [("philox_r", 16, 100), ("philox_r", 40, 1024), ("philox_r", 40, 9000),
                                            ("java_l", 16, 100), ("java_l", 40, 9000)])
def test_wide_every_way_in(cuda, oracle, dev_keys, engine, width, k):
    """One stream in global-index order through every entry point of one reusable handle, whose
    result() is compared with the oracle's reservoir of the prefix after steps 1, 2, 4, 5 and 7 (so a
    wrong row from a host or staged batch is seen before a later batch overwrites its slot):

      1. host batch of k // 2 + 1 rows (ends inside the fill)        count -> c1 = k // 2 + 1
      2. device batch of 3 k + 11 rows                               count -> c2 = c1 + 3 k + 11
      3. staged batch of k // 4 + 5 rows, flushed by step 4          count -> c3
      4. host batch of 2 k + 3 rows                                  count -> c4
      5. staged batch of 20 k rows, flushed by the result() after it
      6. three sample(row) calls, flushed by step 7
      7. device batch of 50_000 + k rows

    A staged flush of n rows at count c is resolved in place from the pinned buffer when
    expected_changes * 16 <= n, with expected_changes = min(k ln((c + n) / c), n, k) past the fill.
    Step 3, k = 100: c2 = 362, n = 30: 100 ln(392 / 362) = 7.96, x 16 = 127 > 30: copied; at any k
    the batch is ~k / 4 rows at ~3.5 k: k ln(3.75 / 3.5) x 16 = 1.1 k > k / 4.  Step 5: n = 20 k and
    expected_changes <= k, so 16 k <= n: in place.  The test asserts both inequalities on its own
    arithmetic and does not inspect which form ran.  k = 9000 takes resolve_indices_kernel + a
    device-to-host copy + fill_slots_kernel for its host batches; under java_l the staged batches
    carry their events in the pinned event buffers."""
    import torch

    from reservoir_amd import Sampler, _native as NL

    L = NL.load()
    kd, kh = dev_keys(width), _host_keys(width)
    kv = kh.view(f"V{width}").reshape(-1)
    sizes = [k // 2 + 1, 3 * k + 11, k // 4 + 5, 2 * k + 3, 20 * k, 3, 50_000 + k]
    at = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    total = at[-1]
    assert total <= N_KEYS and 20 * k <= 1 << 20
    assert _expected_changes(k, at[2], sizes[2]) * 16 > sizes[2]    # step 3: copied
    assert _expected_changes(k, at[4], sizes[4]) * 16 <= sizes[4]   # step 5: in place
    if engine == "philox_r":
        s = _sampler(k, width, reusable=True)
    else:
        s = Sampler(k, seed=SEED_L, key_type=f"bytes{width}", engine=engine, reusable=True)()

    def check(c):
        m = min(c, k)
        want = _rows_at(_writers(k, 0, c), width)[:m] if engine == "philox_r" else _rows(_algo_l(k, c), width)
        got = s.result()
        assert s.count == c and got.shape == (m, width), c
        assert np.array_equal(got, want), c

    s.sample_all(kh[at[0]:at[1]])
    check(at[1])
    s.sample_all(kd[at[1]:at[2]])
    check(at[2])
    _stage_all(L, NL, s.handle, kv[at[2]:at[3]])
    s.sample_all(kh[at[3]:at[4]])
    check(at[4])
    _stage_all(L, NL, s.handle, kv[at[4]:at[5]])
    check(at[5])
    for row in kh[at[5]:at[6]]:
        s.sample(row.tobytes())
    s.sample_all(kd[at[6]:at[7]])
    check(total)
    if engine == "philox_r":
        _check_state(torch, cuda, s, _writers(k, 0, total), width)
    s.close()


# ---- 4. java_l with byte keys ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 100, 1024, 9000])
@pytest.mark.parametrize("width", [16, 40])
def test_wide_java_l(cuda, oracle, dev_keys, width, k):
    """The reference's Algorithm L (host event chain + replay_kernel) in front of the wide resolve:
    two device batches cut at 12_345, then one host batch of the rest."""
    from reservoir_amd import Sampler

    n = 400_000
    kd, kh = dev_keys(width), _host_keys(width)
    s = Sampler(k, seed=SEED_L, key_type=f"bytes{width}", engine="java_l")()
    s.sample_all(kd[:12_345])
    s.sample_all(kd[12_345:200_000])
    s.sample_all(kh[200_000:n])
    assert s.count == n
    got = s.result()
    assert got.dtype == np.uint8 and got.shape == (k, width)
    assert np.array_equal(got, _rows(_algo_l(k, n), width))
    s.close()


# ---- 5. state exchange -------------------------------------------------------------------------------
def _bounds(n, parts):
    """An index-range split of [0, n) into `parts` ranges; with four parts the second one is empty."""
    if parts == 4:
        b = np.linspace(0, n, 4).astype(np.int64)
        return [int(b[0]), int(b[1]), int(b[1]), int(b[2]), int(b[3])]
    return [int(x) for x in np.linspace(0, n, parts + 1).astype(np.int64)]


@pytest.mark.parametrize("way", ["state", "packed"])
@pytest.mark.parametrize("parts", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 255, 256, 257, 8192, 8193])
@pytest.mark.parametrize("width", [16, 24, 256])
def test_wide_state_exchange(cuda, oracle, dev_keys, width, k, parts, way):
    """An index-range split of n = 3 k + 7 and of n = k - 5 elements (the fill slots then come from
    different parts and m < k): every part seeks to its range, samples it and exports its state; the
    last part merges the others and must equal one oracle run over the whole stream.  way = state:
    export_state / merge_state with idx [P - 1, L] and rows [P - 1, L, W]; way = packed: export_packed
    / merge_packed.  With four parts one range is empty (its state is all -1), L = k + 3 and the packed
    rows are 5 words wider than packed_width; the padding holds indices that would win every slot."""
    import torch

    kd = dev_keys(width)
    pad = 3 if parts == 4 else 0
    extra = 5 if parts == 4 else 0
    for n in (3 * k + 7, k - 5):
        if n <= 0:
            continue
        bounds = _bounds(n, parts)
        last = None
        L = k + pad
        if way == "state":
            idx = torch.full((parts - 1, L), 2**62, dtype=torch.int64, device=cuda)
            rows = torch.full((parts - 1, L, width), 0xEE, dtype=torch.uint8, device=cuda)
        else:
            pw = k * (1 + width // 8)
            packed = torch.full((parts - 1, pw + extra), 2**62, dtype=torch.int64, device=cuda)
        for p in range(parts):
            s = _sampler(k, width)
            s.seek(bounds[p])
            s.sample_all(kd[bounds[p]:bounds[p + 1]])
            if p == parts - 1:
                last = s
                break
            want_p = _writers(k, bounds[p], bounds[p + 1] - bounds[p])
            if bounds[p] == bounds[p + 1]:
                assert (want_p == -1).all()
            if way == "state":
                gi, gr, _, gn = s.export_state(cuda)
                torch.cuda.synchronize()
                assert gn == k and np.array_equal(gi.cpu().numpy(), want_p)
                assert np.array_equal(gr.cpu().numpy(), _rows_at(want_p, width))
                idx[p, :k] = gi
                rows[p, :k] = gr
            else:
                assert s.packed_width == pw
                s.export_packed(packed[p])
                torch.cuda.synchronize()
                row = packed[p].cpu().numpy()
                assert np.array_equal(row[:k], want_p)
                assert np.array_equal(row[k:pw].view(np.uint8).reshape(k, width), _rows_at(want_p, width))
                assert (row[pw:] == 2**62).all()
            s.close()
        if way == "state":
            last.merge_state(idx, rows, torch.zeros((max(parts - 1, 1), L), dtype=torch.int64, device=cuda),
                             [k] * (parts - 1), n)
        else:
            last.merge_packed(packed, n)
        assert last.count == n
        _check_state(torch, cuda, last, _writers(k, 0, n), width, count=n)
        last.close()


@pytest.mark.parametrize("key_type", ["long", "bytes16"])
def test_zero_part_merge_drops_short_publication(cuda, oracle, dev_keys, key_type):
    """A reusable handle that has published m < k rows (a batch inside the fill), then merge_packed
    with a zero-part rows tensor and a total_count above k: result() now holds k rows -- its own for
    the filled slots, zeros beyond -- so the publication of m rows must not be served again (rsv_seek
    drops it when the count crosses k; the merge must too).  A first handle of the same shape leaves k
    nonzero rows in the pooled result buffer the second one is likely to take."""
    import torch

    from reservoir_amd import Sampler

    k, m = 100, 50
    if key_type == "long":
        keys = np.arange(1, 4 * k + 1, dtype=np.int64) * 0x0101010101010101
        kd = torch.from_numpy(keys).to(cuda)
        want = np.zeros(k, dtype=np.int64)
        want[:m] = keys[:m]
    else:
        kd = dev_keys(16)
        want = np.zeros((k, 16), dtype=np.uint8)
        want[:m] = _host_keys(16)[:m]
    s0 = Sampler(k, seed=SEED, stream_id=SID, key_type=key_type, reusable=True)()
    s0.sample_all(kd[: 4 * k])
    assert s0.result().reshape(k, -1).any(axis=1).all()
    s0.close()
    s = Sampler(k, seed=SEED, stream_id=SID, key_type=key_type, reusable=True)()
    s.sample_all(kd[:m])
    assert np.array_equal(s.result(), want[:m])
    s.merge_packed(torch.zeros((0, s.packed_width), dtype=torch.int64, device=cuda), k + 50)
    assert s.count == k + 50
    got = s.result()
    assert got.shape == want.shape and np.array_equal(got, want)
    s.close()


# ---- 6. the grid-stride loops ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(cuda):
    """k = 2^22 + 300 slots of 16-byte keys, n = k + 200_000: more slots than the 256 x 16384 threads of
    the widest resolve, init, index-resolve and fill launches, so their grid-stride loops take a second
    trip.  ~70 MB of rows and 67 MB of slots."""
    import torch

    k = (1 << 22) + 300
    n = k + 200_000
    keys = _rows(np.arange(n, dtype=np.int64), 16)
    want_idx = _writers(k, 0, n)
    assert int((want_idx >= k).sum()) == 190_928  # slots overwritten after the fill
    kd = torch.from_numpy(keys).to(cuda)
    yield k, n, keys, kd, want_idx
    del kd
    _writers.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("feed", ["device", "host"])
def test_wide_grid_stride(cuda, oracle, big, feed):
    """Cuts [0, 2^22 + 100, n]: a fresh batch that ends inside the fill, past the first trip of the
    loops, then one that finishes the fill and overwrites 190_928 slots.  Measured on an MI355X: 0.2 s per
    case and 0.2 s for the shared fixture (the oracle's run, the expected rows and the 67 MB copies)."""
    import torch

    k, n, keys, kd, want_idx = big
    src = kd if feed == "device" else keys
    cuts = [0, (1 << 22) + 100, n]
    s = _sampler(k, 16)
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.sample_all(src[a:b])
    assert s.count == n
    _check_state(torch, cuda, s, want_idx, 16)
    s.close()
