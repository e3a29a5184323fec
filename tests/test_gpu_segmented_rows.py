"""Segmented Sampler.apply over byte keys (K2 rows: rsv_sample_segmented_rows / _update / _merge,
batch.sample_segmented_rows and batch.SegmentedSamplerRows).  Everything is bit-exact: slot j of stream
s holds rows[offsets[s] + w] for w = oracle.algo_r_last_writers(seed, stream_base + s, k, 0, n, 1)[j]
and zeros where w < 0, however the stream is cut, reordered with bases or assembled by merge.  The rows
are built so that every 8-byte word of a row differs from every word of every other row (and from 0): a
gather that mixes granules of two rows, repeats one, or leaves one out cannot pass."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_segmented_state as LK  # the Long-key cases' lengths, forced cuts and pieces

pytestmark = pytest.mark.gpu

SEED, BASE = 31, 2**33 + 5


def _rows(n, W, first=0):
    """Rows first .. first + n of W bytes: word c of row r is (32 r + c + 1) * an odd constant mod 2^64."""
    r = np.arange(first, first + n, dtype=np.uint64)[:, None] * np.uint64(32)
    words = (r + np.arange(W // 8, dtype=np.uint64)[None, :] + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return np.ascontiguousarray(words).view(np.uint8).reshape(n, W)


def _expect(rows, offs, widx):
    """(S, k, W): the rows at the last writers, zeros where there is none."""
    at = np.where(widx >= 0, widx + offs[:-1, None], 0)
    return np.where((widx >= 0)[:, :, None], rows[at], 0).astype(np.uint8)


def _dev(torch, cuda, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(cuda)


@functools.lru_cache(maxsize=None)
def _stateless_case(k):
    """Ragged lengths (0, 1, k-1, k, k+1 and 4096 forced) and their last writers, shared by the widths."""
    from oracle import oracle

    S = 60 if k >= 512 else 300
    rng = np.random.default_rng(8000 + k)
    lens, _ = LK._lengths(k, S, 4 * k + 5000 if k >= 512 else 5000, rng)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    widx = LK._last_writers(oracle, SEED, BASE, k, lens)
    for a in (lens, offs, widx):
        a.setflags(write=False)
    return lens, offs, widx


@pytest.mark.parametrize("k", [1, 8, 64, 100, 512, 1030])
@pytest.mark.parametrize("W", [16, 24, 256])
def test_stateless(cuda, oracle, W, k):
    """Widths x k: the deferred-gather range (k W / 16 <= 64), the plain wave form, and the workgroup
    form; W = 24 moves 8-byte granules with every other row off a 16-byte boundary."""
    import torch

    from reservoir_amd import batch

    lens, offs, widx = _stateless_case(k)
    rows = _rows(int(offs[-1]), W)
    out, cnt = batch.sample_segmented_rows(_dev(torch, cuda, rows), _dev(torch, cuda, offs), k, SEED, BASE)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (lens.size, k, W)
    assert np.array_equal(cnt.cpu().numpy(), np.minimum(lens, k))
    assert np.array_equal(out.cpu().numpy(), _expect(rows, offs, widx)), (W, k)


def test_granule_follows_alignment(cuda, oracle):
    """W = 32 from a 16-byte-aligned base moves 16-byte granules; from a base that is only 8-byte aligned
    the same rows must go through the 8-byte gather (k = 512: the workgroup form)."""
    import torch

    from reservoir_amd import batch

    k, W = 512, 32
    lens, offs, widx = _stateless_case(k)
    rows = _rows(int(offs[-1]), W)
    want = _expect(rows, offs, widx)
    pad = torch.empty(rows.size + 8, dtype=torch.uint8, device=cuda)
    for shift in (0, 8):
        r = pad[shift:shift + rows.size].view(-1, W)
        r.copy_(_dev(torch, cuda, rows))
        out, _ = batch.sample_segmented_rows(r, _dev(torch, cuda, offs), k, SEED, BASE)
        assert np.array_equal(out.cpu().numpy(), want), shift


def test_int64_view(cuda, oracle):
    """int64 (n, W / 8) rows are the same memory as uint8 (n, W)."""
    import torch

    from reservoir_amd import batch

    k, W = 100, 24
    lens, offs, widx = _stateless_case(k)
    rows = _rows(int(offs[-1]), W)
    out, cnt = batch.sample_segmented_rows(_dev(torch, cuda, rows.view(np.int64)), _dev(torch, cuda, offs), k, SEED, BASE)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (lens.size, k, W)
    assert np.array_equal(out.cpu().numpy(), _expect(rows, offs, widx))
    st = batch.SegmentedSamplerRows(lens.size, k, W, SEED, BASE, device=cuda)
    st.update(_dev(torch, cuda, rows.view(np.int64)), _dev(torch, cuda, offs))
    assert np.array_equal(st.idx.cpu().numpy(), widx)
    assert torch.equal(torch.where((st.idx >= 0)[:, :, None], st.rows, torch.zeros_like(st.rows)), out)


def test_global_scratch_table(cuda, oracle):
    """k = 40000: the winner table no longer fits LDS and lives in the global scratch; run twice, so the
    second launch finds the table as the first left it (zero)."""
    import torch

    from reservoir_amd import batch

    k, S, n, W = 40000, 3, 120000, 16
    offs = np.arange(S + 1, dtype=np.int64) * n
    widx = LK._last_writers(oracle, SEED, BASE, k, np.full(S, n))
    rows = _rows(S * n, W)
    want = _expect(rows, offs, widx)
    rd, od = _dev(torch, cuda, rows), _dev(torch, cuda, offs)
    for _ in range(2):
        out, cnt = batch.sample_segmented_rows(rd, od, k, SEED, BASE)
        assert np.array_equal(out.cpu().numpy(), want)
        assert cnt.tolist() == [k] * S


_FIFO_CASE = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from oracle import oracle
from reservoir_amd import batch
import test_gpu_segmented_rows as T
cuda = torch.device("cuda", 0)
for k, W in ((64, 16), (256, 24), (1000, 16)):
    rng = np.random.default_rng(500 + k)
    lens = rng.integers(0, 20_000, size=100)
    lens[:4] = [k, k + 1, 4096, 19_999]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    rows = T._rows(int(offs[-1]), W)
    widx = np.stack([oracle.algo_r_last_writers(31, 77 + s, k, 0, int(n), 1) for s, n in enumerate(lens)])
    out, cnt = batch.sample_segmented_rows(torch.from_numpy(rows).to(cuda), torch.from_numpy(offs).to(cuda), k, 31, 77)
    assert np.array_equal(out.cpu().numpy(), T._expect(rows, offs, widx)), k
    assert np.array_equal(cnt.cpu().numpy(), np.minimum(lens, k)), k
print("fifo overflow ok")
"""


def test_fifo_overflow_rounds(cuda, oracle):
    """RSV_K2_FIFO_CAP = 128 sends dense iterations through the ballot-round path under the rows kernels
    (wave and workgroup form).  The engine reads the variable once per process: a child process sets it."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, RSV_K2_FIFO_CAP="128")
    r = subprocess.run([sys.executable, "-c", _FIFO_CASE.format(root=os.path.dirname(tests), tests=tests)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "fifo overflow ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_rows_past_4gib(cuda, oracle):
    """A stream 2^28 rows into a 16-byte-row tensor starts at byte 2^32: the row address is 64-bit,
    stateless and resumed.  Only the stream's 6000 rows are filled."""
    import torch

    from reservoir_amd import batch

    if torch.cuda.mem_get_info(cuda)[0] < 6 * 2**30:
        pytest.skip("needs 6 GiB of free device memory")
    first, n, k, W = 2**28, 6000, 64, 16
    big = torch.empty((first + n, W), dtype=torch.uint8, device=cuda)
    rows = _rows(n, W, first=first)
    big[first:] = _dev(torch, cuda, rows)
    offs = np.array([first, first + n], dtype=np.int64)
    widx = LK._last_writers(oracle, SEED, BASE, k, [n])
    want = _expect(rows, np.array([0, n]), widx)
    out, cnt = batch.sample_segmented_rows(big, _dev(torch, cuda, offs), k, SEED, BASE)
    assert np.array_equal(out.cpu().numpy(), want) and cnt.tolist() == [k]
    st = batch.SegmentedSamplerRows(1, k, W, SEED, BASE, device=cuda).update(big, _dev(torch, cuda, offs))
    assert np.array_equal(st.rows.cpu().numpy(), want)
    assert np.array_equal(st.idx.cpu().numpy(), widx) and st.next.tolist() == [n]


def test_single_handle(cuda, oracle):
    """Stream s equals a single philox_r Sampler over bytes16 keys with stream_id = stream_base + s."""
    import torch

    from reservoir_amd import Sampler, batch

    k, W = 64, 16
    lens = np.array([0, 10, 64, 65, 3000], dtype=np.int64)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    rows = _rows(int(offs[-1]), W)
    rd = _dev(torch, cuda, rows)
    out, cnt = batch.sample_segmented_rows(rd, _dev(torch, cuda, offs), k, SEED, BASE)
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    for s, n in enumerate(lens):
        h = Sampler(k, key_type=f"bytes{W}", engine="philox_r", seed=SEED, stream_id=BASE + s)()
        if n:
            h.sample_all(rd[offs[s]:offs[s + 1]])
        got = np.asarray(h.result()).view(np.uint8).reshape(-1, W)
        assert got.shape[0] == cnt[s] == min(n, k)
        assert np.array_equal(out[s, :cnt[s]], got), s
        assert not out[s, cnt[s]:].any()


# ---- resumed ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _split_case(k):
    """The Long-key split case's streams (lengths and forced cuts) with their last writers."""
    from oracle import oracle

    S, maxlen, L = (60, 4 * k + 5000, 4 * k + 5000) if k >= 512 else (300, 5000, 4 * k + 5000)
    rng = np.random.default_rng(7000 + k)
    lens, nfixed = LK._lengths(k, S, maxlen, rng)
    forced = LK._forced_cuts(k, L)
    lens[nfixed:nfixed + len(forced)] = L
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    widx = LK._last_writers(oracle, SEED, BASE, k, lens)
    for a in (lens, offs, widx):
        a.setflags(write=False)
    return lens, offs, widx, nfixed, forced


def _assert_state(torch, st, want, widx, wnext, msg):
    idx = st.idx.cpu().numpy()
    assert np.array_equal(idx, widx), msg
    assert np.array_equal(st.next.cpu().numpy(), wnext), msg
    got = np.where((idx >= 0)[:, :, None], st.rows.cpu().numpy(), 0)
    assert np.array_equal(got, want), msg
    assert np.array_equal(st.counts.cpu().numpy(), (widx >= 0).sum(1)), msg


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("W", [16, 24])
@pytest.mark.parametrize("k", [64, 100, 512])
def test_split_invariance(cuda, oracle, k, W, B):
    """Ragged streams fed in B updates -- random cuts, and the Long-key test's forced ones at the fill
    boundary, the dense head's end, block and iteration alignment -- end with the rows, idx and next of
    the whole stream, which is also what the stateless launch gives; empty slots keep their sentinel."""
    import torch

    from reservoir_amd import batch

    lens, offs, widx, nfixed, forced = _split_case(k)
    rows = _rows(int(offs[-1]), W)
    want = _expect(rows, offs, widx)
    cuts = LK._cuts(lens, nfixed, forced, B, np.random.default_rng(900 * k + B))
    st = batch.SegmentedSamplerRows(lens.size, k, W, SEED, BASE, device=cuda)
    st.rows.fill_(0xA5)
    for p in range(B):
        parts = [rows[offs[s] + cuts[s, p]: offs[s] + cuts[s, p + 1]] for s in range(lens.size)]
        po = np.r_[0, np.cumsum([x.shape[0] for x in parts])].astype(np.int64)
        assert st.update(_dev(torch, cuda, np.concatenate(parts)), _dev(torch, cuda, po)) is st
    _assert_state(torch, st, want, widx, lens, (k, W, B))
    assert bool((st.rows[st.idx < 0] == 0xA5).all()), "an empty slot's row was written"
    out, cnt = batch.sample_segmented_rows(_dev(torch, cuda, rows), _dev(torch, cuda, offs), k, SEED, BASE)
    assert np.array_equal(out.cpu().numpy(), want), (k, W, B)
    assert np.array_equal(cnt.cpu().numpy(), (widx >= 0).sum(1))


@pytest.mark.parametrize("k,W", [(17, 24), (600, 16)])
def test_rows_by_id(cuda, oracle, k, W):
    """A permuted subset of state rows named by stream_ids, in two updates with different orders; ids -1
    and S are skipped; state rows that no segment names stay bit-identical in all three tensors, and in
    the named ones the slots past idx = -1 keep their sentinel."""
    import torch

    from reservoir_amd import batch
    from reservoir_amd import _native as N

    S, named_n = 50, 30
    rng = np.random.default_rng(40 + k)
    lens = rng.integers(1, 4 * k + 3000, size=S)
    lens[:3] = [1, k, k + 1]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    rows = _rows(int(offs[-1]), W)
    widx = LK._last_writers(oracle, SEED, BASE, k, lens)
    want = _expect(rows, offs, widx)
    named = rng.permutation(S)[:named_n]
    cuts = LK._cuts(lens, S, [], 2, rng)

    st = batch.SegmentedSamplerRows(S, k, W, SEED, BASE, device=cuda)
    st.rows.fill_(0x5A)
    unnamed = np.setdiff1d(np.arange(S), named)
    un = _dev(torch, cuda, unnamed)
    st.idx[un] = 2**40 + 3
    st.next[un] = 2**41 + 9
    st.idx[un[0], k // 2:] = -1  # an unnamed row with empty slots
    before = (st.rows.clone(), st.idx.clone(), st.next.clone())
    junk = _rows(40, W, first=10**9)
    for p in range(2):
        order = rng.permutation(named)
        parts = [rows[offs[s] + cuts[s, p]: offs[s] + cuts[s, p + 1]] for s in order]
        po = np.r_[0, np.cumsum([x.shape[0] for x in parts])].astype(np.int64)
        # two more segments, with the ids -1 and S: skipped
        pr = np.concatenate(parts + [junk])
        po = np.r_[po, po[-1] + 20, po[-1] + 40]
        ids = np.r_[order, -1, S].astype(np.int64)
        st.update(_dev(torch, cuda, pr), _dev(torch, cuda, po), stream_ids=_dev(torch, cuda, ids), check_ids=False)
    idx = st.idx.cpu().numpy()
    got = st.rows.cpu().numpy()
    assert np.array_equal(idx[named], widx[named])
    assert np.array_equal(np.where((idx >= 0)[:, :, None], got, 0)[named], want[named])
    assert (got[named][idx[named] < 0] == 0x5A).all(), "a slot past idx = -1 was written"
    assert np.array_equal(st.next.cpu().numpy()[named], lens[named])
    for now, was in zip((st.rows, st.idx, st.next), before):
        assert torch.equal(now[un], was[un])

    pr, po = rows[:int(lens[0] + lens[1])], offs[:3]
    for bad in ([1, 1], [0, S], [-1, 0]):
        with pytest.raises(N.IllegalArgumentException):
            st.update(_dev(torch, cuda, pr), _dev(torch, cuda, po),
                      stream_ids=_dev(torch, cuda, np.array(bad, dtype=np.int64)))


@pytest.mark.parametrize("k,W", [(5, 24), (64, 16), (700, 40)])
def test_out_of_order_and_merge(cuda, oracle, k, W):
    """Each stream cut in three index ranges: one state fed the ranges in reverse order with bases, and
    three states fed one range each and merged (as stacked tensors and as objects), equal the whole
    stream; merging a state into itself changes nothing; a row whose parts are all empty keeps its
    sentinels."""
    import torch

    from reservoir_amd import batch

    S, P = 40, 3
    rng = np.random.default_rng(60 + k)
    lens = rng.integers(3, 4 * k + 6000, size=S)
    lens[0] = 0                       # all parts empty
    lens[1:4] = [k + 2, 4 * k + 3, 3]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    rows = _rows(int(offs[-1]), W)
    widx = LK._last_writers(oracle, SEED, BASE, k, lens)
    want = _expect(rows, offs, widx)
    cuts = LK._cuts(lens, S, [], P, rng)
    cuts[1:, P - 1] = np.minimum(cuts[1:, P - 1], lens[1:] - 1)   # a last range that is not empty: next = len
    cuts[1:, 1] = np.minimum(cuts[1:, 1], cuts[1:, P - 1])
    cuts[5, 1:P] = [k, k + 1] if lens[5] > k + 1 else cuts[5, 1:P]
    can_i, can_n = 2**50 + 1, 2**51 + 2

    def fresh():
        st = batch.SegmentedSamplerRows(S, k, W, SEED, BASE, device=cuda)
        st.rows.fill_(0x3C)
        st.idx[0], st.next[0] = can_i, can_n
        return st

    def check(st, msg):
        idx = st.idx.cpu().numpy()
        got = st.rows.cpu().numpy()
        assert np.array_equal(idx[1:], widx[1:]), msg
        assert np.array_equal(np.where((idx >= 0)[:, :, None], got, 0)[1:], want[1:]), msg
        assert (got[1:][idx[1:] < 0] == 0x3C).all(), msg
        assert np.array_equal(st.next.cpu().numpy()[1:], lens[1:]), msg
        assert bool((st.rows[0] == 0x3C).all()) and bool((st.idx[0] == can_i).all()) and int(st.next[0]) == can_n, msg

    def feed(st, p):
        parts = [rows[offs[s] + cuts[s, p]: offs[s] + cuts[s, p + 1]] for s in range(S)]
        po = np.r_[0, np.cumsum([x.shape[0] for x in parts])].astype(np.int64)
        return st.update(_dev(torch, cuda, np.concatenate(parts)), _dev(torch, cuda, po),
                         bases=_dev(torch, cuda, cuts[:, p].copy()))

    rev = fresh()
    for p in reversed(range(P)):
        feed(rev, p)
    check(rev, "reverse order")

    parts = [feed(fresh(), p) for p in range(P)]
    stacked = fresh().merge(torch.stack([s.rows for s in parts]), torch.stack([s.idx for s in parts]),
                            torch.stack([s.next for s in parts]))
    check(stacked, "merge of stacked tensors")
    snap = (stacked.rows.clone(), stacked.idx.clone(), stacked.next.clone())
    assert stacked.merge(stacked) is stacked
    for now, was in zip((stacked.rows, stacked.idx, stacked.next), snap):
        assert torch.equal(now, was)
    check(parts[0].merge(parts[1], parts[2]), "merge of objects")
    check(fresh().merge(parts[1].rows, parts[1].idx, parts[1].next).merge(parts[2]).merge(parts[0]), "one by one")


def test_merge_thirds(cuda, oracle):
    """Three states that each saw a third of every stream (by position), merged into a fresh one."""
    import torch

    from reservoir_amd import batch

    k, W, S, n = 100, 24, 30, 3000
    offs = np.arange(S + 1, dtype=np.int64) * n
    rows = _rows(S * n, W)
    widx = LK._last_writers(oracle, SEED, BASE, k, np.full(S, n))
    want = _expect(rows, offs, widx)
    rd = _dev(torch, cuda, rows).view(S, n, W)
    parts = []
    for p in range(3):
        st = batch.SegmentedSamplerRows(S, k, W, SEED, BASE, device=cuda)
        st.update(rd[:, p * 1000:(p + 1) * 1000].reshape(-1, W), _dev(torch, cuda, offs // 3),
                  bases=torch.full((S,), p * 1000, dtype=torch.int64, device=cuda))
        parts.append(st)
    got = batch.SegmentedSamplerRows(S, k, W, SEED, BASE, device=cuda).merge(*parts)
    _assert_state(torch, got, want, widx, np.full(S, n), "thirds")


def test_python_argument_errors(cuda):
    """Type, device, width and shape errors mirror SegmentedSampler's and SegmentedDistinctRows'."""
    import torch

    from reservoir_amd import batch
    from reservoir_amd import _native as N

    R = batch.SegmentedSamplerRows
    with pytest.raises(N.IllegalArgumentException):
        R(4, 0, 16, 1, device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        R(-1, 4, 16, 1, device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        R(4, 4, 16, 1, device="cpu")
    for w in (12, 20, 264, 0):
        with pytest.raises(N.IllegalArgumentException):
            R(4, 4, w, 1, device=cuda)
    for w in (4, 8):
        with pytest.raises(N.ReservoirError, match="SegmentedSampler "):
            R(4, 4, w, 1, device=cuda)
    with pytest.raises(N.ReservoirError, match="15104"):
        R(4, 15105, 16, 1, device=cuda)
    st = R(4, 8, 16, 1, device=cuda)
    assert st.rows.shape == (4, 8, 16) and st.rows.dtype == torch.uint8
    assert bool((st.idx == -1).all()) and bool((st.next == 0).all()) and bool((st.counts == 0).all())
    rows = torch.arange(160, device=cuda).to(torch.uint8).view(10, 16)
    offs = torch.tensor([0, 4, 10], device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows.cpu(), offs)
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows, offs.cpu())
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows.to(torch.int32), offs)
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows, offs.to(torch.int32))
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows.view(-1), offs)
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows.view(5, 32), offs)                       # 32-byte rows into a 16-byte state
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows, offs, stream_ids=torch.tensor([0], device=cuda))
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows, offs, bases=torch.tensor([0, 0], dtype=torch.int32, device=cuda))
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows, offs, stream_ids=torch.tensor([1, 1], device=cuda))
    with pytest.raises(N.IllegalArgumentException):
        st.update(rows, offs, stream_ids=torch.tensor([0, 4], device=cuda))
    with pytest.raises(N.IllegalArgumentException):  # five segments, four rows, no ids
        st.update(rows, torch.tensor([0, 1, 2, 3, 4, 5], device=cuda))
    with pytest.raises(N.NullPointerException):
        st.merge(st.rows)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(st.rows[:, :4], st.idx[:, :4], st.next)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(st.rows, st.idx.to(torch.int32), st.next)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(st.rows.view(torch.int64), st.idx, st.next)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(R(4, 8, 16, 2, device=cuda))
    with pytest.raises(N.IllegalArgumentException):
        st.merge(R(4, 8, 24, 1, device=cuda))
    # the stateless call: host tensors, dtypes, widths, k
    with pytest.raises(N.IllegalArgumentException):
        batch.sample_segmented_rows(rows.cpu(), offs, 4, 1)
    with pytest.raises(N.IllegalArgumentException):
        batch.sample_segmented_rows(rows.to(torch.float32), offs, 4, 1)
    with pytest.raises(N.ReservoirError, match="rsv_sample_segmented "):
        batch.sample_segmented_rows(rows.view(-1, 4), offs, 4, 1)
    with pytest.raises(N.IllegalArgumentException):
        batch.sample_segmented_rows(rows.view(-1, 20), offs, 4, 1)
    with pytest.raises(N.ReservoirError, match="rsv_sample_segmented "):
        batch.sample_segmented_rows(rows.view(-1, 8), offs, 4, 1)
    with pytest.raises(N.IllegalArgumentException):
        batch.sample_segmented_rows(rows, offs, 0, 1)
    assert st.update(rows[:0], offs[:1]) is st
    assert st.update(rows, offs).next.tolist() == [4, 6, 0, 0]
    assert st.counts.tolist() == [4, 6, 0, 0]
    out, cnt = batch.sample_segmented_rows(rows, offs, 8, 1)
    assert torch.equal(torch.where((st.idx >= 0)[:, :, None], st.rows, torch.zeros_like(st.rows))[:2], out)
