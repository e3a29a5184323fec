"""Resumed segmented Sampler.apply (K2 with state: rsv_sample_segmented_update / _merge,
batch.SegmentedSampler).  Per slot the largest global index wins, so a row fed its stream in pieces --
in order, out of order with bases, or assembled by merge -- must end with exactly the keys and last
writers of the whole stream.  Every expected value comes from the oracle: algo_r_segmented over the
concatenated streams (keys), algo_r_last_writers over [0, n) (idx, fill indices included), and
algo_r(..., i0, res) for rows resumed from a preset state."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, BASE = 31, 2**33 + 5


def _head_end(k):
    """The end of the kernel's dense head (rsv_k2.h: 4k, cut to whole 64-pair rounds)."""
    hx = 4 * k
    if hx - k >= 128:
        hx = k + ((hx - k) & ~127)
    return hx


def _forced_cuts(k, L):
    """Cut lists (ascending positions inside a stream of L elements) that every split case forces."""
    hx = _head_end(k)
    b16 = 16 * ((k >> 4) + 3)
    b1k = 1024 * ((k >> 10) + 1)
    specs = [
        [k - 1], [k], [k + 1],                      # the fill boundary
        [2 * k], [k + 1, 3 * k],                    # inside the dense head (k, 4k)
        [hx], [hx - 1], [hx + 1],                   # the head's end
        [b16], [b16 + 1], [b16 - 1],                # block alignment
        [b1k], [b1k + 1], [b1k - 1], [2 * b1k],     # iteration alignment
        [0, 0, k + 7],                              # empty pieces first
        [0],
        [b16 + 5, b16 + 6],                         # a 1-element piece
        [L - 1],
        [1],
        [k - 1, k, k + 1, hx],
    ]
    return [[min(max(c, 0), L) for c in s] for s in specs]


def _lengths(k, S, maxlen, rng):
    lens = rng.integers(0, maxlen + 1, size=S)
    fixed = [0, 1, max(k - 1, 0), k, k + 1, 4096]
    lens[:len(fixed)] = fixed
    return lens, len(fixed)


def _cuts(lens, first_forced, forced, B, rng):
    """cuts[s] = B + 1 ascending positions, 0 first and lens[s] last; rows first_forced.. take the forced lists."""
    S = lens.size
    cuts = np.zeros((S, B + 1), dtype=np.int64)
    for s in range(S):
        c = np.sort(rng.integers(0, lens[s] + 1, size=B - 1))
        f = s - first_forced
        if 0 <= f < len(forced):
            head = forced[f][:B - 1]
            tail = np.sort(rng.integers(head[-1], lens[s] + 1, size=B - 1 - len(head)))
            c = np.r_[head, tail]
        cuts[s, 1:B] = c
        cuts[s, B] = lens[s]
    return cuts


def _pieces(keys, offs, cuts, p, rows=None):
    """Piece p of every row (or of `rows`, in that order): concatenated keys and their offsets."""
    rows = range(offs.size - 1) if rows is None else rows
    parts = [keys[offs[s] + cuts[s, p]: offs[s] + cuts[s, p + 1]] for s in rows]
    plen = np.array([x.size for x in parts], dtype=np.int64)
    return (np.concatenate(parts) if parts else keys[:0]), np.r_[0, np.cumsum(plen)].astype(np.int64)


def _last_writers(oracle, seed, base, k, lens):
    return np.stack([oracle.algo_r_last_writers(seed, base + s, k, 0, int(n), 1) for s, n in enumerate(lens)])


@functools.lru_cache(maxsize=None)
def _split_case(k):
    """The ragged streams of the split-invariance case at k and their whole-stream oracle (computed once)."""
    from oracle import oracle

    S = 60 if k >= 1000 else 300
    maxlen = 4 * k + 5000 if k >= 1000 else 5000
    L = 4 * k + 5000
    rng = np.random.default_rng(7000 + k)
    lens, nfixed = _lengths(k, S, maxlen, rng)
    forced = _forced_cuts(k, L)
    lens[nfixed:nfixed + len(forced)] = L
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = oracle.splitmix_keys(13 * k + 1, int(offs[-1]))
    want, wcnt = oracle.algo_r_segmented(SEED, BASE, k, keys, offs)
    widx = _last_writers(oracle, SEED, BASE, k, lens)
    assert np.array_equal((widx >= 0).sum(1), wcnt)
    for a in (lens, offs, keys, want, widx):
        a.setflags(write=False)
    return lens, offs, keys, want, widx, nfixed, forced


def _dev(torch, cuda, a, dtype=None):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(cuda)  # (the shared references are read-only)
    return t if dtype is None else t.to(dtype)


def _assert_state(st, want, widx, wnext, msg):
    idx = st.idx.cpu().numpy()
    assert np.array_equal(idx, widx), msg
    assert np.array_equal(st.next.cpu().numpy(), wnext), msg
    got = np.where(idx >= 0, st.keys.cpu().numpy().astype(np.int64), 0)
    assert np.array_equal(got, want), msg
    assert np.array_equal(st.counts.cpu().numpy(), (widx >= 0).sum(1)), msg


def _run_split(cuda, k, B, dtype_name):
    import torch

    from reservoir_amd import batch

    lens, offs, keys, want, widx, nfixed, forced = _split_case(k)
    dtype = getattr(torch, dtype_name)
    if dtype == torch.int32:  # the same streams through 4-byte keys: the low words, sign-extended
        keys = keys.astype(np.int32).astype(np.int64)
        want = np.where(widx >= 0, want.astype(np.int32).astype(np.int64), 0)
    rng = np.random.default_rng(900 * k + B)
    cuts = _cuts(lens, nfixed, forced, B, rng)
    st = batch.SegmentedSampler(lens.size, k, SEED, BASE, dtype=dtype, device=cuda)
    for p in range(B):
        pk, po = _pieces(keys, offs, cuts, p)
        assert st.update(_dev(torch, cuda, pk, dtype), _dev(torch, cuda, po)) is st
    _assert_state(st, want, widx, lens, (k, B))
    out, cnt = batch.sample_segmented(_dev(torch, cuda, keys, dtype), _dev(torch, cuda, offs), k, SEED, BASE)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), want), (k, B)
    assert np.array_equal(cnt.cpu().numpy(), (widx >= 0).sum(1)), (k, B)


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("k", [1, 2, 17, 63, 64, 65, 100, 511, 512, 513, 1024, 4096, 15104])
def test_split_invariance(cuda, oracle, k, B):
    """Ragged streams fed in B updates -- random cuts, and forced ones at the fill boundary, inside and
    at the end of the dense head, at block and iteration alignment, empty pieces first, 1-element
    pieces -- end with the keys, idx and next of the whole stream; untouched slots keep idx -1."""
    _run_split(cuda, k, B, "int64")


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("k", [64, 1024])
def test_split_invariance_int32(cuda, oracle, k, B):
    _run_split(cuda, k, B, "int32")


@pytest.mark.parametrize("k", [17, 600])
def test_rows_by_id(cuda, oracle, k):
    """A permuted subset of rows named by stream_ids, in two updates with different orders; ids -1 and
    S are skipped; rows not named keep their canaries bit for bit in all three tensors."""
    import torch

    from reservoir_amd import batch
    from reservoir_amd import _native as N

    S, named_n = 50, 30
    rng = np.random.default_rng(40 + k)
    lens = rng.integers(1, 4 * k + 3000, size=S)
    lens[:3] = [1, k, k + 1]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = oracle.splitmix_keys(5 * k, int(offs[-1]))
    want, _ = oracle.algo_r_segmented(SEED, BASE, k, keys, offs)
    widx = _last_writers(oracle, SEED, BASE, k, lens)
    named = rng.permutation(S)[:named_n]
    cuts = _cuts(lens, S, [], 2, rng)

    st = batch.SegmentedSampler(S, k, SEED, BASE, device=cuda)
    unnamed = np.setdiff1d(np.arange(S), named)
    un = _dev(torch, cuda, unnamed)
    st.keys[un] = 0x5A5A5A5A5A5A5A5A
    st.idx[un] = 2**40 + 3
    st.next[un] = 2**41 + 9
    before = (st.keys.clone(), st.idx.clone(), st.next.clone())
    for p in range(2):
        order = rng.permutation(named)
        pk, po = _pieces(keys, offs, cuts, p, rows=order)
        # two more segments, with the ids -1 and S: skipped
        junk = oracle.splitmix_keys(99, 40)
        pk = np.r_[pk, junk]
        po = np.r_[po, po[-1] + 20, po[-1] + 40]
        ids = np.r_[order, -1, S].astype(np.int64)
        st.update(_dev(torch, cuda, pk), _dev(torch, cuda, po), stream_ids=_dev(torch, cuda, ids), check_ids=False)
    idx = st.idx.cpu().numpy()
    got = np.where(idx >= 0, st.keys.cpu().numpy(), 0)
    assert np.array_equal(idx[named], widx[named])
    assert np.array_equal(got[named], want[named])
    assert np.array_equal(st.next.cpu().numpy()[named], lens[named])
    for now, was in zip((st.keys, st.idx, st.next), before):
        assert torch.equal(now[un], was[un])

    pk, po = _pieces(keys, offs, cuts, 0, rows=[0, 1])
    for bad in ([1, 1], [0, S], [-1, 0]):
        with pytest.raises(N.IllegalArgumentException):
            st.update(_dev(torch, cuda, pk), _dev(torch, cuda, po),
                      stream_ids=_dev(torch, cuda, np.array(bad, dtype=np.int64)))


@pytest.mark.parametrize("k", [5, 64, 700])
def test_out_of_order_and_merge(cuda, oracle, k):
    """Each stream cut in three index ranges: one state fed the ranges in reverse order with bases, and
    three states fed one range each and merged (as stacked tensors and as objects), equal the whole
    stream; merging a state into itself changes nothing; a row whose parts are all empty keeps its
    canaries."""
    import torch

    from reservoir_amd import batch

    S, P = 40, 3
    rng = np.random.default_rng(60 + k)
    lens = rng.integers(3, 4 * k + 6000, size=S)
    lens[0] = 0                       # all parts empty
    lens[1:4] = [k + 2, 4 * k + 3, 3]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = oracle.splitmix_keys(3 * k + 2, int(offs[-1]))
    want, _ = oracle.algo_r_segmented(SEED, BASE, k, keys, offs)
    widx = _last_writers(oracle, SEED, BASE, k, lens)
    cuts = _cuts(lens, S, [], P, rng)
    cuts[1:, P - 1] = np.minimum(cuts[1:, P - 1], lens[1:] - 1)   # a last range that is not empty: next = len
    cuts[1:, 1] = np.minimum(cuts[1:, 1], cuts[1:, P - 1])
    cuts[5, 1:P] = [k, k + 1] if lens[5] > k + 1 else cuts[5, 1:P]
    can_k, can_i, can_n = 0x1234567812345678, 2**50 + 1, 2**51 + 2

    def fresh():
        st = batch.SegmentedSampler(S, k, SEED, BASE, device=cuda)
        st.keys[0], st.idx[0], st.next[0] = can_k, can_i, can_n
        return st

    def check(st, msg):
        idx = st.idx.cpu().numpy()
        got = np.where(idx >= 0, st.keys.cpu().numpy(), 0)
        assert np.array_equal(idx[1:], widx[1:]), msg
        assert np.array_equal(got[1:], want[1:]), msg
        assert np.array_equal(st.next.cpu().numpy()[1:], lens[1:]), msg
        assert bool((st.keys[0] == can_k).all()) and bool((st.idx[0] == can_i).all()) and int(st.next[0]) == can_n, msg

    def feed(st, p):
        pk, po = _pieces(keys, offs, cuts, p)
        return st.update(_dev(torch, cuda, pk), _dev(torch, cuda, po), bases=_dev(torch, cuda, cuts[:, p].copy()))

    rev = fresh()
    for p in reversed(range(P)):
        feed(rev, p)
    check(rev, "reverse order")

    parts = [feed(fresh(), p) for p in range(P)]
    stacked = fresh().merge(torch.stack([s.keys for s in parts]), torch.stack([s.idx for s in parts]),
                            torch.stack([s.next for s in parts]))
    check(stacked, "merge of stacked tensors")
    snap = (stacked.keys.clone(), stacked.idx.clone(), stacked.next.clone())
    assert stacked.merge(stacked) is stacked
    for now, was in zip((stacked.keys, stacked.idx, stacked.next), snap):
        assert torch.equal(now, was)
    check(parts[0].merge(parts[1], parts[2]), "merge of objects")
    check(fresh().merge(parts[1].keys, parts[1].idx, parts[1].next).merge(parts[2]).merge(parts[0]), "one by one")


def _large_base(cuda, oracle, k, S, N0, min_changed, full_oracle):
    import torch

    from reservoir_amd import batch

    seed, base, n = 9, 100, 5000
    keys = oracle.splitmix_keys(77 + k, S * n)
    offs = (np.arange(S + 1, dtype=np.int64) * n)
    preset = (np.arange(S * k, dtype=np.int64).reshape(S, k) * 3 + 1) | (1 << 62)
    lw = np.stack([oracle.algo_r_last_writers(seed, base + r, k, N0, n, 1) for r in range(S)])
    widx = np.where(lw >= 0, lw, np.arange(k, dtype=np.int64)[None, :])
    want = preset.copy()
    # rows without a writer in [N0, N0 + n) keep the preset; algo_r runs on every row (full_oracle) or on
    # the rows with a writer plus a sample of the others (S = 20000: every row would take ~7 s of CPU)
    hit = (lw >= 0).any(1)
    rows = np.arange(S) if full_oracle else np.union1d(np.flatnonzero(hit),
                                                       np.random.default_rng(k).integers(0, S, size=500))
    for r in rows:
        res, _ = oracle.algo_r(seed, base + int(r), k, keys[r * n:(r + 1) * n], N0, preset[r].copy())
        want[r] = res
    changed = int((want != preset).any(1).sum())
    assert np.array_equal((want != preset).any(1), hit)
    assert changed >= min_changed, f"the oracle changes only {changed} rows: the case would pass vacuously"

    st = batch.SegmentedSampler(S, k, seed, base, device=cuda)
    st.keys.copy_(_dev(torch, cuda, preset))
    st.idx.copy_(torch.arange(k, device=cuda)[None, :].expand(S, k))
    st.next.fill_(N0)
    st.update(_dev(torch, cuda, keys), _dev(torch, cuda, offs))
    assert np.array_equal(st.keys.cpu().numpy(), want), N0
    assert np.array_equal(st.idx.cpu().numpy(), widx), N0
    assert bool((st.next == N0 + n).all())


# expected rows with a replacement: S * 5000 * k / N0 = 305 at 2^27 and 9.5 at 2^32 (the oracle gives 304,
# 305 and 17 for exactly these parameters)
@pytest.mark.parametrize("N0,min_changed", [(2**27 - 6000, 200), (2**27 - 2500, 200), (2**32 - 2500, 10)])
def test_large_base_indices(cuda, oracle, N0, min_changed):
    """Rows resumed at large indices from a preset state (k = 4096: the workgroup form): the 32-bit path,
    the switch to 64-bit indices inside the segment's range, and beyond 2^32."""
    _large_base(cuda, oracle, 4096, 2000, N0, min_changed, True)


def test_large_base_indices_wave_form(cuda, oracle):
    """The same at k = 64 (one wave per stream), 64-bit indices; ~48 of the 20000 rows change."""
    _large_base(cuda, oracle, 64, 20000, 2**27 - 2500, 1, False)


@pytest.mark.parametrize("k", [1, 5])
def test_sparse_region(cuda, oracle, k):
    """Streams of 20000 elements reach the sparse region (i + 1 >= 256 k: only a zero level-0 byte can
    hit); cuts at 256 k - 1, 256 k and 256 k + 1."""
    import torch

    from reservoir_amd import batch

    n = 20000
    specs = [[256 * k - 1], [256 * k], [256 * k + 1], [256 * k - 1, 256 * k, 256 * k + 1], [k, 256 * k, 10000, 19999]]
    S = len(specs) + 3
    lens = np.full(S, n, dtype=np.int64)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = oracle.splitmix_keys(21 + k, int(offs[-1]))
    want, _ = oracle.algo_r_segmented(SEED, BASE, k, keys, offs)
    widx = _last_writers(oracle, SEED, BASE, k, lens)
    for B in (2, 5):
        cuts = _cuts(lens, 0, specs, B, np.random.default_rng(B + k))
        st = batch.SegmentedSampler(S, k, SEED, BASE, device=cuda)
        for p in range(B):
            pk, po = _pieces(keys, offs, cuts, p)
            st.update(_dev(torch, cuda, pk), _dev(torch, cuda, po))
        _assert_state(st, want, widx, lens, (k, B))
    out, _ = batch.sample_segmented(_dev(torch, cuda, keys), _dev(torch, cuda, offs), k, SEED, BASE)
    assert np.array_equal(out.cpu().numpy(), want)


_FIFO_CASE = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from oracle import oracle
from reservoir_amd import batch
cuda = torch.device("cuda", 0)
for k in (64, 256, 1000):
    rng = np.random.default_rng(500 + k)
    lens = rng.integers(0, 20_000, size=200)
    lens[:4] = [k, k + 1, 4096, 19_999]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = oracle.splitmix_keys(11 * k, int(offs[-1]))
    want, wcnt = oracle.algo_r_segmented(31, 77, k, keys, offs)
    widx = np.stack([oracle.algo_r_last_writers(31, 77 + s, k, 0, int(n), 1) for s, n in enumerate(lens)])
    cuts = np.sort(rng.integers(0, lens[:, None] + 1, size=(lens.size, 2)), axis=1)
    cuts = np.c_[np.zeros_like(lens), cuts, lens]
    st = batch.SegmentedSampler(lens.size, k, 31, 77, device=cuda)
    for p in range(3):
        parts = [keys[offs[s] + cuts[s, p]: offs[s] + cuts[s, p + 1]] for s in range(lens.size)]
        po = np.r_[0, np.cumsum([x.size for x in parts])].astype(np.int64)
        st.update(torch.from_numpy(np.concatenate(parts)).to(cuda), torch.from_numpy(po).to(cuda))
    idx = st.idx.cpu().numpy()
    assert np.array_equal(idx, widx), k
    assert np.array_equal(np.where(idx >= 0, st.keys.cpu().numpy(), 0), want), k
    assert np.array_equal(st.next.cpu().numpy(), lens), k
print("fifo overflow ok")
"""


def test_fifo_overflow_rounds(cuda, oracle):
    """RSV_K2_FIFO_CAP = 128 sends dense iterations through the ballot-round path of the resumed loops
    (k = 64, 256: one wave per stream; 1000: one workgroup): streams of up to 20000 elements in three
    updates equal the oracle.  The engine reads the variable once per process: a child process sets it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RSV_K2_FIFO_CAP="128")
    r = subprocess.run([sys.executable, "-c", _FIFO_CASE.format(root=root)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "fifo overflow ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_python_argument_errors(cuda):
    """Type, device and shape errors mirror SegmentedDistinct's."""
    import torch

    from reservoir_amd import batch
    from reservoir_amd import _native as N

    with pytest.raises(N.IllegalArgumentException):
        batch.SegmentedSampler(4, 0, 1, device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        batch.SegmentedSampler(-1, 4, 1, device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        batch.SegmentedSampler(4, 4, 1, dtype=torch.float32, device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        batch.SegmentedSampler(4, 4, 1, device="cpu")
    with pytest.raises(N.ReservoirError, match="15104"):
        batch.SegmentedSampler(4, 15105, 1, device=cuda)
    st = batch.SegmentedSampler(4, 8, 1, device=cuda)
    assert st.keys.shape == (4, 8) and bool((st.idx == -1).all()) and bool((st.next == 0).all())
    assert bool((st.counts == 0).all())
    keys = torch.arange(10, device=cuda)
    offs = torch.tensor([0, 4, 10], device=cuda)
    with pytest.raises(N.IllegalArgumentException):
        st.update(keys.cpu(), offs)
    with pytest.raises(N.IllegalArgumentException):
        st.update(keys.to(torch.int32), offs)
    with pytest.raises(N.IllegalArgumentException):
        st.update(keys, offs, stream_ids=torch.tensor([0], device=cuda))
    with pytest.raises(N.IllegalArgumentException):
        st.update(keys, offs, bases=torch.tensor([0, 0], dtype=torch.int32, device=cuda))
    with pytest.raises(N.IllegalArgumentException):  # five segments, four rows, no ids
        st.update(keys, torch.tensor([0, 1, 2, 3, 4, 5], device=cuda))
    with pytest.raises(N.NullPointerException):
        st.merge(st.keys)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(st.keys[:, :4], st.idx[:, :4], st.next)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(st.keys, st.idx.to(torch.int32), st.next)
    with pytest.raises(N.IllegalArgumentException):
        st.merge(batch.SegmentedSampler(4, 8, 2, device=cuda))
    assert st.update(keys[:0], offs[:1]) is st
    assert st.update(keys, offs).next.tolist() == [4, 6, 0, 0]
    assert st.counts.tolist() == [4, 6, 0, 0]
