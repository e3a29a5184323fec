"""Keyless segmented Sampler.apply (rsv_sample_segmented_indexed / _update / _merge, batch.sample_segmented_indexed,
batch.SegmentedObjectSampler): only the streams' lengths reach the device and indices come back.  Every expected
value comes from oracle.algo_r_last_writers(seed, stream, k, i0, n) -- per slot the global index of its last writer
over [i0, i0 + n), fill indices included, -1 where there is none -- and never from the code under test."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, BASE = 0x9E3779B97F4A7C15, 2**33 + 5   # a 64-bit seed, stream ids beyond 32 bits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head_end(k):
    """The end of the kernels' dense head (rsv_k2.h: 4k, cut to whole 64-pair rounds)."""
    hx = 4 * k
    if hx - k >= 128:
        hx = k + ((hx - k) & ~127)
    return hx


def _want(O, k, lens, seed=SEED, base=BASE):
    """The whole-stream oracle: idx (S, k) and counts (S,)."""
    idx = np.stack([O.algo_r_last_writers(seed, base + s, k, 0, int(n), 1) for s, n in enumerate(lens)])
    return idx, np.minimum(np.asarray(lens, dtype=np.int64), k)


def _offsets(lens, start=0):
    return np.r_[start, start + np.cumsum(np.asarray(lens, dtype=np.int64))].astype(np.int64)


def _dev(torch, cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _stateless_lengths(k, rng):
    hx = _head_end(k)
    b16 = 16 * ((k >> 4) + 3)
    b1k = 1024 * ((k >> 10) + 2)
    fixed = [0, 1, k - 1, k, k + 1, hx - 1, hx, hx + 1, b16 - 1, b16 + 1, b1k - 1, b1k + 1, 4096]
    return np.array([max(n, 0) for n in fixed] + rng.integers(0, 4 * k + 5001, size=14).tolist(), dtype=np.int64)


# ---- stateless -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 17, 64, 65, 100, 511, 512, 1024])
def test_stateless_equals_the_oracle(cuda, oracle, k):
    import torch

    from reservoir_amd import batch

    lens = _stateless_lengths(k, np.random.default_rng(100 + k))
    widx, wcnt = _want(oracle, k, lens)
    idx, cnt = batch.sample_segmented_indexed(_dev(torch, cuda, _offsets(lens, 7)), k, SEED, BASE)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (lens.size, k)
    assert np.array_equal(idx.cpu().numpy(), widx)
    assert np.array_equal(cnt.cpu().numpy(), wcnt)


def test_stateless_global_table_form(cuda, oracle):
    """k beyond the LDS table (4 k bytes no longer fit beside the waves' rings): the table in global scratch,
    twice, so the second launch finds the scratch as the first one left it."""
    import torch

    from reservoir_amd import batch

    k = 30300
    lens = np.array([0, 1, k - 1, k, k + 1, 140000], dtype=np.int64)
    widx, wcnt = _want(oracle, k, lens)
    offs = _dev(torch, cuda, _offsets(lens))
    for _ in range(2):
        idx, cnt = batch.sample_segmented_indexed(offs, k, SEED, BASE)
        assert np.array_equal(idx.cpu().numpy(), widx)
        assert np.array_equal(cnt.cpu().numpy(), wcnt)


@pytest.mark.parametrize("k", [64, 600])
def test_stateless_names_the_keyed_launch_winners(cuda, oracle, k):
    """For int64 keys over the same offsets, sample_segmented's output is keys[offsets[s] + idx] where idx >= 0
    and 0 elsewhere."""
    import torch

    from reservoir_amd import batch

    lens = _stateless_lengths(k, np.random.default_rng(300 + k))
    offs = _offsets(lens)
    keys = oracle.splitmix_keys(5 * k + 1, int(offs[-1]))
    d_offs = _dev(torch, cuda, offs)
    out, cnt = batch.sample_segmented(_dev(torch, cuda, keys), d_offs, k, SEED, BASE)
    idx, icnt = batch.sample_segmented_indexed(d_offs, k, SEED, BASE)
    idx = idx.cpu().numpy()
    at = np.clip(offs[:-1, None] + idx, 0, max(keys.size - 1, 0))
    assert np.array_equal(out.cpu().numpy(), np.where(idx >= 0, keys[at], 0))
    assert np.array_equal(cnt.cpu().numpy(), icnt.cpu().numpy())


# ---- update --------------------------------------------------------------------------------------
def _raw_update(torch, L, k, seed, base, idx, nxt, lens, ids=None, bases=None):
    """One rsv_sample_segmented_indexed_update over segments of the given lengths; returns (hits, hit_counts)
    as numpy arrays.  hits and hit_counts start as garbage: the kernel must write all of them."""
    from reservoir_amd import _native as N

    dev = idx.device
    B = len(lens)
    offs = _dev(torch, dev, _offsets(lens, 3))
    d_ids = None if ids is None else _dev(torch, dev, np.asarray(ids, dtype=np.int64))
    d_bases = None if bases is None else _dev(torch, dev, np.asarray(bases, dtype=np.int64))
    hits = torch.full((B, k), -77, dtype=torch.int64, device=dev)
    hc = torch.full((B,), -77, dtype=torch.int64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    N.check(L.rsv_sample_segmented_indexed_update(
        p(offs), p(d_ids), p(d_bases), B, idx.shape[0], k, seed & (2**64 - 1), base & (2**64 - 1), p(idx), p(nxt),
        p(hits), p(hc), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return hits.cpu().numpy(), hc.cpu().numpy()


def _forced_cuts(k, L):
    hx = _head_end(k)
    b16 = 16 * ((k >> 4) + 3)
    b1k = 1024 * ((k >> 10) + 1)
    specs = [
        [k - 1], [k], [k + 1],                      # the fill boundary
        [2 * k], [k + 1, 3 * k],                    # inside the dense head
        [hx], [hx - 1], [hx + 1],                   # the head's end
        [b16], [b16 + 1], [b16 - 1],                # block alignment
        [b1k], [b1k + 1], [b1k - 1], [2 * b1k],     # iteration alignment
        [0, 0, k + 7], [0],                         # empty pieces first
        [b16 + 5, b16 + 6],                         # a one-element piece
        [L - 1], [1],
        [k - 1, k, k + 1, hx],
    ]
    return [[min(max(c, 0), L) for c in s] for s in specs]


def _cuts(lens, forced, B, rng):
    """cuts[s] = B + 1 ascending positions, 0 first and lens[s] last; the first rows take the forced lists."""
    S = lens.size
    cuts = np.zeros((S, B + 1), dtype=np.int64)
    for s in range(S):
        c = np.sort(rng.integers(0, lens[s] + 1, size=B - 1))
        if s < len(forced) and B > 1:
            head = forced[s][:B - 1]
            tail = np.sort(rng.integers(head[-1], lens[s] + 1, size=B - 1 - len(head)))
            c = np.r_[head, tail].astype(np.int64)
        cuts[s, 1:B] = c
        cuts[s, B] = lens[s]
    return cuts


@functools.lru_cache(maxsize=None)
def _update_case(k):
    """Ragged streams at k: the forced-cut rows of full length first, then fixed and random lengths."""
    L = 4 * k + 5000
    forced = _forced_cuts(k, L)
    rng = np.random.default_rng(7000 + k)
    lens = np.r_[np.full(len(forced), L), [0, 1, max(k - 1, 0), k, k + 1, 4096],
                 rng.integers(0, L + 1, size=8)].astype(np.int64)
    lens.setflags(write=False)
    return lens, forced


def _prefix_want(O, k, upto):
    return np.stack([O.algo_r_last_writers(SEED, BASE + s, k, 0, int(n), 1) for s, n in enumerate(upto)])


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("k", [17, 64, 600])
def test_update_in_pieces(cuda, oracle, k, B):
    """Every row fed in B pieces: after every launch idx and next equal the oracle over the prefix, hits names
    exactly the slots that changed, by position inside the segment, and the final idx is SegmentedSampler's."""
    import torch

    from reservoir_amd import _native as N
    from reservoir_amd import batch

    L_ = N.load()
    lens, forced = _update_case(k)
    S = lens.size
    cuts = _cuts(lens, forced, B, np.random.default_rng(900 * k + B))
    idx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    nxt = torch.zeros(S, dtype=torch.int64, device=cuda)
    keyed = batch.SegmentedSampler(S, k, SEED, BASE, device=cuda)
    for p in range(B):
        before = idx.cpu().numpy()
        plen = cuts[:, p + 1] - cuts[:, p]
        hits, hc = _raw_update(torch, L_, k, SEED, BASE, idx, nxt, plen)
        after = idx.cpu().numpy()
        assert np.array_equal(after, _prefix_want(oracle, k, cuts[:, p + 1])), (k, B, p)
        # a row that has not been named with elements yet keeps next = 0
        assert np.array_equal(nxt.cpu().numpy(), cuts[:, p + 1]), (k, B, p)
        assert np.array_equal(hits, np.where(after != before, after - cuts[:, p, None], -1)), (k, B, p)
        assert np.array_equal(hc, (hits >= 0).sum(1)), (k, B, p)
        keyed.update(torch.zeros(int(plen.sum()), dtype=torch.int64, device=cuda), _dev(torch, cuda, _offsets(plen)))
    assert np.array_equal(idx.cpu().numpy(), keyed.idx.cpu().numpy())
    assert np.array_equal(nxt.cpu().numpy(), keyed.next.cpu().numpy())


@pytest.mark.parametrize("k", [64, 600])
def test_update_skipped_segments(cuda, oracle, k):
    """An id out of range, a negative base and an empty segment: a row of -1, a count of 0, the state untouched."""
    import torch

    from reservoir_amd import _native as N

    L_ = N.load()
    S = 6
    idx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    nxt = torch.zeros(S, dtype=torch.int64, device=cuda)
    _raw_update(torch, L_, k, SEED, BASE, idx, nxt, [3000] * S)
    before, nbefore = idx.cpu().numpy(), nxt.cpu().numpy()
    ids = [0, -1, S, 3, 4, 5]
    bases = [3000, 3000, 3000, -5, 3000, 3000]
    lens = [500, 500, 500, 500, 0, 700]
    hits, hc = _raw_update(torch, L_, k, SEED, BASE, idx, nxt, lens, ids, bases)
    after, nafter = idx.cpu().numpy(), nxt.cpu().numpy()
    for b in (1, 2, 3, 4):
        assert (hits[b] == -1).all() and hc[b] == 0, b
    for r in (1, 2, 3, 4):
        assert np.array_equal(after[r], before[r]) and nafter[r] == nbefore[r], r
    for b, r, n in ((0, 0, 3500), (5, 5, 3700)):
        assert np.array_equal(after[r], oracle.algo_r_last_writers(SEED, BASE + r, k, 0, n, 1))
        assert nafter[r] == n
        assert np.array_equal(hits[b], np.where(after[r] != before[r], after[r] - 3000, -1))
        assert hc[b] == (hits[b] >= 0).sum()


@pytest.mark.parametrize("k", [64, 600])
def test_update_out_of_order_permuted_and_subset(cuda, oracle, k):
    """Pieces fed last to first with bases=, the rows named by a permutation, then a subset of them."""
    import torch

    from reservoir_amd import _native as N

    L_ = N.load()
    rng = np.random.default_rng(40 + k)
    S = 9
    lens = rng.integers(2 * k, 4 * k + 4000, size=S).astype(np.int64)
    cuts = np.c_[np.zeros(S, dtype=np.int64), np.sort(rng.integers(0, lens[:, None] + 1, size=(S, 2)), axis=1), lens]
    idx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    nxt = torch.zeros(S, dtype=torch.int64, device=cuda)
    widx, _ = _want(oracle, k, lens)
    for p in (2, 1, 0):
        rows = rng.permutation(S) if p else np.array([1, 4, 6, 8, 0])   # piece 0: a subset first, the rest after
        for part in ([rows] if p else [rows, np.setdiff1d(np.arange(S), rows)]):
            before = idx.cpu().numpy()
            hits, hc = _raw_update(torch, L_, k, SEED, BASE, idx, nxt, cuts[part, p + 1] - cuts[part, p], part,
                                   cuts[part, p])
            after = idx.cpu().numpy()
            others = np.setdiff1d(np.arange(S), part)
            assert np.array_equal(after[others], before[others])
            assert np.array_equal(hits, np.where(after[part] != before[part], after[part] - cuts[part, p, None], -1))
            assert np.array_equal(hc, (hits >= 0).sum(1))
    assert np.array_equal(idx.cpu().numpy(), widx)
    assert np.array_equal(nxt.cpu().numpy(), lens)


@pytest.mark.parametrize("k,S", [(64, 3000), (600, 300)])
def test_update_large_bases(cuda, oracle, k, S):
    """Segments at 2^33 and above (64-bit indices): idx is the oracle's last writer over the segment's range.
    A slot is hit with probability n k / n0 per row: about 11 hits over the rows at either shape."""
    import torch

    from reservoir_amd import _native as N

    L_ = N.load()
    n0, n = 2**33 + 1000, 500_000
    idx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    nxt = torch.zeros(S, dtype=torch.int64, device=cuda)
    hits, hc = _raw_update(torch, L_, k, SEED, BASE, idx, nxt, [n] * S, None, [n0] * S)
    want = np.stack([oracle.algo_r_last_writers(SEED, BASE + s, k, n0, n, 0) for s in range(S)])
    assert (want >= 0).sum() > 0
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(hits, np.where(want >= 0, want - n0, -1))
    assert np.array_equal(hc, (want >= 0).sum(1))
    assert (nxt.cpu().numpy() == n0 + n).all()


# ---- merge ---------------------------------------------------------------------------------------
def _raw_merge(torch, L, k, part_idx, part_next, idx, nxt):
    from reservoir_amd import _native as N

    src = torch.full(tuple(idx.shape), -77, dtype=torch.int32, device=idx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    N.check(L.rsv_sample_segmented_indexed_merge(
        p(part_idx), p(part_next), part_idx.shape[0], idx.shape[0], k, p(idx), p(nxt), p(src),
        C.c_void_p(torch.cuda.current_stream(idx.device).cuda_stream)))
    return src.cpu().numpy()


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("k", [64, 600])
def test_merge_of_parts(cuda, oracle, k, P):
    """The state saw piece 0 of every stream and P other states one later piece each."""
    import torch

    from reservoir_amd import _native as N

    L_ = N.load()
    rng = np.random.default_rng(60 + k + P)
    S = 12
    lens = rng.integers(0, 4 * k + 4000, size=S).astype(np.int64)
    lens[:2] = [0, k]
    cuts = np.c_[np.zeros(S, dtype=np.int64), np.sort(rng.integers(0, lens[:, None] + 1, size=(S, P)), axis=1), lens]
    states = []
    for p in range(P + 1):
        idx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
        nxt = torch.zeros(S, dtype=torch.int64, device=cuda)
        _raw_update(torch, L_, k, SEED, BASE, idx, nxt, cuts[:, p + 1] - cuts[:, p], None, cuts[:, p])
        states.append((idx, nxt))
    idx, nxt = states[0]
    part_idx = torch.stack([s[0] for s in states[1:]])
    part_next = torch.stack([s[1] for s in states[1:]])
    before = idx.cpu().numpy()
    src = _raw_merge(torch, L_, k, part_idx, part_next, idx, nxt)
    after = idx.cpu().numpy()
    widx, _ = _want(oracle, k, lens)
    assert np.array_equal(after, widx)
    # a part that saw an empty piece has next = 0: the row's next is the largest end any of them reached
    wnext = np.max(np.where(cuts[:, 1:] > cuts[:, :-1], cuts[:, 1:], 0), axis=1)
    assert np.array_equal(nxt.cpu().numpy(), wnext)
    assert np.array_equal(src == -1, after == before)
    assert src.min() >= -1 and src.max() < P
    pi = part_idx.cpu().numpy()
    r, j = np.nonzero(src >= 0)
    assert np.array_equal(pi[src[r, j], r, j], after[r, j])


def test_merge_reports_the_lowest_of_equal_parts(cuda, oracle):
    import torch

    from reservoir_amd import _native as N

    L_ = N.load()
    k, S = 64, 5
    pidx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    pnext = torch.zeros(S, dtype=torch.int64, device=cuda)
    _raw_update(torch, L_, k, SEED, BASE, pidx, pnext, [900, 30, 64, 5000, 0])
    idx = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    nxt = torch.zeros(S, dtype=torch.int64, device=cuda)
    src = _raw_merge(torch, L_, k, torch.stack([pidx, pidx]), torch.stack([pnext, pnext]), idx, nxt)
    assert np.array_equal(src, np.where(pidx.cpu().numpy() >= 0, 0, -1))
    assert np.array_equal(idx.cpu().numpy(), pidx.cpu().numpy())


# ---- objects -------------------------------------------------------------------------------------
def _object_streams(kind, lens):
    if kind == "str":
        return [[f"row-{s}-{i}" for i in range(n)] for s, n in enumerate(lens)]
    return [[(s, i, float(i) / 2) for i in range(n)] for s, n in enumerate(lens)]


def _feed(st, streams, cuts, p, rows=None):
    rows = range(len(streams)) if rows is None else rows
    parts = [streams[s][cuts[s][p]:cuts[s][p + 1]] for s in rows]
    flat = [e for part in parts for e in part]
    return flat, _offsets([len(x) for x in parts])


OBJ_K, OBJ_LENS = 16, [0, 5, 16, 17, 300, 2000]
OBJ_CUTS = (
    [[0, n] for n in OBJ_LENS],                                        # whole
    [[0, min(n, 15), min(n, 16), n] for n in OBJ_LENS],                # around the fill boundary
    [[0, 0, n // 3, n // 3, n // 3 + 1, n] for n in OBJ_LENS],         # empty and one-element pieces
)


@pytest.mark.parametrize("pattern", range(3))
@pytest.mark.parametrize("kind", ["str", "tuple"])
def test_object_sampler_equals_one_handle_per_row(cuda, kind, pattern):
    from reservoir_amd import Sampler, batch

    streams = _object_streams(kind, OBJ_LENS)
    cuts = OBJ_CUTS[pattern]
    calls = []
    fn = lambda e: (calls.append(e), ("m", e))[1]
    st = batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED, BASE, map_fn=fn, device=cuda)
    for p in range(len(cuts[0]) - 1):
        flat, offs = _feed(st, streams, cuts, p)
        n0 = len(calls)
        assert st.update(flat, offs) is st
        assert len(calls) - n0 == int(st.last_hit_counts.sum())
    for r, stream in enumerate(streams):
        h = Sampler(OBJ_K, seed=SEED, stream_id=BASE + r, key_type="object")(lambda e: ("m", e))
        h.sample_all(stream)
        assert st.result(r) == list(h.result()), (kind, pattern, r)
    assert st.results() == [st.result(r) for r in range(len(streams))]
    assert st.counts.tolist() == [min(n, OBJ_K) for n in OBJ_LENS]
    # the same streams in one stateless launch
    flat, offs = _feed(st, streams, [[0, n] for n in OBJ_LENS], 0)
    assert batch.sample_segmented_objects(flat, offs, OBJ_K, SEED, BASE, map_fn=fn) == st.results()


def test_object_sampler_map_fn_failure_leaves_the_state(cuda):
    import torch

    from reservoir_amd import batch

    streams = _object_streams("str", OBJ_LENS)
    cuts = [[0, n // 2, n] for n in OBJ_LENS]
    state = {"calls": 0, "fail": False}

    def fn(e):
        state["calls"] += 1
        if state["fail"] and state["calls"] == 3:
            raise KeyError(e)
        return e.upper()

    st = batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED, BASE, map_fn=fn, device=cuda)
    flat, offs = _feed(st, streams, cuts, 0)
    st.update(flat, offs)
    idx, nxt, res = st.idx.clone(), st.next.clone(), st.results()
    flat, offs = _feed(st, streams, cuts, 1)
    state.update(calls=0, fail=True)
    with pytest.raises(KeyError):
        st.update(flat, offs)
    assert torch.equal(st.idx, idx) and torch.equal(st.next, nxt) and st.results() == res
    state.update(calls=0, fail=False)
    st.update(flat, offs)
    whole = batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED, BASE, map_fn=str.upper, device=cuda)
    flat, offs = _feed(whole, streams, [[0, n] for n in OBJ_LENS], 0)
    whole.update(flat, offs)
    assert st.results() == whole.results() and torch.equal(st.idx, whole.idx) and torch.equal(st.next, whole.next)


def test_object_sampler_merge_of_two_halves(cuda):
    import torch

    from reservoir_amd import _native as N
    from reservoir_amd import batch

    streams = _object_streams("tuple", OBJ_LENS)
    cuts = [[0, n // 2, n] for n in OBJ_LENS]
    a = batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED, BASE, device=cuda)
    b = batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED, BASE, device=cuda)
    flat, offs = _feed(a, streams, cuts, 0)
    a.update(flat, offs)
    flat, offs = _feed(b, streams, cuts, 1)
    b.update(flat, offs, bases=np.array([c[1] for c in cuts], dtype=np.int64))
    whole = batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED, BASE, device=cuda)
    flat, offs = _feed(whole, streams, [[0, n] for n in OBJ_LENS], 0)
    whole.update(flat, offs)
    assert a.merge(b) is a
    assert a.results() == whole.results() and torch.equal(a.idx, whole.idx) and torch.equal(a.next, whole.next)
    with pytest.raises(N.IllegalArgumentException):
        a.merge(batch.SegmentedObjectSampler(len(streams), OBJ_K, SEED + 1, BASE, device=cuda))


# ---- the split form ------------------------------------------------------------------------------
SPLIT_KS = (1, 64, 512, 2048, 3000)
SPLIT_LENS = (700, 0, 1, 2047, 5, 2048, 2049, 100, 6144, 6145, 21257, 64)   # the long ones among short streams


def _split_launches(setting):
    """(k, lens) of every launch a child process makes under one RSV_K2_SPLIT_LEN setting."""
    if setting is None:   # the default split length: one stream of three split lengths plus 5
        from reservoir_amd import batch

        return [(64, (3 * (batch.SPLIT_LEN_DEFAULT or 2**20) + 5,))]
    out = []
    for k in SPLIT_KS:
        out += [(k, SPLIT_LENS), (k, (21257,)), (k, (6145,))]
    # more long streams than the launch's work list records (1024): the ones beyond it are done whole
    out += [(64, tuple(2049 + s % 7 for s in range(1100))), (512, tuple(2049 + 3 * (s % 5) for s in range(1040)))]
    return out


def _split_child(setting, path):
    import torch

    from reservoir_amd import batch

    cuda = torch.device("cuda", 0)
    got = {}
    for n, (k, lens) in enumerate(_split_launches(setting)):
        idx, cnt = batch.sample_segmented_indexed(_dev(torch, cuda, _offsets(lens)), k, SEED, BASE)
        got[f"idx{n}"], got[f"cnt{n}"] = idx.cpu().numpy(), cnt.cpu().numpy()
    np.savez(path, **got)


@pytest.mark.parametrize("setting", ["2048", "0", None])
def test_split_form_equals_the_oracle(cuda, oracle, setting):
    """RSV_K2_SPLIT_LEN is read once per process, so each setting runs in a fresh child: 2048 (pieces, k at and
    above the split length: fill indices span pieces), 0 (no split) and unset (the default length)."""
    env = {k: v for k, v in os.environ.items() if k != "RSV_K2_SPLIT_LEN"}
    if setting is not None:
        env["RSV_K2_SPLIT_LEN"] = setting
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "split.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(setting), path], env=env,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.load(path)
        for n, (k, lens) in enumerate(_split_launches(setting)):
            widx = np.stack([oracle.algo_r_last_writers(SEED, BASE + s, k, 0, int(ln), 0) for s, ln in enumerate(lens)])
            assert np.array_equal(got[f"idx{n}"], widx), (setting, k, lens)
            assert np.array_equal(got[f"cnt{n}"], np.minimum(np.array(lens), k)), (setting, k, lens)


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "child":
    sys.path.insert(0, ROOT)
    _split_child(None if sys.argv[2] == "None" else sys.argv[2], sys.argv[3])
