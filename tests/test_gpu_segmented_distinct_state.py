"""Resumed segmented Sampler.distinct (K5 with state: rsv_distinct_segmented_update / _merge,
batch.SegmentedDistinct): S long-lived distinct samplers advanced by one launch per batch and
combined across launches.

Bottom-k by (scrambled hash, key) over distinct keys is a function of the key set alone, so however
a stream is cut into updates or split into merged parts, its row must equal -- exactly: keys, hashes,
counts, zeros beyond the count -- the value computed here with numpy over the CONCATENATED stream:

    h = byteswap64(r1 ^ byteswap64(r0 ^ hash(u)))   for u = the stream's distinct keys
    order = lexsort((u, h))[:k]

with (r0, r1) from oracle.Distinct(k, seed_s).r0/.r1, and batch.distinct_segmented over the
concatenation.  The constructor zero-fills the counts only and an update leaves a row without keys
alone, so a row that never received a key is compared by its count (0) alone.
"""
import ctypes as C

import numpy as np
import pytest
from segdistinct_ref import _expected, _hash_np, _r01, _scramble, _with_repeats

pytestmark = pytest.mark.gpu


def _offs(lens):
    return np.r_[0, np.cumsum(lens)].astype(np.int64)


def _cuts(rng, lens, B):
    """Random cut positions: cuts[s] = 0 <= c_1 <= ... <= c_{B-1} <= len_s, as an (S, B + 1) array."""
    S = lens.size
    c = np.sort(rng.integers(0, lens[:, None] + 1, size=(S, B - 1)), axis=1)
    return np.concatenate([np.zeros((S, 1), dtype=np.int64), c, lens[:, None]], axis=1).astype(np.int64)


def _piece(offs, cuts, t, *arrays):
    """Batch t of the cut streams: (its offsets, the flat pieces of every array)."""
    ln = cuts[:, t + 1] - cuts[:, t]
    po = _offs(ln)
    idx = np.repeat(offs[:-1] + cuts[:, t] - po[:-1], ln) + np.arange(int(po[-1]))
    return (po,) + tuple(a[idx] for a in arrays)


def _stateless(cuda, keys, offs, k, seed, base, **kw):
    import torch

    from reservoir_amd import batch

    if "hashes" in kw:
        kw["hashes"] = torch.from_numpy(kw["hashes"]).to(cuda)
    return batch.distinct_segmented(torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda), k, seed=seed,
                                    stream_base=base, **kw)


def _new(cuda, S, k, seed, base, hash="identity", dtype=None):
    import torch

    from reservoir_amd import batch

    return batch.SegmentedDistinct(S, k, seed, stream_base=base, hash=hash, dtype=dtype or torch.int64, device=cuda)


def _feed(sd, cuda, po, keys, hashes=None, ids=None, **kw):
    import torch

    return sd.update(torch.from_numpy(keys).to(cuda), torch.from_numpy(po).to(cuda),
                     stream_ids=None if ids is None else torch.from_numpy(ids).to(cuda),
                     hashes=None if hashes is None else torch.from_numpy(hashes).to(cuda), **kw)


def _state(sd):
    return sd.keys.cpu().numpy(), sd.hashes.cpu().numpy(), sd.counts.cpu().numpy()


def _check(got, want, touched=None):
    gk, gh, gc = got
    wk, wh, wc = (w.cpu().numpy() if hasattr(w, "cpu") else w for w in want)
    assert np.array_equal(gc, wc)
    gk, gh = gk.astype(np.int64), gh.copy()
    if touched is not None:  # rows that never received a key: the count says empty, the slots are not the engine's
        assert not gc[~touched].any()
        gk[~touched] = 0
        gh[~touched] = 0
    assert np.array_equal(gh, wh)
    assert np.array_equal(gk, wk.astype(np.int64))  # slots beyond the count are 0 on both sides


def _first_with_distinct(seg, d):
    """The shortest prefix length of seg holding exactly d distinct keys."""
    _, first = np.unique(seg, return_index=True)
    first = np.sort(first)
    assert first.size > d
    return int(first[d])  # the position of the (d+1)-th new key: the prefix before it has d


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("k", [1, 2, 64, 65, 256, 257, 1024, 1025, 4096])
def test_batch_split_invariance(cuda, oracle, k, B):
    """B update launches over randomly cut ragged streams = numpy = one stateless launch = the oracle."""
    rng = np.random.default_rng(k * 10 + B)
    big = k >= 1000
    S = 60 if big else 300
    top = 4 * k + 5000 if big else 5000
    lens = rng.integers(0, top, size=S)
    lens[:8] = [0, 1, top, top, top, k, 4096, 3]
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(k, int(offs[-1])), offs)
    cuts = _cuts(rng, lens, B)
    cuts[6, 1:B] = [1] + [1] * (B - 2)            # a 1-element piece, then empty pieces (B = 5), then the rest
    cuts[5, 1:B] = 0                              # empty pieces first
    for s, d in ((2, k - 1), (3, k), (4, k + 1)):  # the first piece holds exactly k - 1, k, k + 1 distinct keys
        c = _first_with_distinct(keys[offs[s]:offs[s + 1]], d)
        cuts[s, 1:B] = np.maximum(np.sort(cuts[s, 1:B]), c)
        cuts[s, 1] = c
        assert np.unique(keys[offs[s]:offs[s] + c]).size == d
    assert (np.diff(cuts, axis=1) >= 0).all()
    assert (np.diff(cuts, axis=1) % 256 != 0).any() and (np.diff(cuts, axis=1) == 0).any()
    seed, base = 77, 1000
    r0, r1 = _r01(oracle, k, seed, base, S)
    want = _expected(keys, keys, offs, k, r0, r1)
    sd = _new(cuda, S, k, seed, base)
    for t in range(B):
        po, pk = _piece(offs, cuts, t, keys)
        assert _feed(sd, cuda, po, pk) is sd
    got = _state(sd)
    _check(got, want, lens > 0)
    _check(got, _stateless(cuda, keys, offs, k, seed, base, hash="identity"), lens > 0)
    for s in range(S):  # the oracle's RandomValues per stream (injective hash: the same set)
        ref = oracle.Distinct(k, seed + base + s, oracle.HASH_IDENTITY)
        ref.sample_all(keys[offs[s]:offs[s + 1]])
        rk, rh = ref.result()
        m = int(got[2][s])
        assert m == rk.size, s
        assert np.array_equal(got[0][s, :m], rk) and np.array_equal(got[1][s, :m], rh), s


@pytest.mark.parametrize("k", [64, 257, 1024, 4096])
def test_full_set_admits_nothing(cuda, oracle, k):
    """A full row against a batch above its last entry (bit-identical afterwards), then one below its
    first entry (the row is replaced), then repeats of its members (unchanged)."""
    import torch

    S, n = 6, 4 * k
    offs = np.arange(0, S * n + 1, n, dtype=np.int64)
    keys = oracle.splitmix_keys(k + 1, S * n)
    assert np.unique(keys).size == keys.size
    seed, base = 21, 5
    r0, r1 = _r01(oracle, k, seed, base, S)
    sid = np.repeat(np.arange(S), n)
    asc = keys[np.lexsort((keys, _scramble(r0[sid], r1[sid], keys), sid))].reshape(S, n)  # each stream's own order
    rng = np.random.default_rng(k)

    def feed(sd, cols):
        part = rng.permuted(cols, axis=1)
        return _feed(sd, cuda, np.arange(0, part.size + 1, part.shape[1], dtype=np.int64), part.reshape(-1).copy())

    def want_of(cols):
        flat = np.ascontiguousarray(cols).reshape(-1)
        return _expected(flat, flat, np.arange(0, flat.size + 1, cols.shape[1], dtype=np.int64), k, r0, r1)

    sd = _new(cuda, S, k, seed, base)
    feed(sd, asc[:, 2 * k:3 * k + 7])
    _check(_state(sd), want_of(asc[:, 2 * k:3 * k]))
    before = [t.clone() for t in (sd.keys, sd.hashes, sd.counts)]
    feed(sd, asc[:, 3 * k:])  # every (h, key) above the row's last entry
    assert all(torch.equal(a, b) for a, b in zip(before, (sd.keys, sd.hashes, sd.counts)))
    feed(sd, asc[:, :k])  # every (h, key) below the row's first entry
    _check(_state(sd), want_of(asc[:, :k]))
    assert np.array_equal(_state(sd)[0], asc[:, :k])
    before = [t.clone() for t in (sd.keys, sd.hashes, sd.counts)]
    feed(sd, np.concatenate([asc[:, :k], asc[:, :k]], axis=1))  # current members only
    assert all(torch.equal(a, b) for a, b in zip(before, (sd.keys, sd.hashes, sd.counts)))


@pytest.mark.parametrize("k", [5, 64, 512])
@pytest.mark.parametrize("mode", ["java_long", "precomputed"])
def test_ties_across_batches(cuda, oracle, k, mode):
    """Long.hashCode folded to 300 values; precomputed key % 37.  Split in three: every admission after
    the first batch is a tie on h, decided by the key against the loaded T."""
    rng = np.random.default_rng(k * 7 + len(mode))
    lens = rng.integers(0, 3000, size=100)
    offs = _offs(lens)
    x = _with_repeats(rng, oracle.splitmix_keys(k + 9, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 4, 50, lens.size)
    cuts = _cuts(rng, lens, 3)
    if mode == "java_long":
        keys = ((x >> 32) << 32) | (((x >> 32) ^ (x % 300)) & 0xFFFFFFFF)
        hashed = _hash_np(keys, "java_long")
        assert np.unique(hashed).size <= 300
        sd = _new(cuda, lens.size, k, 4, 50, hash="java_long")
        for t in range(3):
            po, pk = _piece(offs, cuts, t, keys)
            _feed(sd, cuda, po, pk)
        ref = _stateless(cuda, keys, offs, k, 4, 50, hash="java_long")
    else:
        keys = x
        hashed = keys % 37
        sd = _new(cuda, lens.size, k, 4, 50, hash="precomputed")
        for t in range(3):
            po, pk, ph = _piece(offs, cuts, t, keys, hashed)
            _feed(sd, cuda, po, pk, hashes=ph)
        ref = _stateless(cuda, keys, offs, k, 4, 50, hashes=hashed)
    _check(_state(sd), _expected(keys, hashed, offs, k, r0, r1), lens > 0)
    _check(_state(sd), ref, lens > 0)


@pytest.mark.parametrize("k", [17, 600])
@pytest.mark.parametrize("hash", ["java_int", "default"])
def test_int32_keys(cuda, oracle, k, hash):
    import torch

    rng = np.random.default_rng(k)
    lens = rng.integers(0, 3000, size=100)
    offs = _offs(lens)
    n = int(offs[-1])
    keys = np.where(rng.random(n) < 0.5, rng.integers(-2**31, 2**31, size=n), rng.integers(-700, 700, size=n))
    keys = keys.astype(np.int32)
    assert (keys < 0).any()
    r0, r1 = _r01(oracle, k, 9, 0, lens.size)
    cuts = _cuts(rng, lens, 3)
    sd = _new(cuda, lens.size, k, 9, 0, hash=hash, dtype=torch.int32)
    for t in range(3):
        po, pk = _piece(offs, cuts, t, keys)
        _feed(sd, cuda, po, pk)
    assert sd.keys.dtype == torch.int32 and sd.hashes.dtype == torch.int64
    _check(_state(sd), _expected(keys, _hash_np(keys, "java_int"), offs, k, r0, r1), lens > 0)


def test_stream_ids_permutation_and_subset(cuda, oracle):
    """Segments in a random order of all rows; then a third of the rows, the others pre-filled with a
    sentinel pattern in keys, hashes and counts that must come back unchanged."""
    import torch

    rng = np.random.default_rng(5)
    k, S = 50, 120
    lens = rng.integers(0, 2000, size=S)
    lens[:2] = [0, 1]
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(5, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 3, 10, S)
    want = _expected(keys, keys, offs, k, r0, r1)
    cuts = _cuts(rng, lens, 2)
    sd = _new(cuda, S, k, 3, 10)
    for t in range(2):
        perm = rng.permutation(S)  # segment b of the launch belongs to row perm[b]
        poffs = _offs(lens[perm])
        pkeys = np.concatenate([keys[offs[s]:offs[s + 1]] for s in perm])
        po, pk = _piece(poffs, cuts[perm], t, pkeys)
        _feed(sd, cuda, po, pk, ids=perm.astype(np.int64))
    _check(_state(sd), want, lens > 0)

    named = np.sort(rng.permutation(S)[:S // 3])
    mask = np.zeros(S, dtype=bool)
    mask[named] = True
    sd = _new(cuda, S, k, 3, 10)
    sent_k = torch.arange(S * k, dtype=torch.int64, device=cuda).reshape(S, k) * 7 - 11
    sent_h = -sent_k - 3
    sent_c = torch.arange(S, dtype=torch.int64, device=cuda) % (k + 1)
    sd.keys.copy_(sent_k)
    sd.hashes.copy_(sent_h)
    sd.counts.copy_(sent_c)
    sd.counts[torch.from_numpy(named).to(cuda)] = 0
    noffs = _offs(lens[named])
    nkeys = np.concatenate([keys[offs[s]:offs[s + 1]] for s in named])
    for t in range(2):
        po, pk = _piece(noffs, cuts[named], t, nkeys)
        _feed(sd, cuda, po, pk, ids=named.astype(np.int64))
    gk, gh, gc = _state(sd)
    assert np.array_equal(gk[~mask], sent_k.cpu().numpy()[~mask])
    assert np.array_equal(gh[~mask], sent_h.cpu().numpy()[~mask])
    assert np.array_equal(gc[~mask], sent_c.cpu().numpy()[~mask])
    live = mask & (lens > 0)
    assert np.array_equal(gk[live], want[0][live]) and np.array_equal(gh[live], want[1][live])
    assert np.array_equal(gc[mask], want[2][mask])


def test_reversed_ids_grid_stride(cuda, oracle):
    """S = 100,003 short segments in reversed row order, two updates: more rows than the grid holds."""
    rng = np.random.default_rng(100_003)
    S, k = 100_003, 8
    lens = rng.integers(0, 41, size=S)
    offs = _offs(lens)
    keys = rng.integers(-60, 60, size=int(offs[-1])).astype(np.int64) * 0x9E3779B97F4A7
    base = 2**63 - 50_000  # the seed wraps past INT64_MAX inside the launch
    r0, r1 = _r01(oracle, k, 12, base, S)
    want = _expected(keys, keys, offs, k, r0, r1)
    cuts = _cuts(rng, lens, 2)
    rev = np.arange(S - 1, -1, -1, dtype=np.int64)
    sid = np.repeat(np.arange(S), lens)
    order = np.lexsort((np.arange(sid.size), -sid))  # the streams reversed, each in its own order
    rkeys, roffs = keys[order], _offs(lens[rev])
    sd = _new(cuda, S, k, 12, base)
    for t in range(2):
        po, pk = _piece(roffs, cuts[rev], t, rkeys)
        _feed(sd, cuda, po, pk, ids=rev)
    _check(_state(sd), want, lens > 0)


def test_check_ids_raises_before_any_launch(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException

    sd = _new(cuda, 10, 4, 1, 0)
    sd.keys.fill_(-1)
    sd.hashes.fill_(-2)
    keys = torch.arange(12, dtype=torch.int64, device=cuda)
    offs = torch.tensor([0, 4, 8, 12], dtype=torch.int64, device=cuda)
    for ids in ([1, 5, 1], [0, 10, 2], [-1, 3, 4]):
        with pytest.raises(IllegalArgumentException):
            sd.update(keys, offs, stream_ids=torch.tensor(ids, dtype=torch.int64, device=cuda))
    torch.cuda.synchronize()
    assert not sd.counts.any() and (sd.keys == -1).all() and (sd.hashes == -2).all()
    with pytest.raises(IllegalArgumentException):  # one id per segment
        sd.update(keys, offs, stream_ids=torch.tensor([1, 2], dtype=torch.int64, device=cuda))
    sd.update(keys, offs, stream_ids=torch.tensor([9, 0, 4], dtype=torch.int64, device=cuda))
    assert sd.counts.cpu().tolist() == [4, 0, 0, 0, 4, 0, 0, 0, 0, 4]


@pytest.mark.parametrize("mode", ["identity", "precomputed"])
@pytest.mark.parametrize("P", [1, 2, 8])
@pytest.mark.parametrize("k", [5, 256, 257, 1024, 1025])
def test_merge(cuda, oracle, k, P, mode):
    """Streams split by index into P parts, each sampled by the stateless call, stacked and merged:
    into an empty state and into a non-empty one; then the merged row is resumed by one more update."""
    import torch

    rng = np.random.default_rng(k * 100 + P + len(mode))
    big = k >= 1000
    S = 40 if big else 100
    top = 4 * k + 5000 if big else 5000
    lens = rng.integers(0, top, size=S)
    lens[:5] = [0, 1, top, k, 3 * k + 50]
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(k + P, int(offs[-1])), offs)
    hashed = keys % 37 if mode == "precomputed" else keys
    seed, base = 31, 400
    r0, r1 = _r01(oracle, k, seed, base, S)

    def kw(h):
        return dict(hashes=h) if mode == "precomputed" else dict(hash="identity")

    cuts = _cuts(rng, lens, P + 2)  # piece 0 seeds the non-empty state, 1..P are the parts, P + 1 resumes
    cuts[2, 1:3] = [k + 10, 4 * k + 20]  # stream 2: part 1 holds 3k + 10 keys, more than k distinct
    cuts[2, 3:P + 2] = np.maximum(cuts[2, 3:P + 2], 4 * k + 20)
    cuts[3, 2:P + 1] = cuts[3, 1]        # stream 3: empty parts (count 0) beside a non-empty one
    assert (np.diff(cuts, axis=1) >= 0).all()
    assert np.unique(keys[offs[2] + k + 10:offs[2] + 4 * k + 20]).size > k
    parts = []
    for p in range(1, P + 1):
        po, pk, ph = _piece(offs, cuts, p, keys, hashed)
        parts.append(_stateless(cuda, pk, po, k, seed, base, **kw(ph)))
    pk_, ph_, pc_ = (torch.stack([x[i] for x in parts]) for i in range(3))
    pc = pc_.cpu().numpy()
    if mode == "identity":
        assert (pc == 0).any() and ((pc > 0) & (pc < k)).any() and (pc == k).any()

    def want_of(a, b):  # the stateless value over pieces [a, b) of every stream
        sub = np.stack([cuts[:, a], cuts[:, b]], axis=1)
        po, pk, ph = _piece(offs, sub, 0, keys, hashed)
        return po, pk, ph, _expected(pk, ph, po, k, r0, r1)

    # into an empty state
    sd = _new(cuda, S, k, seed, base, hash=mode)
    assert sd.merge(pk_, ph_, pc_) is sd
    po, pk, ph, want = want_of(1, P + 1)
    _check(_state(sd), want, np.diff(po) > 0)
    _check(_state(sd), _stateless(cuda, pk, po, k, seed, base, **kw(ph)), np.diff(po) > 0)

    # into a non-empty state, then one more update on the merged rows
    sd = _new(cuda, S, k, seed, base, hash=mode)
    po, pk, ph = _piece(offs, cuts, 0, keys, hashed)
    _feed(sd, cuda, po, pk, hashes=ph if mode == "precomputed" else None)
    sd.merge(pk_, ph_, pc_)
    po, pk, ph, want = want_of(0, P + 1)
    _check(_state(sd), want, np.diff(po) > 0)
    po, pk, ph = _piece(offs, cuts, P + 1, keys, hashed)
    _feed(sd, cuda, po, pk, hashes=ph if mode == "precomputed" else None)
    _check(_state(sd), _expected(keys, hashed, offs, k, r0, r1), lens > 0)
    _check(_state(sd), _stateless(cuda, keys, offs, k, seed, base, **kw(hashed)), lens > 0)


def test_merge_of_state_objects(cuda, oracle):
    """merge(other) and merge(a, b): the index-split recipe with SegmentedDistinct objects."""
    rng = np.random.default_rng(17)
    k, S = 40, 50
    lens = rng.integers(0, 1500, size=S)
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(17, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 2, 0, S)
    cuts = _cuts(rng, lens, 3)
    sds = []
    for t in range(3):
        po, pk = _piece(offs, cuts, t, keys)
        sds.append(_feed(_new(cuda, S, k, 2, 0), cuda, po, pk))
    a = _new(cuda, S, k, 2, 0).merge(sds[0]).merge(sds[1], sds[2])
    _check(_state(a), _expected(keys, keys, offs, k, r0, r1), lens > 0)
    from reservoir_amd import IllegalArgumentException

    with pytest.raises(IllegalArgumentException):
        a.merge(_new(cuda, S, k, 3, 0))  # another seed: its hashes mean something else


@pytest.mark.parametrize("k", [10, 700])
def test_handle_equivalence(cuda, oracle, k):
    """One Sampler.distinct(k, seed=seed+base+s, order="set") handle per stream, fed the same batches."""
    import torch

    from reservoir_amd import Sampler

    rng = np.random.default_rng(k)
    S, B = 6, 4
    lens = rng.integers(0, 6000, size=S)
    lens[1] = k // 2
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(k, int(offs[-1])), offs)
    cuts = _cuts(rng, lens, B)
    sd = _new(cuda, S, k, 40, 7)
    handles = [Sampler.distinct(k, seed=40 + 7 + s, order="set")(hash="identity") for s in range(S)]
    for t in range(B):
        po, pk = _piece(offs, cuts, t, keys)
        _feed(sd, cuda, po, pk)
        for s in range(S):
            if po[s + 1] > po[s]:
                handles[s].sample_all(torch.from_numpy(pk[po[s]:po[s + 1]]).to(cuda))
    gk, _, gc = _state(sd)
    for s in range(S):
        assert np.array_equal(handles[s].result(), gk[s, :gc[s]]), s


def test_stream_order_and_repeatability(cuda, oracle):
    """4 updates queued back to back on a non-default torch stream with check_ids=False, no host wait
    between them, one synchronize; two identical runs are bit-identical."""
    import torch

    rng = np.random.default_rng(8)
    k, S, B = 100, 200, 4
    lens = rng.integers(0, 3000, size=S)
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(2, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 6, 0, S)
    want = _expected(keys, keys, offs, k, r0, r1)
    cuts = _cuts(rng, lens, B)
    ids = torch.arange(S, dtype=torch.int64, device=cuda)
    dev = []
    for t in range(B):
        po, pk = _piece(offs, cuts, t, keys)
        dev.append((torch.from_numpy(pk).to(cuda), torch.from_numpy(po).to(cuda)))
    runs = [_new(cuda, S, k, 6, 0), _new(cuda, S, k, 6, 0)]
    for sd in runs:  # equal starting bytes, so that the rows no key reaches compare equal too
        sd.keys.zero_()
        sd.hashes.zero_()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        for sd in runs:
            for pk, po in dev:
                sd.update(pk, po, stream_ids=ids, check_ids=False)
    st.synchronize()
    _check(_state(runs[0]), want)
    assert all(torch.equal(x, y) for x, y in zip(*[(sd.keys, sd.hashes, sd.counts) for sd in runs]))


def test_raw_abi_null_stream_ids(cuda, oracle):
    """The C ABI through ctypes: two updates with stream_ids_dev = NULL, then a merge of the row set
    into a second state."""
    import torch

    from reservoir_amd import _native as N

    rng = np.random.default_rng(9)
    k, S = 100, 200
    lens = rng.integers(0, 3000, size=S)
    lens[0] = 0
    offs = _offs(lens)
    keys = _with_repeats(rng, oracle.splitmix_keys(3, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 6, 2, S)
    want = _expected(keys, keys, offs, k, r0, r1)
    cuts = _cuts(rng, lens, 2)
    L = N.load()
    vp = C.c_void_p
    stream = vp(torch.cuda.current_stream(cuda).cuda_stream)

    def state():
        return (torch.full((S, k), -1, dtype=torch.int64, device=cuda), torch.full((S, k), -1, dtype=torch.int64, device=cuda),
                torch.zeros(S, dtype=torch.int64, device=cuda))

    sk, sh, sc = state()
    for t in range(2):
        po, pk = _piece(offs, cuts, t, keys)
        kd, od = torch.from_numpy(pk).to(cuda), torch.from_numpy(po).to(cuda)
        N.check(L.rsv_distinct_segmented_update(
            vp(kd.data_ptr()), None, vp(od.data_ptr()), None, S, S, 8, k, N.HASH_IDENTITY, 6, 2,
            vp(sk.data_ptr()), vp(sh.data_ptr()), vp(sc.data_ptr()), stream))
        torch.cuda.synchronize()
    got = (sk.cpu().numpy(), sh.cpu().numpy(), sc.cpu().numpy())
    assert (got[0][0] == -1).all() and (got[1][0] == -1).all()  # the row without keys was not written
    _check(got, want, lens > 0)
    mk, mh, mc = state()
    N.check(L.rsv_distinct_segmented_merge(vp(sk.data_ptr()), vp(sh.data_ptr()), vp(sc.data_ptr()), 1, S, 8, k,
                                           vp(mk.data_ptr()), vp(mh.data_ptr()), vp(mc.data_ptr()), stream))
    torch.cuda.synchronize()
    _check((mk.cpu().numpy(), mh.cpu().numpy(), mc.cpu().numpy()), want, lens > 0)


def test_bad_arguments_raise(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, NullPointerException, ReservoirError, batch

    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinct(4, 0, 1, device=cuda)
    with pytest.raises(ReservoirError, match="4096"):
        batch.SegmentedDistinct(4, 4097, 1, device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.SegmentedDistinct(4, 4, 1, hash="md5", device=cuda)
    sd = batch.SegmentedDistinct(2, 4, 1, device=cuda)
    keys = torch.arange(10, dtype=torch.int64, device=cuda)
    offs = torch.tensor([0, 3, 6, 10], dtype=torch.int64, device=cuda)
    with pytest.raises(IllegalArgumentException):
        sd.update(keys.cpu(), offs)
    with pytest.raises(IllegalArgumentException):
        sd.update(keys.to(torch.int32), offs)
    with pytest.raises(IllegalArgumentException):  # three segments, two rows, no ids
        sd.update(keys, offs)
    with pytest.raises(IllegalArgumentException):
        sd.update(keys, offs[:3], hashes=keys[:6])  # hashes without hash="precomputed"
    with pytest.raises(NullPointerException):
        batch.SegmentedDistinct(2, 4, 1, hash="precomputed", device=cuda).update(keys, offs[:3])
    with pytest.raises(IllegalArgumentException):
        sd.merge(sd.keys[:1], sd.hashes[:1], sd.counts[:1])
    assert not sd.counts.any()
