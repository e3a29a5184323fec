"""rsv_distinct_segmented_candidates and batch.SegmentedObjectDistinct on the GPU: Sampler.distinct for any B over
many streams per launch, the engine reading hashes only.

Every launch here goes through the raw entry point on sentinel-padded buffers (outputs and state), and the pads
are checked after each one.  The reference per stream is RandomValues over the whole stream (segobj_ref), the
oracle's DistinctRows over 16-byte rows of the element ids, and -- for tightness -- the exact running T.
"""
import bisect
import ctypes as C

import hash_targets as HT
import numpy as np
import pytest
import segobj_ref as R
from segdistinct_ref import _wrap

pytestmark = pytest.mark.gpu

PAD = 64
SENT = -0x0123456789ABCDEF
MIN, MAX = HT.MIN, HT.MAX
M64 = 2**64 - 1


class Buf:
    """n int64 on the device between two pads of sentinels."""

    def __init__(self, cuda, n, fill=SENT):
        import torch

        self.n = n
        self.full = torch.full((n + 2 * PAD,), SENT, dtype=torch.int64, device=cuda)
        self.t = self.full[PAD:PAD + n]
        if fill != SENT:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr()) if self.n else C.c_void_p(self.full.data_ptr() + 8 * PAD)

    def intact(self):
        return bool((self.full[:PAD] == SENT).all()) and bool((self.full[PAD + self.n:] == SENT).all())

    def host(self):
        return self.t.cpu().numpy().copy()


class State:
    """The four caller-held tensors of S rows, padded; counts zero, the slots sentinels (a row with count 0 is
    empty whatever its slots hold)."""

    def __init__(self, cuda, S, k, bound=True):
        self.S, self.k = S, k
        self.sh, self.sc = Buf(cuda, S * k), Buf(cuda, S, 0)
        self.sizes = Buf(cuda, S, 0) if bound else None
        self.maxh = Buf(cuda, S, MIN) if bound else None

    def bufs(self):
        return [b for b in (self.sh, self.sc, self.sizes, self.maxh) if b is not None]

    def snapshot(self):
        return [b.full.cpu().numpy().copy() for b in self.bufs()]

    def set_row(self, r, values):
        import torch

        v = np.sort(np.asarray(values, dtype=np.int64))
        self.sh.t[r * self.k:r * self.k + v.size] = torch.from_numpy(v).to(self.sh.t.device)
        self.sc.t[r] = v.size


def _dev(cuda, a):
    import torch

    a = np.ascontiguousarray(a, dtype=np.int64)
    return torch.from_numpy(a).to(cuda) if a.size else torch.zeros(1, dtype=torch.int64, device=cuda)


def launch(cuda, hashed, offs, k, seed, base, cap, st, ids=None):
    """One raw launch; returns (pos (B, cap), hs (B, cap), counts (B,)) on the host, entries never written being
    SENT.  Checks every pad."""
    import torch

    from reservoir_amd import _native as N

    B = offs.size - 1
    hd, od = _dev(cuda, hashed), _dev(cuda, offs)
    idd = _dev(cuda, ids) if ids is not None else None
    pos, hs, cnt = Buf(cuda, B * cap), Buf(cuda, B * cap), Buf(cuda, B)
    N.check(N.load().rsv_distinct_segmented_candidates(
        C.c_void_p(hd.data_ptr()), C.c_void_p(od.data_ptr()), C.c_void_p(idd.data_ptr()) if idd is not None else None,
        B, st.S, k, seed & M64, base & M64, st.sh.ptr, st.sc.ptr, st.sizes.ptr if st.sizes else None,
        st.maxh.ptr if st.maxh else None, pos.ptr, hs.ptr, cap, cnt.ptr,
        C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
    torch.cuda.synchronize()
    for b in [pos, hs, cnt] + st.bufs():
        assert b.intact(), "a launch wrote outside its buffers"
    return pos.host().reshape(B, cap), hs.host().reshape(B, cap), cnt.host()


def _ids(rng, n, repeats=0.3):
    """n element ids (64-bit, so the identity is an injective hash), a share of them repeats of earlier ones"""
    ids = rng.integers(MIN, MAX, size=n, dtype=np.int64)
    if n > 1:
        again = rng.random(n) < repeats
        ids = np.where(again, ids[rng.integers(0, np.maximum(np.arange(n), 1))], ids)
    return ids


def _hashed(ids, hash):
    return ids if hash == "injective" else ids % 97


def _offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _oracle_set(oracle, k, seed, ids, hashed):
    ref = oracle.DistinctRows(k, seed, 16)
    ref.sample_all(R.rows16(ids), hashed)
    rows, hs = ref.result()
    return sorted(bytes(r) for r in rows), sorted(hs.tolist())


def check_stream(oracle, k, seed_r, ids, hashed, sh, cand, ch):
    """One stream against the reference.  ids / hashed / sh: its elements, their hashes, scrambled; cand / ch: the
    candidates' positions inside the stream and the hashes returned with them."""
    n = ids.size
    assert np.all(np.diff(cand) > 0), "positions strictly ascending"
    assert cand.size == 0 or (cand[0] >= 0 and cand[-1] < n), "positions inside the segment"
    assert np.array_equal(ch, sh[cand]), "out_hashes are the scrambled hashes at those positions"
    adm, want = R.admissions(k, ids, sh)
    assert np.isin(adm, cand).all(), "an element the reference admits is missing"
    got = R.replay(k, ids, sh, cand)
    assert R.same_replica(got, want), "the replay of the candidates is not the reference's heap"
    es, hs = got.heap()
    rows, ohs = _oracle_set(oracle, k, seed_r, ids, hashed)
    assert sorted(bytes(r) for r in R.rows16(np.array(es, dtype=np.int64))) == rows and sorted(hs) == ohs
    return got


def _lengths(k):
    nt, w = R.form_of(k)
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, nt * 4 - 1, nt * 4, nt * 4 + 1, 8 * w]


@pytest.mark.parametrize("hash", ["injective", "colliding"])
@pytest.mark.parametrize("k", [1, 2, 64, 65, 256, 257, 1024, 1025, 4096])
def test_sound_and_exact(cuda, oracle, k, hash):
    """Fresh rows, one launch, every length at which the loop takes another path (both sides of a step, of a
    chunk of NT x 4, of the set's size) and one of eight buffers, so that several merges run."""
    rng = np.random.default_rng(7 * k + (hash == "colliding"))
    lens = _lengths(k)
    offs = _offs(lens)
    ids = _ids(rng, int(offs[-1]))
    hashed = _hashed(ids, hash)
    seed, base = 0xA11CE, 3
    sh = R.scrambled(oracle, k, seed, base, hashed, offs)
    cap = max(lens)
    pos, hs, cnt = launch(cuda, hashed, offs, k, seed, base, cap, State(cuda, len(lens), k, bound=False))
    for b, n in enumerate(lens):
        a = int(offs[b])
        assert 0 <= cnt[b] <= n
        c = int(cnt[b])
        assert (pos[b, c:] == SENT).all() and (hs[b, c:] == SENT).all()
        check_stream(oracle, k, _wrap(seed + base + b), ids[a:a + n], hashed[a:a + n], sh[a:a + n], pos[b, :c] - a,
                     hs[b, :c])
    if hash == "injective":  # a long stream is filtered: the bound is in force
        assert cnt[-1] < lens[-1] // 2


@pytest.mark.parametrize("k,B,top", [(8, 33_000, 40), (4096, 1_100, 300)])
def test_teams_take_one_stream_after_another(cuda, oracle, k, B, top):
    """More segments than the launch's grid (32 768 teams at k = 8, 1 024 at k = 4096), short streams.  A fresh
    row is open for its first step at least, and these streams end inside it (k = 8) or never hold k distinct
    hashes (k = 4096): every element is a candidate, which numpy states for all rows; a sample of the rows is
    replayed against the reference as well."""
    rng = np.random.default_rng(k)
    lens = rng.integers(0, top + 1, size=B)
    lens[[0, 1, B - 1]] = [top, 0, top]
    offs = _offs(lens)
    ids = _ids(rng, int(offs[-1]))
    seed, base = 77, 2**63
    sh = R.scrambled(oracle, k, seed, base, ids, offs)
    st = State(cuda, B, k, bound=False)
    pos, hs, cnt = launch(cuda, ids, offs, k, seed, base, top, st)
    assert np.array_equal(cnt, lens)
    keep = np.arange(top)[None, :] < lens[:, None]
    assert np.array_equal(pos[keep], np.arange(offs[-1])) and np.array_equal(hs[keep], sh)
    assert (pos[~keep] == SENT).all()
    for b in list(range(0, B, max(1, B // 60))) + [B - 1]:
        a, n = int(offs[b]), int(lens[b])
        check_stream(oracle, k, _wrap(seed + base + b), ids[a:a + n], ids[a:a + n], sh[a:a + n], pos[b, :n] - a, hs[b, :n])
    # the shadow each team left: the distinct scrambled hashes of its stream, the k smallest, ascending
    shd, scd = st.sh.host().reshape(B, k), st.sc.host()
    for b in (0, 1, 2, B // 2, B - 1):
        d = np.unique(sh[offs[b]:offs[b + 1]])[:k]
        assert scd[b] == d.size and np.array_equal(shd[b, :d.size], d) and (lens[b] == 0 or (shd[b, d.size:] == 0).all())


def _planted_launch(cuda, oracle, k, T, feed, seed=41, base=6, r=1, S=3):
    """Row r holds a full shadow whose k-th value is T (below it T - 3, T - 6, ... or down to MIN when T sits at
    the bottom); one segment of elements whose scrambled hashes are exactly `feed` goes into it."""
    st = State(cuda, S, k)
    members = [T] + [max(T - 3 * j, MIN + (k - 1 - j)) for j in range(1, k)]
    assert len(set(members)) == k and min(members) >= MIN
    st.set_row(r, members)
    r0, r1 = HT.r01(oracle, _wrap(seed + base + r))
    hashed = HT.plant(r0, r1, feed)
    before = st.snapshot()
    pos, hs, cnt = launch(cuda, hashed, np.array([0, len(feed)]), k, seed, base, max(len(feed), 1), st,
                          ids=np.array([r]))
    return pos[0], hs[0], int(cnt[0]), st, before


@pytest.mark.parametrize("k,T", [(2, t) for t in HT.EDGES if t != MIN] + [(1, t) for t in HT.EDGES if t != MIN] +
                         [(k, t) for k in (65, 300, 1100) for t in (-1, 0, MAX - 1, MAX)])
def test_exactly_T_is_no_candidate_and_T_minus_one_is(cuda, oracle, k, T):
    """h == T is refused -- a repeat of the k-th member and a distinct element sharing its hash look alike --
    T - 1 passes, and two distinct elements sharing a hash below T are both returned."""
    feed = [T, T - 1, T, MAX, T - 1, MIN, T, MIN]
    feed += [T] * 70 + [T - 1]  # and in a second step of the loop
    pos, hs, c, _, _ = _planted_launch(cuda, oracle, k, T, feed)
    want = [i for i, h in enumerate(feed) if h < T]
    assert c == len(want) and pos[:c].tolist() == want and hs[:c].tolist() == [feed[i] for i in want]


def test_open_row_returns_long_max(cuda, oracle):
    """An empty row, no bound from the caller: every element is a candidate, h == INT64_MAX included."""
    k, seed, base = 4, 41, 6
    feed = [5, MAX, 7, MAX, MIN]
    r0, r1 = HT.r01(oracle, _wrap(seed + base))
    for bound in (False, True):
        st = State(cuda, 1, k, bound=bound)
        pos, hs, cnt = launch(cuda, HT.plant(r0, r1, feed), np.array([0, 5]), k, seed, base, 8, st)
        assert cnt[0] == 5 and pos[0, :5].tolist() == [0, 1, 2, 3, 4] and hs[0, :5].tolist() == feed
        assert st.sc.host()[0] == 4 and st.sh.host()[:4].tolist() == [MIN, 5, 7, MAX]


@pytest.mark.parametrize("k", [1, 300])
def test_T_at_long_min_returns_nothing(cuda, oracle, k):
    """A full shadow whose T is INT64_MIN (k = 1), and a full row fed only hashes at or above its bound: zero
    candidates, and the four state tensors are byte-identical."""
    T = MIN if k == 1 else -5
    feed = [T, T + 1, MAX, 0 if k == 1 else T, T] * 30
    pos, hs, c, st, before = _planted_launch(cuda, oracle, k, T, feed)
    assert c == 0 and (pos == SENT).all() and (hs == SENT).all()
    assert all(np.array_equal(x, y) for x, y in zip(st.snapshot(), before))


def test_the_callers_bound_alone(cuda, oracle):
    """97 hash values under k = 100: the shadow never fills, so once the replica is full the candidates are exactly
    the elements below its maxHash as of the last replay."""
    k, seed, base, n = 100, 5, 0, 400
    rng = np.random.default_rng(97)
    st = State(cuda, 1, k)
    from reservoir_amd.values import RandomValues

    v, whole_ids, whole_sh = RandomValues(k), [], []
    for u in range(3):
        ids = _ids(rng, n)
        hashed = ids % 97
        sh = R.scrambled(oracle, k, seed, base, hashed, np.array([0, n]))
        size, maxh = v.size, v.max_hash
        pos, hs, cnt = launch(cuda, hashed, np.array([0, n]), k, seed, base, n, st)
        c = int(cnt[0])
        if u == 0:
            assert c == n  # open
        else:
            assert size == k
            assert np.array_equal(pos[0, :c], np.flatnonzero(sh < maxh))
        R.replay(k, ids, sh, pos[0, :c], v)
        st.sizes.t[0], st.maxh.t[0] = v.size, v.max_hash
        assert st.sc.host()[0] <= 97
        whole_ids.append(ids)
        whole_sh.append(sh)
    _, want = R.admissions(k, np.concatenate(whole_ids), np.concatenate(whole_sh))
    assert R.same_replica(v, want)


@pytest.mark.parametrize("k", [64, 256, 1024, 4096])
def test_a_bound_is_stale_by_one_buffer_at_most(cuda, oracle, k):
    """Tightness, from the design: T is refreshed by every merge, and a merge runs before the buffer of W
    entries overflows.  So a candidate i that the exact running T no longer admits was still admitted at some
    position j* <= i, and fewer than a buffer of candidates lie in [j*, i).  (A kernel that returns everything
    fails this at the end of the stream, one that never refreshes T as soon as T has fallen.)"""
    _, W = R.form_of(k)
    n = 8 * W
    # all distinct: an odd multiplier is a bijection on 64-bit words
    ids = (np.random.default_rng(k).permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(np.int64)
    seed, base = 2**64 - 1, 9
    sh = R.scrambled(oracle, k, seed, base, ids, np.array([0, n]))
    assert np.unique(sh).size == n
    pos, _, cnt = launch(cuda, ids, np.array([0, n]), k, seed, base, n, State(cuda, 1, k, bound=False))
    cand = pos[0, :int(cnt[0])]
    T = R.running_T(k, sh).tolist()
    neg = [-t for t in T]  # ascending: T never rises
    worst = 0
    for x, i in enumerate(cand.tolist()):
        h = int(sh[i])
        j = bisect.bisect_left(neg, -h, 0, i + 1) - 1  # the latest j <= i with T[j] > h; T[0] is above every hash
        assert j >= 0
        worst = max(worst, x - int(np.searchsorted(cand, j)))
    print(f"k={k} W={W} n={n} candidates={cand.size} worst={worst}")
    assert worst <= W
    admitted = [i for i, h in enumerate(sh.tolist()) if h < T[i]]  # and nothing the exact T admits is missing
    assert np.isin(admitted, cand).all()


def _host_update(cuda, oracle, st, reps, k, seed, base, ids, hashed, offs, rows, cap):
    """What a caller does with one batch: launch, replay per row, upload the replicas' size and maxHash."""
    sh = R.scrambled(oracle, k, seed, base, hashed, offs, rows=np.clip(rows, 0, st.S - 1))
    pos, hs, cnt = launch(cuda, hashed, offs, k, seed, base, cap, st, ids=rows)
    for b, r in enumerate(rows.tolist()):
        c = int(cnt[b])
        if not 0 <= r < st.S:
            assert c == 0 and (pos[b] == SENT).all()
            continue
        assert c <= cap
        assert np.array_equal(hs[b, :c], sh[pos[b, :c]])
        v = R.replay(k, ids, sh, pos[b, :c], reps.get(r))
        reps[r] = v
        st.sizes.t[r], st.maxh.t[r] = v.size, v.max_hash
    return cnt


@pytest.mark.parametrize("k", [5, 100, 1100])
def test_updates_in_pieces(cuda, oracle, k):
    """Six streams over ten rows through permuted ids, cut into 1, 2 and 8 updates, a non-zero stream_base and a
    seed that wraps past 2^64: the replicas are the single launch's and the reference's, rows no segment names
    keep every byte, ids outside the range are skipped with count 0."""
    S, seed, base = 10, 2**64 - 2, 5
    rng = np.random.default_rng(k)
    named = np.array([7, 2, 9, 0, 4, 3])
    lens = np.array([3 * k + 50, 2500, 0, 1, 6000 if k > 100 else 900, k])
    streams = [_ids(rng, int(n)) for n in lens]
    streams[1] = streams[1] % 50 + 1  # one stream with heavy repeats under a colliding hash
    final = {}
    for cuts in (1, 2, 8):
        st, reps = State(cuda, S, k), {}
        for r in (1, 5, 6, 8):  # unnamed rows: whatever they hold stays
            st.sh.t[r * k:(r + 1) * k] = 0x7777 + r
            st.sc.t[r] = (3, 10**9, -5, k)[r % 4]
        for t in range(cuts):
            pieces = [s[len(s) * t // cuts:len(s) * (t + 1) // cuts] for s in streams]
            order = rng.permutation(len(named))
            rows = np.concatenate([named[order], [-1, S]])  # and two segments no row takes
            segs = [pieces[i] for i in order] + [_ids(rng, 30), _ids(rng, 30)]
            ids = np.concatenate(segs)
            hashed = np.where(np.abs(ids) <= 50, ids % 7, ids)
            before = st.snapshot()
            _host_update(cuda, oracle, st, reps, k, seed, base, ids, hashed, _offs([len(s) for s in segs]), rows,
                         max(max(len(s) for s in segs), 1))
            after = st.snapshot()
            for r in (1, 5, 6, 8):
                assert np.array_equal(after[0][PAD + r * k:PAD + (r + 1) * k], before[0][PAD + r * k:PAD + (r + 1) * k])
                assert all(a[PAD + r] == b[PAD + r] for a, b in zip(after[1:], before[1:]))
        final[cuts] = {r: reps[r].heap() + (reps[r].max_hash,) for r in reps}
    assert final[1] == final[2] == final[8]
    for i, r in enumerate(named.tolist()):
        ids = streams[i]
        if ids.size == 0:
            assert final[1][r][0] == []
            continue
        hashed = np.where(np.abs(ids) <= 50, ids % 7, ids)
        sh = R.scrambled(oracle, k, seed, base, hashed, np.array([0, ids.size]), rows=[r])
        _, want = R.admissions(k, ids, sh)
        assert final[1][r] == want.heap() + (want.max_hash,)


def test_counts_are_clamped_and_garbage_with_count_zero_is_empty(cuda, oracle):
    k, n = 70, 400
    ids = _ids(np.random.default_rng(1), 3 * n)
    offs = _offs([n, n, n])
    st, clean = State(cuda, 3, k, bound=False), State(cuda, 3, k, bound=False)
    st.sh.t.fill_(0x5A5A5A5A5A5A5A5A)  # row 0: garbage slots, count 0
    st.sc.t[1] = -5  # row 1: clamped to 0
    st.sc.t[2] = 10**9  # row 2: clamped to k, the slots are what they are
    got = launch(cuda, ids, offs, k, 3, 0, n, st)
    want = launch(cuda, ids, offs, k, 3, 0, n, clean)
    for b in (0, 1):
        assert got[2][b] == want[2][b] and np.array_equal(got[0][b], want[0][b]) and np.array_equal(got[1][b], want[1][b])
        assert np.array_equal(st.sh.host()[b * k:(b + 1) * k], clean.sh.host()[b * k:(b + 1) * k])
    assert 0 <= got[2][2] <= n and (0 <= st.sc.host()[2] <= k or st.sc.host()[2] == 10**9)
    assert np.array_equal(st.sc.host()[:2], clean.sc.host()[:2])


def test_overflow_leaves_the_row_and_the_rerun_completes_it(cuda, oracle):
    k, seed, base = 64, 12, 1
    lens = [300, 5000, 0, 40, 2000]
    offs = _offs(lens)
    ids = _ids(np.random.default_rng(8), int(offs[-1]))
    big, small = State(cuda, 5, k), State(cuda, 5, k)
    P, H, Cn = launch(cuda, ids, offs, k, seed, base, 5000, big)
    before = small.snapshot()
    p, h, c = launch(cuda, ids, offs, k, seed, base, 8, small)
    assert np.array_equal(c, Cn) and (c[[0, 1, 3, 4]] > 8).all() and c[2] == 0
    over = np.flatnonzero(c > 8)
    for b in over:
        assert np.array_equal(p[b], P[b, :8]) and np.array_equal(h[b], H[b, :8])
    after = small.snapshot()
    assert all(np.array_equal(x, y) for x, y in zip(after, before)), "an overflowed row was written"
    # a launch in which only some segments overflow: the others advance as in the large-cap run
    mid = State(cuda, 5, k)
    cap = int(np.sort(Cn)[-2])
    p, h, c = launch(cuda, ids, offs, k, seed, base, cap, mid)
    assert np.array_equal(c, Cn) and (c > cap).sum() == 1
    worst = int(np.argmax(Cn))
    shm, shb = mid.sh.host().reshape(5, k), big.sh.host().reshape(5, k)
    for b in range(5):
        if b == worst:
            assert mid.sc.host()[b] == 0 and (shm[b] == SENT).all()
        else:
            assert np.array_equal(p[b, :c[b]], P[b, :c[b]]) and np.array_equal(shm[b], shb[b]) or lens[b] == 0
    # the rerun of the one that overflowed, with the count it reported
    p2, h2, c2 = launch(cuda, ids, offs[worst:worst + 2], k, seed, base, int(Cn[worst]), mid, ids=np.array([worst]))
    assert c2[0] == Cn[worst] and np.array_equal(p2[0], P[worst, :Cn[worst]]) and np.array_equal(h2[0], H[worst, :Cn[worst]])
    assert np.array_equal(mid.sh.host(), big.sh.host()) and np.array_equal(mid.sc.host(), big.sc.host())


@pytest.mark.parametrize("k", [33, 700, 4096])
def test_two_identical_launches_are_bit_equal(cuda, oracle, k):
    _, W = R.form_of(k)
    lens = [3 * W + 17, 0, 2 * k + 1, 100]
    offs = _offs(lens)
    ids = _ids(np.random.default_rng(k), int(offs[-1]))
    a, b = State(cuda, 4, k), State(cuda, 4, k)
    ra = launch(cuda, ids, offs, k, 1, 2, max(lens), a)
    rb = launch(cuda, ids, offs, k, 1, 2, max(lens), b)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    assert all(np.array_equal(x, y) for x, y in zip(a.snapshot(), b.snapshot()))


def test_thin_call_is_the_raw_launch(cuda, oracle):
    import torch

    from reservoir_amd import batch

    k, lens = 20, [500, 0, 77]
    offs = _offs(lens)
    ids = _ids(np.random.default_rng(4), int(offs[-1]))
    P, H, Cn = launch(cuda, ids, offs, k, 9, 4, 500, State(cuda, 3, k, bound=False))
    pos, hs, cnt = batch.distinct_segmented_candidates(torch.from_numpy(ids).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                                       9, stream_base=4, cap=500)
    cnt = cnt.cpu().numpy()
    assert np.array_equal(cnt, Cn)
    for b in range(3):
        assert np.array_equal(pos[b, :cnt[b]].cpu().numpy(), P[b, :cnt[b]])
        assert np.array_equal(hs[b, :cnt[b]].cpu().numpy(), H[b, :cnt[b]])
    # the default cap reads the offsets; an overflow is reported, not hidden
    _, _, c2 = batch.distinct_segmented_candidates(torch.from_numpy(ids).to(cuda), torch.from_numpy(offs).to(cuda), k, 9,
                                                   stream_base=4)
    assert np.array_equal(c2.cpu().numpy(), Cn)


# ---- batch.SegmentedObjectDistinct ----
def _elements(kind, rng, n):
    pool = rng.integers(0, 3 * n // 4 + 1, size=n)
    if kind == "str":
        return [f"user-{i}" for i in pool.tolist()]
    return [(int(i) % 13, f"t{i}") for i in pool.tolist()]


def _hash_fn(which):
    return hash if which == "python" else (lambda b: len(repr(b)) * 31 + (sum(map(ord, repr(b))) % 11))


def _reference(oracle, k, seed, elems, hashes):
    """The reference's set through the oracle: the elements as ids in order of first appearance."""
    table = {}
    ids = np.array([table.setdefault(e, len(table)) for e in elems], dtype=np.int64)
    rows, _ = _oracle_set(oracle, k, seed, ids, np.asarray(hashes, dtype=np.int64))
    back = {bytes(R.rows16([i])[0]): e for e, i in table.items()}
    return sorted(repr(back[r]) for r in rows)


@pytest.mark.parametrize("cap", [None, 4])
@pytest.mark.parametrize("which", ["python", "colliding"])
@pytest.mark.parametrize("kind", ["str", "tuple"])
def test_class_equals_one_handle_per_stream(cuda, oracle, kind, which, cap):
    """Strings and tuples under Python's hash and a colliding one, fed in two updates through permuted ids; a
    forced cap of 4 sends almost every segment through the rerun and changes nothing."""
    from reservoir_amd import Sampler, batch

    k, S, seed, base = 12, 5, 2**64 - 4, 3
    rng = np.random.default_rng(len(kind) + len(which))
    hf = _hash_fn(which)
    calls = [0]

    def mp(x):
        calls[0] += 1
        return x[1]

    streams = [_elements(kind, rng, n) for n in (300, 0, 45, 700, 11)]
    so = batch.SegmentedObjectDistinct(S, k, seed, stream_base=base, map_fn=mp, cap=cap, device=cuda)
    total = 0
    for t in range(2):
        order = rng.permutation(S)
        segs = [streams[i][len(streams[i]) * t // 2:len(streams[i]) * (t + 1) // 2] for i in order]
        elems = [("wrapped", e) for s in segs for e in s]
        total += len(elems)
        hashes = np.array([hf(e[1]) for e in elems], dtype=np.int64)
        so.update(elems, hashes, _offs([len(s) for s in segs]), stream_ids=order.astype(np.int64))
    info = so.info()
    assert calls[0] == info["candidates"] < total, "only candidates are mapped"
    assert info["launches"] >= 2 and (cap is None or (info["reruns"] > 0 and info["launches"] == 4))
    for r in range(S):
        d = Sampler.distinct(k, key_type="object", seed=_wrap(seed + base + r))(hash=hf)
        if streams[r]:
            d.sample_all(streams[r])
        assert so.result(r) == d.result(), (r, kind, which)
        assert sorted(map(repr, so.result(r))) == _reference(oracle, k, _wrap(seed + base + r), streams[r],
                                                             [hf(e) for e in streams[r]])
    assert so.results() == [so.result(r) for r in range(S)]


def test_a_throwing_map_drops_the_batch(cuda, oracle):
    from reservoir_amd import batch

    k, S = 6, 4
    rng = np.random.default_rng(5)
    poison = [False]

    def mp(x):
        if poison[0] and x.startswith("bad-"):
            raise KeyError(x)
        return x

    so = batch.SegmentedObjectDistinct(S, k, 21, map_fn=mp, device=cuda)
    twin = batch.SegmentedObjectDistinct(S, k, 21, device=cuda)
    # row 2 stays empty in the first batch, so in the second it is open: its elements are candidates for certain
    first = [[] if r == 2 else _elements("str", rng, 40) for r in range(S)]
    second = [[f"bad-{i}" for i in range(9)] if r == 2 else _elements("str", rng, 60) for r in range(S)]

    def feed(o, segs):
        elems = [e for s in segs for e in s]
        o.update(elems, np.array([hash(e) for e in elems], dtype=np.int64), _offs([len(s) for s in segs]))

    feed(so, first)
    feed(twin, first)
    state = [t.clone() for t in so._state()]
    def heaps_of(o):
        return {r: o.replica(r).heap() if o.replica(r) is not None else None for r in range(S)}

    heaps = heaps_of(so)
    assert heaps[2] is None
    info = so.info()
    poison[0] = True
    with pytest.raises(KeyError):
        feed(so, second)
    assert all(bool((a == b).all()) for a, b in zip(state, so._state())), "a state row changed"
    assert heaps == heaps_of(so) and so.info()["candidates"] == info["candidates"]
    poison[0] = False
    feed(so, second)  # the retry behaves as if the failed batch never came
    feed(twin, second)
    assert so.results() == twin.results()
    assert all(bool((a == b).all()) for a, b in zip(twin._state(), so._state()))
