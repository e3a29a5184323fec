"""Sampler.distinct for any B (key_type="object"): the hash-only candidate pass of rsv_objects.hip
through the raw C ABI (rsv_distinct_candidates / rsv_candidates_read / _commit / _abort) and through
the Python mirror (reservoir_amd.object_distinct), against the reference's RandomValues
(Sampler.scala:383-412) as the C oracle runs it.

Soundness: the candidates are a superset of the positions at which RandomValues, run over the whole
stream, admits an element; replaying only the candidates gives the oracle's set.  Tightness: the
candidate counts stay far below n (so "return everything" fails).  Edges: tiny batches, an 8-byte
aligned head, a constant hash, a crowded boundary hash (the strict <), a forced candidate-room
overflow.  The ABI's state machine, and the call sequence of ObjectDistinct.scala (C++ mirror).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GOLD = np.uint64(0x9E3779B97F4A7C15)
FILTER_TILE = 256 * 8 * 2  # elements one obj_filter workgroup covers per iteration


def _rows(ids, width):
    """width-byte key of element id (the splitmix stream of the id, little-endian words)."""
    ids = np.asarray(ids, dtype=np.uint64)
    out = np.empty((ids.size, width // 8), dtype=np.uint64)
    for w in range(width // 8):
        z = ids * np.uint64(0x9E3779B97F4A7C15) + np.uint64((w * 0x632BE59BD9B4E019 + 1) & M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        out[:, w] = z ^ (z >> np.uint64(31))
    return out.view(np.uint8).reshape(ids.size, width)


def _stream(n, seed):
    """element ids with ~30 % repeats, in random order"""
    rng = np.random.default_rng(seed)
    d = int(n * 0.7)
    ids = np.concatenate([np.arange(d), rng.integers(0, d, n - d)])
    rng.shuffle(ids)
    return ids


def _hashes(ids, kind):
    if kind == "random":   # a 64-bit hash: injective in practice
        return (_rows(ids, 8).view(np.int64).reshape(-1) ^ 0x5A5A).astype(np.int64)
    if kind == "collide":  # 97 hash values: fewer than k = 100 distinct hashes, crowded buckets
        return (np.asarray(ids, dtype=np.int64) % 97) - 48
    raise ValueError(kind)


def _byteswap64(v):
    return (v * GOLD).byteswap() * GOLD


def _scramble(r0, r1, hashes):
    """oracle.scramble over an int64 array (checked against the oracle in test_scramble_mirror)"""
    h = np.asarray(hashes, dtype=np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        return _byteswap64(np.uint64(r1 & M64) ^ _byteswap64(np.uint64(r0 & M64) ^ h)).view(np.int64)


def _r01(oracle, seed):
    d = oracle.Distinct(1, seed, oracle.HASH_IDENTITY)
    return d.r0, d.r1


def test_scramble_mirror(oracle):
    r0, r1 = _r01(oracle, 9)
    hs = _hashes(np.arange(200), "random")
    assert _scramble(r0, r1, hs).tolist() == [oracle.scramble(r0, r1, int(h)) for h in hs]


class Handle:
    """A raw index-only distinct handle."""

    def __init__(self, k, seed, hash_kind=None, kind=None):
        from reservoir_amd import _native as N

        self.N, self.L = N, N.load()
        cfg = N.RsvConfig()
        N.check(self.L.rsv_config_init(C.byref(cfg)))
        cfg.kind = N.KIND_DISTINCT if kind is None else kind
        cfg.max_sample_size = k
        cfg.hash_kind = N.HASH_PRECOMPUTED if hash_kind is None else hash_kind
        cfg.seed = seed
        self.h = C.c_void_p()
        N.check(self.L.rsv_create(C.byref(cfg), C.byref(self.h)))

    def __del__(self):
        if self.h:
            self.L.rsv_destroy(self.h)
            self.h = None

    def candidates_status(self, hashes):
        """rsv_distinct_candidates over a CUDA tensor or a numpy array -> (status, n_cand)"""
        nc = C.c_int64(-1)
        if isinstance(hashes, np.ndarray):
            ptr, mem = hashes.ctypes.data_as(C.c_void_p), self.N.MEM_HOST
        elif hashes is None:
            ptr, mem = None, self.N.MEM_DEVICE
        else:
            import torch

            torch.cuda.current_stream().synchronize()
            ptr, mem = C.c_void_p(hashes.data_ptr()), self.N.MEM_DEVICE
        n = 0 if hashes is None else len(hashes)
        return self.L.rsv_distinct_candidates(self.h, ptr, n, mem, C.byref(nc)), nc.value

    def candidates(self, hashes):
        st, c = self.candidates_status(hashes)
        self.N.check(st)
        offs = np.full(max(c, 1), -7, dtype=np.int64)
        hs = np.full(max(c, 1), -7, dtype=np.int64)
        self.N.check(self.L.rsv_candidates_read(self.h, offs.ctypes.data_as(C.c_void_p),
                                                hs.ctypes.data_as(C.c_void_p), c))
        return offs[:c], hs[:c]

    def commit(self, v):
        self.N.check(self.L.rsv_candidates_commit(self.h, v.size, v.max_hash))

    def abort(self):
        self.N.check(self.L.rsv_candidates_abort(self.h))

    @property
    def count(self):
        return int(self.L.rsv_count(self.h))


def _admissions(k, ids, sh):
    """RandomValues over the whole stream: the positions it admits, and the replica"""
    from reservoir_amd.values import RandomValues

    v = RandomValues(k)
    adm = []
    for i, (e, h) in enumerate(zip(ids.tolist(), sh.tolist())):
        if v.admits(e, h):
            adm.append(i)
            v.sample(e, h)
    return np.array(adm, dtype=np.int64), v


def _oracle_ids(oracle, k, seed, ids, hs):
    """the oracle's set over the 16-byte rows of the ids, as sorted row bytes"""
    ref = oracle.DistinctRows(k, seed, 16)
    ref.sample_all(_rows(ids, 16), hs)
    rows, _ = ref.result()
    return sorted(bytes(r) for r in rows)


def _ids_as_rows(ids):
    return sorted(bytes(r) for r in _rows(np.asarray(ids, dtype=np.int64), 16))


def _run(cuda, k, seed, ids, hs, cuts, sh, device=True):
    """The candidate protocol over the batches [cuts[i], cuts[i+1]): checks the offsets and hashes of
    every batch, replays the candidates; returns (global candidate positions, replica, per-batch counts).
    device: True (hs copied to the GPU), False (host batches) or the CUDA tensor that holds hs."""
    import torch

    from reservoir_amd.values import RandomValues

    hd = hs if device is False else torch.from_numpy(hs).to(cuda) if device is True else device
    H = Handle(k, seed)
    v = RandomValues(k)
    pos, counts = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        offs, ch = H.candidates(hd[a:b])
        assert np.all(np.diff(offs) > 0), "offsets strictly ascending"
        assert offs.size == 0 or (offs[0] >= 0 and offs[-1] < b - a)
        assert np.array_equal(ch, sh[a + offs]), "scrambled hashes"
        for e, h in zip(ids[a + offs].tolist(), ch.tolist()):
            v.sample(e, h)
        H.commit(v)
        assert H.count == b - cuts[0]
        pos.append(a + offs)
        counts.append(offs.size)
    return np.concatenate(pos) if pos else np.empty(0, np.int64), v, counts


@functools.lru_cache(maxsize=None)
def _case(hkind):
    n = 300_000
    ids = _stream(n, 17)
    return ids, _hashes(ids, hkind)


@functools.lru_cache(maxsize=None)
def _want(k, hkind):
    """shared references: the whole-stream admissions and the oracle's set (seed 9)"""
    from oracle import oracle as O

    ids, hs = _case(hkind)
    sh = _scramble(*_r01(O, 9), hs)
    adm, v = _admissions(k, ids, sh)
    return sh, adm, _oracle_ids(O, k, 9, ids, hs), v.max_hash


# ---- 1. candidate soundness through the raw ABI --------------------------------------------------
@pytest.mark.parametrize("cuts", [(0, 300_000), (0, 70_001, 70_004, 300_000)], ids=["one", "three"])
@pytest.mark.parametrize("hkind", ["random", "collide"])
@pytest.mark.parametrize("k", [1, 100, 4096])
def test_candidates_are_a_superset_and_replay_to_the_oracle(cuda, k, hkind, cuts):
    ids, hs = _case(hkind)
    sh, adm, want, max_hash = _want(k, hkind)
    pos, v, counts = _run(cuda, k, 9, ids, hs, cuts, sh)
    print(f"k={k} {hkind} cuts={cuts}: admissions {adm.size}, candidates {counts}")
    assert np.all(np.isin(adm, pos)), "an admission of the reference is no candidate"
    assert _ids_as_rows(v.result()) == want
    assert v.max_hash == max_hash


def test_host_hashes_give_the_same_candidates(cuda):
    ids, hs = _case("random")
    sh, adm, want, _ = _want(100, "random")
    cuts = (0, 70_001, 300_000)
    pd, vd, _ = _run(cuda, 100, 9, ids, hs, cuts, sh)
    ph, vh, _ = _run(cuda, 100, 9, ids, hs, cuts, sh, device=False)
    assert np.array_equal(pd, ph)
    assert _ids_as_rows(vh.result()) == want


# ---- 2. tightness ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [100, 4096])
def test_distinct_hashes_return_few_candidates(cuda, oracle, k):
    """all-distinct 64-bit hashes into an empty sampler, one batch: the reference admits about
    k (1 + ln(n / k)) of them (~1.2k and ~32k); the chunk loop stays within n / 8"""
    import torch

    n = 2**22 + 3
    hs = oracle.splitmix_keys(0xD15 + k, n)
    assert np.unique(hs).size == n
    H = Handle(k, 5)
    st, c = H.candidates_status(torch.from_numpy(hs).to(cuda))
    assert st == 0
    print(f"k={k}: n_cand {c} of {n}")
    assert 0 < c <= n // 8
    H.abort()


def test_callers_max_hash_bounds_a_colliding_hash(cuda):
    """97 hash values, k = 100: the engine's shadow never fills, the committed maxHash must take over"""
    ids, hs = _case("collide")
    sh, adm, want, _ = _want(100, "collide")
    cuts = (0, 100_000, 200_001, 300_000)
    pos, v, counts = _run(cuda, 100, 9, ids, hs, cuts, sh)
    print(f"collide-97 k=100: candidates per batch {counts}")
    assert counts[1] + counts[2] <= (300_000 - 100_000) // 16
    assert np.all(np.isin(adm, pos))
    assert _ids_as_rows(v.result()) == want


def test_python_maps_only_the_candidates(cuda):
    import torch

    from reservoir_amd import Sampler

    ids, hs = _case("random")
    calls = []

    def m(x):
        calls.append(x)
        return f"B{x}"

    d = Sampler.distinct(100, key_type="object", seed=9)(m, hash=lambda b: 0)
    d.sample_all(ids.tolist(), hashes=torch.from_numpy(hs).to(cuda))
    c = d.distinct_info()["candidates"]
    assert len(calls) == c and 100 <= c <= ids.size // 8
    _, _, want, _ = _want(100, "random")
    assert _ids_as_rows([int(b[1:]) for b in d.result()]) == want


# ---- 3. edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 4096])
def test_tiny_and_tile_sized_batches(cuda, oracle, k):
    """n in {0, 1, 2, 3, 255, 256, 257} and one filter tile +- 1; each stream also one element into
    its tensor (a hash pointer that is only 8-byte aligned), in one batch and in three"""
    r01 = _r01(oracle, 3)
    for n in (0, 1, 2, 3, 255, 256, 257, FILTER_TILE - 1, FILTER_TILE, FILTER_TILE + 1):
        ids = np.random.default_rng(n + k).integers(0, max(1, n * 7 // 10), n + 1)
        hs = _hashes(ids, "random") if n % 2 else (_hashes(ids, "random") % 50)
        sh = _scramble(*r01, hs)
        for lo in (0, 1):
            cuts = (lo, lo + n) if n < 4 or lo == 0 else (lo, lo + n // 3, lo + n // 3 + 1, lo + n)
            pos, v, _ = _run(cuda, k, 3, ids, hs, cuts, sh)
            adm, _ = _admissions(k, ids[lo:lo + n], sh[lo:lo + n])
            assert np.all(np.isin(adm + lo, pos)), (n, lo)
            assert _ids_as_rows(v.result()) == _oracle_ids(oracle, k, 3, ids[lo:lo + n], hs[lo:lo + n]), (n, lo)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned16", "plus8"])
@pytest.mark.parametrize("bounded", [False, True], ids=["open", "bounded"])
def test_filter_alignment_edges(cuda, oracle, bounded, shift):
    """obj_filter at the edges of its 16-byte loads: batches of n = 1, 2, 3, 17 and 4099 hashes (4096 =
    one workgroup's full tile, plus the head before the first 16-byte boundary and the odd tail) that
    start on a 16-byte boundary or 8 bytes past one, into an empty handle (everything is a candidate) and
    behind a committed batch of 2048 (+ 1) elements (k = 3: the filter runs with a bound).  The batch's
    first and last element are fresh and hashed below everything before them, so the reference admits
    both."""
    import torch
    from hash_targets import MIN, plant

    k, seed, pre = 3, 3, 2048
    r01 = _r01(oracle, seed)
    for n in (1, 2, 3, 17, 4099):
        a = pre + shift if bounded else shift
        ids = np.random.default_rng(n).integers(0, (a + n) * 7 // 10 + 1, a + n)
        hs = _hashes(ids, "random")
        for e, i in enumerate(sorted({a, a + n - 1})):
            ids[i] = a + n + e
            hs[i] = plant(*r01, [MIN + 10 - e])[0]
        sh = _scramble(*r01, hs)
        hd = torch.from_numpy(hs).to(cuda)
        assert hd.data_ptr() % 16 == 0 and hd[a:].data_ptr() % 16 == 8 * shift
        lo = 0 if bounded else a
        pos, v, counts = _run(cuda, k, seed, ids, hs, (lo, a, a + n) if bounded else (a, a + n), sh, device=hd)
        adm, _ = _admissions(k, ids[lo:], sh[lo:])
        assert a - lo in adm and a + n - 1 - lo in adm  # the planted head and tail
        assert np.all(np.isin(adm + lo, pos)), (n, "an admission of the reference is no candidate")
        assert _ids_as_rows(v.result()) == _oracle_ids(oracle, k, seed, ids[lo:], hs[lo:]), n
        assert not bounded or n <= 3 or counts[1] < n, counts  # a bound was in force


def test_empty_batch_is_valid(cuda):
    from reservoir_amd.values import RandomValues

    H = Handle(5, 1)
    st, c = H.candidates_status(None)  # NULL hashes with n == 0
    assert (st, c) == (0, 0)
    assert H.L.rsv_candidates_read(H.h, None, None, 0) == 0
    H.commit(RandomValues(5))
    assert H.count == 0


def test_constant_hash_returns_everything(cuda, oracle):
    """one hash value: every element is a candidate until the caller's set is full; the result is the
    oracle's k first distinct elements"""
    k, n = 50, 5000
    ids = _stream(n, 4)
    hs = np.full(n, 1234, dtype=np.int64)
    sh = _scramble(*_r01(oracle, 2), hs)
    pos, v, counts = _run(cuda, k, 2, ids, hs, (0, 3000, n), sh)
    assert counts[0] == 3000 and counts[1] == 0  # full set, maxHash = the one hash: nothing is below it
    first = list(dict.fromkeys(ids.tolist()))[:k]
    assert sorted(v.result()) == sorted(first)
    assert _ids_as_rows(v.result()) == _oracle_ids(oracle, k, 2, ids, hs)


def test_crowded_boundary_hash_is_not_a_candidate(cuda, oracle):
    """k = 100 distinct hash values fill the shadow; hundreds of further distinct elements carry
    exactly its largest value T: the reference admits h < maxHash <= T only, and so does the filter"""
    k = 100
    r01 = _r01(oracle, 6)
    raw = oracle.splitmix_keys(99, 4000)
    order = np.argsort(_scramble(*r01, raw))
    low, b, high = raw[order[:k - 1]], raw[order[k - 1]], raw[order[k:]]
    hs1 = np.concatenate([low, np.full(300, b)])            # 99 lower values, then the boundary bucket
    hs2 = np.concatenate([np.full(500, b), high[:1500]])    # more of the bucket, and larger hashes
    rng = np.random.default_rng(1)
    rng.shuffle(hs2)
    hs = np.concatenate([hs1, hs2]).astype(np.int64)
    ids = np.arange(hs.size)                                # all distinct elements
    sh = _scramble(*r01, hs)
    pos, v, counts = _run(cuda, k, 6, ids, hs, (0, hs1.size, hs.size), sh)
    assert counts == [hs1.size, 0]
    assert _ids_as_rows(v.result()) == _oracle_ids(oracle, k, 6, ids, hs)
    assert sorted(v.result()) == list(range(k))


def test_candidate_room_overflow_changes_nothing(cuda, monkeypatch):
    """RSV_OBJ_ROOM shrinks the first batch's candidate room: the dropped candidates are counted, the
    room regrown and the batch rerun"""
    ids, hs = _case("random")
    sh, adm, want, _ = _want(100, "random")
    cuts = (0, 150_000, 300_000)
    pos, v, counts = _run(cuda, 100, 9, ids, hs, cuts, sh)
    monkeypatch.setenv("RSV_OBJ_ROOM", "64")
    pos2, v2, counts2 = _run(cuda, 100, 9, ids, hs, cuts, sh)
    assert counts[0] > 64
    assert np.array_equal(pos, pos2) and counts == counts2
    assert _ids_as_rows(v2.result()) == want


# ---- 4. Python forms -------------------------------------------------------------------------------
def _collide_hash(b):
    return int(b[1:]) % 1000 - 500


@pytest.mark.parametrize("hname", ["builtin", "collide"])
@pytest.mark.parametrize("k", [1, 100, 5000])
def test_python_forms_equal_the_oracle(cuda, oracle, k, hname):
    import torch

    from reservoir_amd import Sampler

    n = 60_000
    ids = _stream(n, k)
    B = [f"B{i}" for i in ids.tolist()]
    hf = hash if hname == "builtin" else _collide_hash
    hs = np.array([hf(b) for b in B], dtype=np.int64)
    want = _oracle_ids(oracle, k, 21, ids, hs)
    hd = torch.from_numpy(hs).to(cuda)

    def make():
        kw = {} if hname == "builtin" else {"hash": hf}
        return Sampler.distinct(k, key_type="object", seed=21)(lambda i: f"B{i}", **kw)

    def check(d):
        assert d.count == n
        got = d.result()
        assert len(got) == len(set(got)) == len(want)
        assert _ids_as_rows([int(b[1:]) for b in got]) == want

    d = make()  # sample() per element
    for i in ids[:20_000].tolist():
        d.sample(i)
    assert d.count == 20_000
    d.sample_all(ids[20_000:].tolist())
    check(d)
    d = make()  # one list
    d.sample_all(ids.tolist())
    check(d)
    d = make()  # hashes= numpy
    d.sample_all(ids.tolist(), hashes=hs)
    check(d)
    d = make()  # hashes= CUDA tensor
    d.sample_all(ids.tolist(), hashes=hd)
    check(d)
    d = make()  # mixed and split
    d.sample_all(ids[:7].tolist(), hashes=hd[:7])
    for i in ids[7:1000].tolist():
        d.sample(i)
    d.sample_all(ids[1000:30_001].tolist(), hashes=hs[1000:30_001])
    d.sample_all(iter(ids[30_001:40_000].tolist()))
    d.sample_all(ids[40_000:], hashes=hd[40_000:])
    check(d)


def test_reusable_repeats_and_single_use_closes(cuda, oracle):
    from reservoir_amd import IllegalStateException, Sampler

    ids = _stream(20_000, 3)
    hs = np.array([_collide_hash(f"B{i}") for i in ids.tolist()], dtype=np.int64)
    d = Sampler.distinct(100, reusable=True, key_type="object", seed=8)(lambda i: f"B{i}", hash=_collide_hash)
    d.sample_all(ids[:9000].tolist())
    r1 = d.result()
    r1_copy = list(r1)
    assert d.is_open and d.result() == r1
    assert _ids_as_rows([int(b[1:]) for b in r1]) == _oracle_ids(oracle, 100, 8, ids[:9000], hs[:9000])
    d.sample_all(ids[9000:].tolist())
    r2 = d.result()
    assert r1 == r1_copy, "a later batch must not clobber an earlier result"
    assert _ids_as_rows([int(b[1:]) for b in r2]) == _oracle_ids(oracle, 100, 8, ids, hs)
    assert d.count == ids.size and d.distinct_info()["size"] == 100

    s = Sampler.distinct(100, key_type="object", seed=8)(lambda i: f"B{i}", hash=_collide_hash)
    s.sample_all(ids.tolist())
    assert s.result() == r2
    assert not s.is_open and s.count == ids.size
    for call in (lambda: s.sample(1), lambda: s.sample_all([1]), s.result):
        with pytest.raises(IllegalStateException):
            call()


def test_throwing_map_drops_the_batch(cuda):
    from reservoir_amd import Sampler

    ids = _stream(30_000, 5)
    hs = _hashes(ids, "random")
    bad = {"on": False}

    def m(i):
        if bad["on"] and i % 3 == 0:
            raise KeyError(i)
        return f"B{i}"

    def make():
        return Sampler.distinct(100, reusable=True, key_type="object", seed=2)(m, hash=lambda b: 0)

    d, clean = make(), make()
    for s in (d, clean):
        s.sample_all(ids[:10_000].tolist(), hashes=hs[:10_000])
    before = d.result()
    bad["on"] = True
    with pytest.raises(KeyError):
        d.sample_all(ids[10_000:20_000].tolist(), hashes=hs[10_000:20_000])
    bad["on"] = False
    assert d.is_open and d.count == 10_000 and d.result() == before
    for s in (d, clean):
        s.sample_all(ids[20_000:].tolist(), hashes=hs[20_000:])
    assert d.count == clean.count == 20_000
    assert d.result() == clean.result()
    assert d.distinct_info() == clean.distinct_info()


# ---- 5. the ABI's state machine ----------------------------------------------------------------------
def test_abi_status_codes(cuda):
    import torch

    from reservoir_amd import _native as N

    L = N.load()
    hs = _hashes(np.arange(5000), "random")
    hd = torch.from_numpy(hs).to(cuda)
    nc = C.c_int64(0)
    buf = np.zeros(5000, dtype=np.int64)
    p = buf.ctypes.data_as(C.c_void_p)

    # another hash kind / another sampler kind
    assert Handle(10, 1, hash_kind=N.HASH_JAVA_LONG).candidates_status(hd)[0] == N.E_UNSUPPORTED
    assert Handle(10, 1, hash_kind=N.HASH_IDENTITY).candidates_status(hd)[0] == N.E_UNSUPPORTED
    assert Handle(10, 1, kind=N.KIND_ELEMENTS).candidates_status(hd)[0] == N.E_UNSUPPORTED
    # arguments
    H = Handle(10, 1)
    assert L.rsv_distinct_candidates(H.h, None, 5, N.MEM_DEVICE, C.byref(nc)) == N.E_NULL_POINTER
    assert L.rsv_distinct_candidates(H.h, C.c_void_p(hd.data_ptr()), -1, N.MEM_DEVICE, C.byref(nc)) == N.E_ILLEGAL_ARGUMENT
    assert L.rsv_distinct_candidates(H.h, C.c_void_p(hd.data_ptr()), 5, 7, C.byref(nc)) == N.E_ILLEGAL_ARGUMENT
    assert L.rsv_distinct_candidates(H.h, C.c_void_p(hd.data_ptr()), 5, N.MEM_DEVICE, None) == N.E_NULL_POINTER
    assert L.rsv_distinct_candidates(None, C.c_void_p(hd.data_ptr()), 5, N.MEM_DEVICE, C.byref(nc)) == N.E_NULL_POINTER
    # nothing pending
    assert L.rsv_candidates_read(H.h, p, p, 5000) == N.E_ILLEGAL_STATE
    assert L.rsv_candidates_commit(H.h, 0, 0) == N.E_ILLEGAL_STATE
    assert L.rsv_candidates_abort(H.h) == N.E_ILLEGAL_STATE
    # a handle that holds keys
    K = Handle(10, 1)
    assert L.rsv_sample_batch(K.h, C.c_void_p(hd.data_ptr()), 100, N.MEM_DEVICE, C.c_void_p(hd.data_ptr())) == 0
    assert K.candidates_status(hd)[0] == N.E_ILLEGAL_STATE
    # a pending batch: only read, commit, abort, is_open, count (and destroy)
    st, c = H.candidates_status(hd)
    assert st == 0 and c > 0
    assert L.rsv_is_open(H.h) == 1 and H.count == 0
    info = N.RsvDistinctInfo()
    info.struct_size = C.sizeof(N.RsvDistinctInfo)
    ms = C.c_double()
    pending_calls = [
        lambda: H.candidates_status(hd)[0],
        lambda: L.rsv_sample(H.h, p, p),
        lambda: L.rsv_sample_batch(H.h, C.c_void_p(hd.data_ptr()), 5, N.MEM_DEVICE, C.c_void_p(hd.data_ptr())),
        lambda: L.rsv_stage_commit(H.h, 0),
        lambda: L.rsv_result(H.h, p, 5000, C.byref(nc)),
        lambda: L.rsv_result_device(H.h, C.c_void_p(hd.data_ptr()), 5000, C.byref(nc)),
        lambda: L.rsv_get_distinct_info(H.h, C.byref(info)),
        lambda: L.rsv_export_packed(H.h, C.c_void_p(hd.data_ptr())),
        lambda: L.rsv_export_log(H.h, 0, None, None, 0, C.byref(nc)),
        lambda: L.rsv_synchronize(H.h),
        lambda: L.rsv_set_stream(H.h, None),
        lambda: L.rsv_profile_enable(H.h, 1),
        lambda: L.rsv_profile_read(H.h, C.byref(ms), C.byref(nc)),
        lambda: L.rsv_seek(H.h, 10),
    ]
    for i, call in enumerate(pending_calls):
        assert call() == N.E_ILLEGAL_STATE, i
    assert L.rsv_candidates_read(H.h, p, p, c - 1) == N.E_ILLEGAL_ARGUMENT
    assert L.rsv_candidates_read(H.h, None, p, c) == N.E_NULL_POINTER
    assert L.rsv_candidates_read(H.h, p, p, c) == 0
    assert L.rsv_candidates_commit(H.h, -1, 0) == N.E_ILLEGAL_ARGUMENT
    assert L.rsv_candidates_commit(H.h, 11, 0) == N.E_ILLEGAL_ARGUMENT
    assert L.rsv_candidates_commit(H.h, 10, 2**62) == 0
    assert H.count == 5000
    # index-only from now on: keyed calls, results, exports and merges are refused
    keyed_calls = pending_calls[1:9] + [
        lambda: L.rsv_merge_packed(H.h, C.c_void_p(hd.data_ptr()), 1, 5000, 5000),
        lambda: L.rsv_export_state(H.h, None, None, None, C.byref(nc)),
        lambda: L.rsv_merge_state(H.h, None, None, None, None, 0, 0, 0),
        lambda: L.rsv_merge_log(H.h, None, None, 0, 0),
    ]
    for i, call in enumerate(keyed_calls):
        assert call() == N.E_ILLEGAL_STATE, i
    assert L.rsv_synchronize(H.h) == 0
    assert L.rsv_is_open(H.h) == 1


def test_abort_leaves_no_trace(cuda, oracle):
    import torch

    ids, hs = _case("random")
    sh, _, _, _ = _want(100, "random")
    hd = torch.from_numpy(hs).to(cuda)
    cuts = (0, 50_000, 120_000)
    pos, v, counts = _run(cuda, 100, 9, ids, hs, cuts, sh)

    from reservoir_amd.values import RandomValues

    H = Handle(100, 9)
    st, c = H.candidates_status(hd[200_000:])  # dropped before anything was committed
    assert st == 0 and c > 0
    H.abort()
    assert H.count == 0
    w = RandomValues(100)
    offs, ch = H.candidates(hd[:50_000])
    for e, h in zip(ids[offs].tolist(), ch.tolist()):
        w.sample(e, h)
    H.commit(w)
    assert H.count == 50_000
    st, c = H.candidates_status(hd[200_000:])  # small hashes in here would tighten a leaked shadow
    assert st == 0
    H.abort()
    assert H.count == 50_000
    offs2, ch2 = H.candidates(hd[50_000:120_000])
    H.abort()
    offs3, ch3 = H.candidates(hd[50_000:120_000])
    assert np.array_equal(offs2, offs3) and np.array_equal(ch2, ch3)
    assert np.array_equal(np.concatenate([offs, 50_000 + offs3]), pos)


def test_profile_brackets_the_filter(cuda):
    import torch

    hs = _hashes(np.arange(100_000), "random")
    H = Handle(100, 1)
    assert H.L.rsv_profile_enable(H.h, 1) == 0
    st, c = H.candidates_status(torch.from_numpy(hs).to(cuda))
    assert st == 0
    H.abort()
    ms, launches = C.c_double(), C.c_int64()
    assert H.L.rsv_profile_read(H.h, C.byref(ms), C.byref(launches)) == 0
    assert launches.value >= 2 and ms.value > 0  # the fill chunk, then the rest


# ---- 6. ObjectDistinct.scala's call sequence (C++ mirror) ------------------------------------------
def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def test_cpp_object_distinct_mirror(tmp_path, cuda, oracle):
    """n = 2^24 hash twins with 30 % repeats in host batches of 2^20, k = 65536, hash = Long.hashCode:
    the mirror's set equals the oracle's.  The ids follow tests/cpp/test_object_distinct.cpp's formula."""
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "reservoir_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_object_distinct.cpp"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "reservoir_amd"), "-lreservoir_hip",
                    f"-Wl,-rpath,{os.path.join(ROOT, 'reservoir_amd')}"], check=True)
    n, k, seed, bits = 2**24, 65536, 13, 22
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        rep = (_mix(i ^ np.uint64(0xABCD)) % np.uint64(10) < np.uint64(3)) & (i > 0)
        src = np.where(rep, _mix(i + np.uint64(77)) % np.maximum(i, np.uint64(1)), i)
        v = _mix(src * GOLD + np.uint64(seed))
        hi = v >> np.uint64(32)
        ids = ((hi << np.uint64(32)) | ((hi ^ (v & np.uint64((1 << bits) - 1))) & np.uint64(0xFFFFFFFF))).view(np.int64)
    ref = oracle.Distinct(k, seed, oracle.HASH_JAVA_LONG)
    ref.sample_all(ids)
    want, _ = ref.result()
    f = tmp_path / "case.txt"
    f.write_text(f"{n} {k} {seed} {bits} {1 << 20}\n" + " ".join(str(int(x)) for x in np.sort(want)) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
