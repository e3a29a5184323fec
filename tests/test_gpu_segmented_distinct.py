"""Segmented Sampler.distinct (K5, rsv_distinct_segmented): S independent distinct samplers per launch.

Stream s is seeded with java.util.Random(seed + stream_base + s) and holds the min(k, D_s) distinct
keys with the smallest (scrambled hash, key), ascending.  Every comparison is exact (keys, hashes,
counts, zeros beyond the count) against a value computed here with numpy:

    h = byteswap64(r1 ^ byteswap64(r0 ^ hash(u)))   for u = the stream's distinct keys
    order = lexsort((u, h))[:k]

with (r0, r1) from oracle.Distinct(k, seed_s).r0/.r1, and for the identity hash also against the
oracle's RandomValues restatement per stream.  Forms: one wave per stream up to k = 256, a 256-thread
workgroup up to k = 1024, a 1024-thread workgroup up to k = 4096.
"""
import ctypes as C

import numpy as np
import pytest
from segdistinct_ref import WAVE_MAX_K, _expected, _hash_np, _r01, _scramble, _with_repeats

pytestmark = pytest.mark.gpu


def _run(cuda, keys, offs, k, seed, stream_base=0, **kw):
    import torch

    from reservoir_amd import batch

    if "hashes" in kw:
        kw["hashes"] = torch.from_numpy(kw["hashes"]).to(cuda)
    ok, oh, cnt = batch.distinct_segmented(torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                           seed=seed, stream_base=stream_base, **kw)
    return ok.cpu().numpy(), oh.cpu().numpy(), cnt.cpu().numpy()


def _check(got, want):
    gk, gh, gc = got
    wk, wh, wc = want
    assert np.array_equal(gc, wc)
    assert np.array_equal(gh, wh)
    assert np.array_equal(gk.astype(np.int64), wk)  # slots beyond the count are 0 on both sides


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, WAVE_MAX_K, WAVE_MAX_K + 1, 1000, 1024, 1025, 4096])
def test_ragged_parity(cuda, oracle, k):
    rng = np.random.default_rng(k)
    big = k >= 1000
    lens = rng.integers(0, 4 * k + 5000 if big else 5000, size=60 if big else 300)
    lens[:6] = [0, 1, k - 1, k, k + 1, 4096]
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = _with_repeats(rng, oracle.splitmix_keys(k, int(offs[-1])), offs)
    seed, base = 77, 1000
    r0, r1 = _r01(oracle, k, seed, base, lens.size)
    want = _expected(keys, keys, offs, k, r0, r1)
    got = _run(cuda, keys, offs, k, seed, base, hash="identity")
    _check(got, want)
    for s in range(lens.size):  # the oracle's RandomValues per stream (injective hash: the same set)
        ref = oracle.Distinct(k, seed + base + s, oracle.HASH_IDENTITY)
        ref.sample_all(keys[offs[s]:offs[s + 1]])
        rk, rh = ref.result()
        m = int(got[2][s])
        assert m == rk.size, s
        assert np.array_equal(got[0][s, :m], rk) and np.array_equal(got[1][s, :m], rh), s


@pytest.mark.parametrize("k", [5, 64, 512])
@pytest.mark.parametrize("mode", ["java_long", "precomputed"])
def test_colliding_hashes(cuda, oracle, k, mode):
    """Long.hashCode folded to 300 values; precomputed key % 37 (fewer hash values than k = 64: every
    admission is a tie on h, decided by the key)."""
    rng = np.random.default_rng(k * 7 + len(mode))
    lens = rng.integers(0, 3000, size=100)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    x = _with_repeats(rng, oracle.splitmix_keys(k + 9, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 4, 50, lens.size)
    if mode == "java_long":
        keys = ((x >> 32) << 32) | (((x >> 32) ^ (x % 300)) & 0xFFFFFFFF)
        hashed = _hash_np(keys, "java_long")
        assert np.unique(hashed).size <= 300
        got = _run(cuda, keys, offs, k, 4, 50, hash="java_long")
    else:
        keys = x
        hashed = keys % 37
        got = _run(cuda, keys, offs, k, 4, 50, hashes=hashed)
    _check(got, _expected(keys, hashed, offs, k, r0, r1))


@pytest.mark.parametrize("k", [17, 600])
@pytest.mark.parametrize("hash", ["java_int", "default"])
def test_int32_keys(cuda, oracle, k, hash):
    rng = np.random.default_rng(k)
    lens = rng.integers(0, 3000, size=100)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n = int(offs[-1])
    keys = np.where(rng.random(n) < 0.5, rng.integers(-2**31, 2**31, size=n), rng.integers(-700, 700, size=n))
    keys = keys.astype(np.int32)
    assert (keys < 0).any()
    r0, r1 = _r01(oracle, k, 9, 0, lens.size)
    got = _run(cuda, keys, offs, k, 9, hash=hash)
    assert got[0].dtype == np.int32
    _check(got, _expected(keys, _hash_np(keys, "java_int"), offs, k, r0, r1))


@pytest.mark.parametrize("k", [64, 1024])
def test_worst_case_arrival(cuda, oracle, k):
    """Descending (h, key) under the stream's own (r0, r1): every element is admitted; ascending:
    nothing after the first k; all-equal keys: one member, repeated."""
    S, n = 8, 20_000
    offs = np.arange(0, S * n + 1, n, dtype=np.int64)
    keys = oracle.splitmix_keys(k + 1, S * n)
    assert np.unique(keys).size == keys.size
    r0, r1 = _r01(oracle, k, 21, 5, S)
    sid = np.repeat(np.arange(S), n)
    asc = keys[np.lexsort((keys, _scramble(r0[sid], r1[sid], keys), sid))]
    desc = asc.reshape(S, n)[:, ::-1].reshape(-1).copy()
    want = _expected(asc, asc, offs, k, r0, r1)
    assert np.array_equal(want[0], asc.reshape(S, n)[:, :k])
    _check(_run(cuda, desc, offs, k, 21, 5, hash="identity"), want)
    _check(_run(cuda, asc, offs, k, 21, 5, hash="identity"), want)
    same = np.repeat(keys[:S], n)
    got = _run(cuda, same, offs, k, 21, 5, hash="identity")
    assert np.array_equal(got[2], np.ones(S, dtype=np.int64))
    _check(got, _expected(same, same, offs, k, r0, r1))


def test_offsets_start_past_zero(cuda, oracle):
    """offsets[0] = 3: 8-byte keys start off a 16-byte boundary; the keys before it are not read."""
    rng = np.random.default_rng(3)
    for k in (8, 300):
        lens = rng.integers(0, 2000, size=40)
        offs = (3 + np.r_[0, np.cumsum(lens)]).astype(np.int64)
        keys = oracle.splitmix_keys(31, int(offs[-1]))
        keys[3:] = _with_repeats(rng, keys[3:].copy(), offs - 3)
        r0, r1 = _r01(oracle, k, 1, 0, lens.size)
        _check(_run(cuda, keys, offs, k, 1, hash="identity"), _expected(keys, keys, offs, k, r0, r1))


@pytest.mark.parametrize("S", [1, 2, 100_003])
def test_short_streams_and_grid_stride(cuda, oracle, S):
    rng = np.random.default_rng(S)
    lens = rng.integers(0, 41, size=S)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = rng.integers(-60, 60, size=int(offs[-1])).astype(np.int64) * 0x9E3779B97F4A7
    r0, r1 = _r01(oracle, 8, 12, 2**63 - 50_000, S)  # the seed wraps past INT64_MAX inside the launch
    _check(_run(cuda, keys, offs, 8, 12, 2**63 - 50_000, hash="identity"), _expected(keys, keys, offs, 8, r0, r1))


def test_all_empty_launch(cuda):
    for k in (8, 2000):
        gk, gh, gc = _run(cuda, np.zeros(0, dtype=np.int64), np.zeros(51, dtype=np.int64), k, 1, hash="identity")
        assert gk.shape == (50, k) and not gk.any() and not gh.any() and not gc.any()
    gk, gh, gc = _run(cuda, np.zeros(0, dtype=np.int64), np.zeros(4, dtype=np.int64), 8, 1,
                      hashes=np.zeros(0, dtype=np.int64))
    assert not gk.any() and not gh.any() and not gc.any()


def test_torch_stream_repeat_and_null_hashes(cuda, oracle):
    """A non-default torch stream; two runs bit-identical; out_hashes_dev = NULL through ctypes."""
    import torch

    from reservoir_amd import _native as N
    from reservoir_amd import batch

    rng = np.random.default_rng(8)
    k, S = 100, 200
    lens = rng.integers(0, 3000, size=S)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = _with_repeats(rng, oracle.splitmix_keys(2, int(offs[-1])), offs)
    r0, r1 = _r01(oracle, k, 6, 0, S)
    want = _expected(keys, keys, offs, k, r0, r1)
    kd, od = torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        a = batch.distinct_segmented(kd, od, k, seed=6, hash="identity")
        b = batch.distinct_segmented(kd, od, k, seed=6, hash="identity")
    st.synchronize()
    _check([t.cpu().numpy() for t in a], want)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    out = torch.full((S, k), -1, dtype=torch.int64, device=cuda)
    cnt = torch.full((S,), -1, dtype=torch.int64, device=cuda)
    torch.cuda.synchronize()
    N.check(N.load().rsv_distinct_segmented(
        C.c_void_p(kd.data_ptr()), None, C.c_void_p(od.data_ptr()), S, 8, k, N.HASH_IDENTITY, 6, 0,
        C.c_void_p(out.data_ptr()), None, C.c_void_p(cnt.data_ptr()),
        C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(cnt.cpu().numpy(), want[2])


def test_bad_arguments_raise(cuda):
    import torch

    from reservoir_amd import IllegalArgumentException, ReservoirError, batch

    keys = torch.arange(10, dtype=torch.int64, device=cuda)
    offs = torch.tensor([0, 10], dtype=torch.int64, device=cuda)
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented(keys, offs, 0, seed=1)
    with pytest.raises(ReservoirError, match="4096"):
        batch.distinct_segmented(keys, offs, 4097, seed=1)
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented(keys, offs, 4, seed=1, hash="md5")
    with pytest.raises(IllegalArgumentException):
        batch.distinct_segmented(keys.cpu(), offs, 4, seed=1)


@pytest.mark.parametrize("k", [10, 700])
def test_reference_properties(cuda, oracle, k):
    """Without the oracle: the result does not depend on the arrival order; stream s of a launch is
    stream 0 of a launch of its segment alone with stream_base + s; and it is what a single
    Sampler.distinct(k, seed=seed_s, order="set") handle holds after the same keys."""
    import torch

    from reservoir_amd import Sampler

    rng = np.random.default_rng(k)
    S = 6
    lens = rng.integers(0, 6000, size=S)
    lens[1] = k // 2
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    keys = _with_repeats(rng, oracle.splitmix_keys(k, int(offs[-1])), offs)
    got = _run(cuda, keys, offs, k, 40, 7, hash="identity")
    perm = keys.copy()
    for s in range(S):
        rng.shuffle(perm[offs[s]:offs[s + 1]])
    _check(_run(cuda, perm, offs, k, 40, 7, hash="identity"), got)
    for s in range(S):
        seg = keys[offs[s]:offs[s + 1]]
        solo = _run(cuda, seg, np.array([0, seg.size], dtype=np.int64), k, 40, 7 + s, hash="identity")
        _check(solo, (got[0][s:s + 1], got[1][s:s + 1], got[2][s:s + 1]))
        d = Sampler.distinct(k, seed=40 + 7 + s, order="set")(hash="identity")
        if seg.size:
            d.sample_all(torch.from_numpy(seg).to(cuda))
        assert np.array_equal(d.result(), got[0][s, :got[2][s]]), s
