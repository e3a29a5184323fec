"""64-bit draw parameters through every K1 and K2 entry.

DrawKey{s0, s1, k0, k1} = (stream lo, stream hi, seed lo, seed hi) feeds the hand-specialised Philox
bodies of rsv_device.h (philox4x32_10, _uniform_hi, _uniform_hi_x2, _uniform_hi_x2_at) and
level1_b0_words (rsv_scan.h).  A default sampler draws its seed from 64 bits of entropy, yet every
other GPU test uses seeds below 2^32 and small stream ids, so k1 = seed >> 32 and (for K1)
s1 = stream >> 32 are zero there.  Here all four words are nonzero, all ones, or the masked image of
a negative Python int, and every entry that reaches K1 or K2 is compared with the CPU oracle -- whose
own dependence on the high words tests/test_oracle_fast.py pins.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1
SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03  # all four 32-bit words nonzero and distinct
# (seed, stream_id) as the caller passes them; the last pair is masked by the Python layer
PARAMS = [(SEED, SID), (2**64 - 1, 2**64 - 1), (-1, -2**63)]
PARAM_IDS = ["golden_ratio", "all_ones", "negative_masked"]
N = 300_000


@functools.lru_cache(maxsize=None)
def _keys(kt):
    from oracle import oracle

    keys = oracle.splitmix_keys(0xD8A3, N)
    return keys if kt == "long" else keys.astype(np.int32)  # wraps: negative Int keys too


@functools.lru_cache(maxsize=None)
def _want(seed, sid, k, kt):
    """The oracle's reservoir over _keys(kt) -- one per (parameters, k, key type), shared by the entries."""
    from oracle import oracle

    want, _ = oracle.algo_r(seed & M64, sid & M64, k, _keys(kt).astype(np.int64))
    return want.astype(_keys(kt).dtype)


def _stage_all(L, Nat, h, keys, step):
    """rsv_stage_acquire / rsv_stage_commit over `keys`, `step` keys at most per commit."""
    i, n = 0, keys.size
    while i < n:
        buf, cap = C.c_void_p(), C.c_int64()
        Nat.check(L.rsv_stage_acquire(h, C.byref(buf), None, C.byref(cap)))
        assert cap.value > 0
        c = min(cap.value, n - i, step)
        C.memmove(buf.value, keys[i:i + c].ctypes.data, c * keys.dtype.itemsize)
        Nat.check(L.rsv_stage_commit(h, c))
        i += c


@pytest.mark.parametrize("k", [1, 64, 1000, 2048, 2049, 9000])
@pytest.mark.parametrize("kt", ["long", "int"])
@pytest.mark.parametrize("seed,sid", PARAMS, ids=PARAM_IDS)
def test_k1_entries_with_64bit_parameters(cuda, oracle, seed, sid, kt, k):
    """Every way keys reach K1 -- device batches (fused k1_resolve_publish up to k = 2048, the
    two-kernel forms at 2049 and 9000), indexed host batches (rsv_sample_indexed: numpy arrays and a
    Range), copied host batches, per-element sample(), zero-copy staging -- with the same 64-bit key."""
    import torch

    from reservoir_amd import Sampler, _native as Nat

    keys = _keys(kt)
    want = _want(seed, sid, k, kt)
    make = lambda: Sampler(k, seed=seed, stream_id=sid, key_type=kt)()  # noqa: E731
    assert make().seed == seed & M64

    # a device tensor in three cuts, the first inside the fill phase
    s = make()
    kd = torch.from_numpy(keys).to(cuda)
    cuts = [0, (k + 1) // 2, 100_001, N]
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.sample_all(kd[a:b])
    assert np.array_equal(s.result(), want), "device batches"

    # host numpy batches (an IndexedSeq: sampled by index, only the winners' keys cross)
    s = make()
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.sample_all(keys[a:b])
    assert np.array_equal(s.result(), want), "host numpy batches"

    # host batches copied whole (an iterator is no IndexedSeq: rsv_sample_batch, RSV_MEM_HOST)
    s = make()
    s.sample_all(iter(keys[:70_003].tolist()))
    s.sample_all(iter(keys[70_003:].tolist()))
    assert np.array_equal(s.result(), want), "copied host batches"

    # per-element sample() for the first 3000 elements, then sample_all
    s = make()
    for x in keys[:3000].tolist():
        s.sample(x)
    s.sample_all(kd[3000:])
    assert np.array_equal(s.result(), want), "per-element"

    # stage_acquire / stage_commit, interleaved with a batch and per-element calls
    L = Nat.load()
    s = make()
    _stage_all(L, Nat, s.handle, keys[: N // 2], 40_000)
    s.sample_all(kd[N // 2: N // 2 + 1000])
    for x in keys[N // 2 + 1000: N // 2 + 1100].tolist():
        s.sample(x)
    _stage_all(L, Nat, s.handle, keys[N // 2 + 1100:], 40_000)
    assert np.array_equal(s.result(), want), "staging"


@pytest.mark.parametrize("k", [1, 64, 1000, 2048, 2049, 9000])
@pytest.mark.parametrize("kt", ["long", "int"])
@pytest.mark.parametrize("seed,sid", PARAMS, ids=PARAM_IDS)
def test_k1_indexed_range_with_64bit_parameters(cuda, oracle, seed, sid, kt, k):
    """sample_all of a Python range: the indexed path (rsv_sample_indexed + rsv_fill_slots), the
    element being its own index."""
    from reservoir_amd import Sampler

    want, _ = oracle.algo_r(seed & M64, sid & M64, k, np.arange(N, dtype=np.int64))
    s = Sampler(k, seed=seed, stream_id=sid, key_type=kt)()
    s.sample_all(range(0, 5))
    s.sample_all(range(5, N))
    got = s.result()
    assert got.dtype == (np.int64 if kt == "long" else np.int32)
    assert np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("seed,sid", PARAMS, ids=PARAM_IDS)
def test_k1_bytes16_with_64bit_parameters(cuda, oracle, seed, sid):
    """Fixed-width byte keys (resolve_wide_kernel behind K1): rows derived from the element's position."""
    import torch

    from reservoir_amd import Sampler

    k = 1000
    ids = np.arange(N, dtype=np.int64)
    rows = lambda i: np.stack([i * 0x9E3779B1 + 7, ~i], axis=1).view(np.uint8)  # noqa: E731
    want_ids, _ = oracle.algo_r(seed & M64, sid & M64, k, ids)
    s = Sampler(k, seed=seed, stream_id=sid, key_type="bytes16")()
    kd = torch.from_numpy(rows(ids)).to(cuda)
    s.sample_all(kd[:500])
    s.sample_all(kd[500:])
    assert np.array_equal(s.result(), rows(want_ids))


@pytest.mark.parametrize("kt", ["long", "int"])
@pytest.mark.parametrize("seed,sid", PARAMS, ids=PARAM_IDS)
def test_k1_index_range_split_with_64bit_parameters(cuda, oracle, seed, sid, kt):
    """A 3-way index-range split (seek + export_packed + merge_packed): every rank draws with the
    same 64-bit key, and the merged reservoir is the single-stream one."""
    import torch

    from reservoir_amd import Sampler

    k, parts = 1000, 3
    keys = _keys(kt)
    want = _want(seed, sid, k, kt)
    kd = torch.from_numpy(keys).to(cuda)
    bounds = [0, 90_001, 200_000, N]
    rows = torch.full((parts - 1, 2 * k), -7, dtype=torch.int64, device=cuda)
    for p in range(parts - 1):
        s = Sampler(k, seed=seed, stream_id=sid, key_type=kt)()
        s.seek(bounds[p])
        s.sample_all(kd[bounds[p]:bounds[p + 1]])
        s.export_packed(rows[p])
        s.close()
    last = Sampler(k, seed=seed, stream_id=sid, key_type=kt)()
    last.seek(bounds[-2])
    last.sample_all(kd[bounds[-2]:])
    last.merge_packed(rows, N)
    assert last.count == N
    assert np.array_equal(last.result(), want)


# ---- K2 ------------------------------------------------------------------------------------------
# stream_base + s is a 64-bit sum: from 2^32 - 150 it carries from s0 into s1 at stream 150 of the
# launch, from 2^64 - 150 it wraps to 0 there
BASES = [SID, 2**32 - 150, 2**64 - 150]
BASE_IDS = ["sid", "carry_s0_s1", "wrap_2pow64"]


@functools.lru_cache(maxsize=None)
def _ragged(k):
    """300 ragged streams of 0..5000 keys, the fill-boundary lengths first."""
    from oracle import oracle

    rng = np.random.default_rng(9000 + k)
    lens = rng.integers(0, 5001, size=300)
    lens[:5] = [0, 1, k - 1, k, k + 1]
    lens[148:153] = [k + 1, 5000, k, 4999, k - 1]  # full-length work on both sides of the carry
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    return lens, offs, oracle.splitmix_keys(31 * k, int(offs[-1]))


@pytest.mark.parametrize("k", [5, 64, 1000, 4416])
@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_k2_segmented_with_64bit_parameters(cuda, oracle, base, k):
    """batch.sample_segmented: the wave form (k = 5, 64) and the workgroup form (k = 1000, 4416)."""
    import torch

    from reservoir_amd import batch

    _, offs, keys = _ragged(k)
    want, wcnt = oracle.algo_r_segmented(SEED, base, k, keys, offs)
    out, cnt = batch.sample_segmented(torch.from_numpy(keys).to(cuda), torch.from_numpy(offs).to(cuda), k,
                                      seed=SEED, stream_base=base)
    assert np.array_equal(cnt.cpu().numpy(), wcnt)
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("dt", ["int64", "int32"])
@pytest.mark.parametrize("k", [64, 1000])
@pytest.mark.parametrize("base", BASES[1:], ids=BASE_IDS[1:])
def test_k2_resumed_with_64bit_parameters(cuda, oracle, base, k, dt):
    """batch.SegmentedSampler.update, every stream cut twice (three updates): the keys of the whole stream
    in the filled slots, and each slot's last writer."""
    import torch

    from reservoir_amd import batch

    lens, offs, keys = _ragged(k)
    keys = keys.astype(dt)
    want, wcnt = oracle.algo_r_segmented(SEED, base, k, keys.astype(np.int64), offs)
    rng = np.random.default_rng(k)
    c1 = rng.integers(0, lens + 1)
    c2 = rng.integers(c1, lens + 1)
    c1[2:5], c2[2:5] = [k // 2, k - 1, k - 1], [k - 1, k - 1, k]  # cuts inside / at the fill boundary
    st = batch.SegmentedSampler(300, k, seed=SEED, stream_base=base, dtype=getattr(torch, dt), device=cuda)
    for lo, hi in ((np.zeros_like(c1), c1), (c1, c2), (c2, lens)):
        piece = np.concatenate([keys[offs[s] + lo[s]: offs[s] + hi[s]] for s in range(300)])
        poffs = np.r_[0, np.cumsum(hi - lo)].astype(np.int64)
        st.update(torch.from_numpy(piece).to(cuda), torch.from_numpy(poffs).to(cuda))
    assert np.array_equal(st.next.cpu().numpy(), lens)
    idx = st.idx.cpu().numpy()
    want_idx = np.stack([oracle.algo_r_last_writers(SEED, (base + s) & M64, k, 0, int(n), 1)
                         for s, n in enumerate(lens)])
    assert np.array_equal(idx, want_idx)
    filled = np.arange(k)[None, :] < wcnt[:, None]
    assert np.array_equal(idx >= 0, filled)
    assert np.array_equal(st.keys.cpu().numpy().astype(np.int64)[filled], want[filled])


def test_export_draws_all_ones_high_index(cuda, oracle):
    """rsv_export_draws at the all-ones key, across index 2^40."""
    from reservoir_amd import batch

    j = batch.export_draws(2**64 - 1, 2**64 - 1, 2**40 - 8, 16).cpu().numpy().astype(np.uint64)
    assert np.array_equal(j, oracle.export_draws(2**64 - 1, 2**64 - 1, 2**40 - 8, 16))
