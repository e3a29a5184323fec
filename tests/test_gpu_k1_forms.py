"""K1's index-range variants and every form a batch is resolved in, against the CPU oracle.

1. k1_body_q<W, FAST> (rsv_scan.h): FAST is chosen per launch when (lo >> 33) == ((hi - 1) >> 33)
   and hi <= 2^40; it rebuilds the winner's index from the launch's block high word ghi, which is
   nonzero only for indices in [2^36, 2^40).  The cases below put launches there, on both sides of
   2^40 and of a multiple of 2^33, and across 2^36 -- at k = 2^20, so that a short range holds
   enough winners (~ k ln(hi / lo)) to mean something; every case first asserts that on the oracle.
2. process_device_batch (rsv_runtime.hip) resolves a batch in one of four forms, chosen by
   kK1FusedMaxK = 2048 (k1_resolve_publish, one dispatch), kFuseMaxDraws = 2^27 (above it the
   two-dispatch form) and kFusedPublishMaxK = 8192 (resolve_kernel<T, true>, which publishes; above it
   resolve_kernel<T, false> and a publication at result()); with a resolve stream the second dispatch is
   resolve_publish_small_kernel<T, 2|4|8> for k <= 512 / 1024 / 2048.  RSV_K1_FUSE=0 and
   RSV_RESOLVE_SMALL=0 force the two-dispatch and the 1024-thread forms; the engine reads them once
   per process, so those cases run in child processes.  The tests do not inspect which kernel ran.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03  # all four 32-bit words nonzero and distinct
K_BIG = 1 << 20


@pytest.fixture(scope="module")
def iota(cuda):
    """arange(2^27) as int32 device keys (512 MB), shared: a slot's key is its winner's offset."""
    import torch

    t = torch.arange(1 << 27, dtype=torch.int32, device=cuda)
    yield t
    del t
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _writers(k, i0, n):
    from oracle import oracle

    w = oracle.algo_r_last_writers(SEED, SID, k, i0, n)
    w.setflags(write=False)
    return w


def _check_state(torch, cuda, s, want_idx, key_of, dt):
    """export_state's idx, the keys of the written slots, and result() (empty slots as zeros)."""
    hit = want_idx >= 0
    want_keys = np.zeros(want_idx.size, dtype=dt)
    want_keys[hit] = key_of(want_idx[hit])
    gidx, gkeys, _, _ = s.export_state(cuda)
    torch.cuda.synchronize()
    assert np.array_equal(gidx.cpu().numpy(), want_idx)
    assert np.array_equal(gkeys.cpu().numpy()[hit], want_keys[hit])
    got = s.result()
    assert got.dtype == dt and np.array_equal(got, want_keys)


RANGES = {  # name: (i0, n)
    "fast_ghi1": (2**36 + 2**33 + 5, 1 << 23),
    "fast_ghi8": (2**39 + 11, 1 << 25),
    "ends_at_2pow40": (2**40 - (1 << 26), 1 << 26),            # FAST, ghi = 15
    "starts_at_2pow40": (2**40, 1 << 26),                      # general, pre_ok false
    "straddles_2pow40": (2**40 - (1 << 25) - 7, 1 << 26),      # general
    "ends_at_3x2pow33": (3 * 2**33 - (1 << 22), 1 << 22),      # FAST
    "starts_at_3x2pow33": (3 * 2**33, 1 << 22),                # FAST
    "straddles_3x2pow33": (3 * 2**33 - (1 << 21) - 9, 1 << 22),  # general, hi_uniform false
    "straddles_2pow36": (2**36 - (1 << 22) - 1, 1 << 23),      # general, K1 splits its launch
}


def _cuts(n, pieces):
    return [0, n] if pieces == 1 else [0, n // 5 + 3, n // 2 + 1, n]


@pytest.mark.parametrize("pieces", [1, 3], ids=["one_batch", "three_cuts"])
@pytest.mark.parametrize("case", list(RANGES))
def test_k1_index_ranges(cuda, oracle, iota, case, pieces):
    """One batch, and three unequal cuts (each batch re-derives FAST from its own lo / hi)."""
    import torch

    from reservoir_amd import Sampler

    i0, n = RANGES[case]
    want_idx = _writers(K_BIG, i0, n)
    assert int((want_idx >= 0).sum()) >= 50, "the range must hold enough winners to mean something"
    s = Sampler(K_BIG, seed=SEED, stream_id=SID, key_type="int")()
    s.seek(i0)
    cuts = _cuts(n, pieces)
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.sample_all(iota[a:b])
    assert s.count == i0 + n
    _check_state(torch, cuda, s, want_idx, lambda idx: idx - i0, np.int32)


@pytest.mark.parametrize("pieces", [1, 3], ids=["one_batch", "three_cuts"])
@pytest.mark.parametrize("case", ["fast_ghi1", "straddles_2pow40"])
def test_k1_index_ranges_long_keys(cuda, oracle, case, pieces):
    """The 8-byte gather of the same launches: splitmix keys."""
    import torch

    from reservoir_amd import Sampler

    i0, n = RANGES[case]
    want_idx = _writers(K_BIG, i0, n)
    assert int((want_idx >= 0).sum()) >= 50
    keys = oracle.splitmix_keys(i0 & 0xFFFF, n)
    kd = torch.from_numpy(keys).to(cuda)
    s = Sampler(K_BIG, seed=SEED, stream_id=SID)()
    s.seek(i0)
    cuts = _cuts(n, pieces)
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.sample_all(kd[a:b])
    _check_state(torch, cuda, s, want_idx, lambda idx: keys[idx - i0], np.int64)
    del kd
    torch.cuda.empty_cache()


# ---- the fused kernel away from base 0 --------------------------------------------------------------
def test_fused_non_fast(cuda, oracle, iota):
    """k = 2048 and 2^27 draws in one batch that crosses index 2^33: one k1_resolve_publish launch
    running k1_body_q<.., false> (hi_uniform false)."""
    import torch

    from reservoir_amd import Sampler

    k, i0, n = 2048, 2**33 - (1 << 26) - 3, 1 << 27
    want_idx = _writers(k, i0, n)
    assert int((want_idx >= 0).sum()) >= 20  # ~ k n / i0 = 32 expected
    s = Sampler(k, seed=SEED, stream_id=SID, key_type="int")()
    s.seek(i0)
    s.sample_all(iota[:n])
    _check_state(torch, cuda, s, want_idx, lambda idx: idx - i0, np.int32)


@pytest.mark.parametrize("kt", ["long", "int"])
def test_fused_fast_high_base_two_batches(cuda, oracle, iota, kt):
    """k = 2048 after seek(2^32 - 100), two fused batches: the second is not fresh, so the slots it
    leaves alone are published from slot_key as the first batch left them."""
    import torch

    from reservoir_amd import Sampler

    k, i0, n = 2048, 2**32 - 100, 1 << 24
    want_idx = _writers(k, i0, n)
    assert int((want_idx >= 0).sum()) >= 1
    if kt == "int":
        kd, key_of, dt = iota[:n], (lambda idx: idx - i0), np.int32
    else:
        keys = oracle.splitmix_keys(77, n)
        kd, key_of, dt = torch.from_numpy(keys).to(cuda), (lambda idx: keys[idx - i0]), np.int64
    s = Sampler(k, seed=SEED, stream_id=SID, key_type=kt)()
    s.seek(i0)
    cut = n // 3 + 5
    s.sample_all(kd[:cut])
    s.sample_all(kd[cut:])
    _check_state(torch, cuda, s, want_idx, key_of, dt)


def test_fused_whole_window_grid_and_ticket_rearm(cuda, oracle, iota):
    """k = 1024, 10^8 draws from base 0 in one batch: fused (<= 2^27 draws) and, from per_window x 768
    level-0 blocks on, launched with k1_grid's whole-window grid.  Then fused launches of another
    grid size queued back to back on the same stream: the completion ticket is re-armed by each."""
    import torch

    from reservoir_amd import Sampler

    k, n, n_small = 1024, 10**8, 3_000_001
    want = _writers(k, 0, n).astype(np.int32)
    want_small = _writers(k, 0, n_small).astype(np.int32)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    live = []
    for m in (n, n_small, n, n_small):
        s = Sampler(k, seed=SEED, stream_id=SID, key_type="int")()
        s.set_stream(stream)
        s.sample_all(iota[:m])
        live.append((s, m))
    for s, m in live:
        assert np.array_equal(s.result(), want if m == n else want_small), m


# ---- every resolve form at the smallest shapes (child processes) ------------------------------------
_FORMS_CASE = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from oracle import oracle
from reservoir_amd import Sampler
SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
cuda = torch.device("cuda", 0)
torch.cuda.set_device(0)
N = 300_000
main = torch.cuda.current_stream(cuda).cuda_stream
side_stream = torch.cuda.Stream(device=cuda)
side = side_stream.cuda_stream
checked = 0
for kt, dt in (("long", np.int64), ("int", np.int32)):
    keys = oracle.splitmix_keys(0xF0 + len(kt), N).astype(dt)
    kd = torch.from_numpy(keys).to(cuda)
    for k in (1, 63, 64, 65, 512, 513, 1024, 1025, 2048, 2049, 8192):
        # a first batch inside the fill phase (fresh: the slots past it are -1 / 0), one that crosses
        # k, two entirely past k, an empty tail
        cuts = [0, k // 2, k + 37, 150_000 + k, N, N]
        want = [oracle.algo_r(SEED, SID, k, keys[:c].astype(np.int64))[0].astype(dt) for c in cuts]
        want_idx = oracle.algo_r_last_writers(SEED, SID, k, 0, N)
        for forked in (False, True):
            for reusable in (False, True):
                s = Sampler(k, seed=SEED, stream_id=SID, key_type=kt, reusable=reusable)()
                if forked:
                    s.set_stream(main)
                    s.set_resolve_stream(side)
                for a, b in zip(cuts[:-1], cuts[1:]):
                    s.sample_all(kd[a:b])
                    if reusable:  # the published generation of every batch, not only the last
                        got = s.result()
                        assert got.dtype == dt and np.array_equal(got, want[cuts.index(b)]), (kt, k, forked, b)
                        checked += 1
                if reusable:
                    idx, kk, _, _ = s.export_state(cuda)
                    torch.cuda.synchronize()
                    assert np.array_equal(idx.cpu().numpy(), want_idx), (kt, k, forked)
                    assert np.array_equal(kk.cpu().numpy(), want[-1]), (kt, k, forked)
                got = s.result()
                assert got.dtype == dt and np.array_equal(got, want[-1]), (kt, k, forked, reusable)
                checked += 1
                s.close()
        # a handle whose first batch is already past the fill phase (fresh, no fill): empty slots -1 / 0
        for forked in (False, True):
            s = Sampler(k, seed=SEED, stream_id=SID, key_type=kt)()
            if forked:
                s.set_stream(main)
                s.set_resolve_stream(side)
            i0 = min(40 * k + 3, 100_003)
            s.seek(i0)
            s.sample_all(kd[: N - i0])
            w = oracle.algo_r_last_writers(SEED, SID, k, i0, N - i0)
            idx, kk, _, _ = s.export_state(cuda)
            torch.cuda.synchronize()
            assert np.array_equal(idx.cpu().numpy(), w), (kt, k, forked)
            wk = np.where(w >= 0, keys[np.maximum(w - i0, 0)], 0).astype(dt)
            assert np.array_equal(kk.cpu().numpy(), wk), (kt, k, forked)
            assert np.array_equal(s.result(), wk), (kt, k, forked)
            checked += 1
torch.cuda.synchronize()
print("resolve forms ok", checked)
"""


@pytest.mark.parametrize("env", [{"RSV_K1_FUSE": "0"}, {"RSV_K1_FUSE": "0", "RSV_RESOLVE_SMALL": "0"}],
                         ids=["two_dispatch", "two_dispatch_1024_threads"])
def test_resolve_forms(cuda, oracle, env):
    """RSV_K1_FUSE=0: every batch is k1_last_writer + a resolve dispatch -- on the sampler's own stream
    resolve_kernel<T, true> with min(1024, roundup64(k)) threads (k = 1 .. 8192: 64 .. 1024 threads);
    with set_resolve_stream resolve_publish_small_kernel<T, 2|4|8> up to k = 2048 and the 1024-thread
    form above.  RSV_RESOLVE_SMALL=0 as well: the 1024-thread form on the resolve stream everywhere.
    long and int keys; the batches of a sampler hit every branch of the resolve kernels (fill inside
    a fresh handle, a batch crossing k, batches past k, an empty tail, a fresh handle with no fill),
    and a reusable sampler's result() is read after every batch (the published generation)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _FORMS_CASE.format(root=root)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "resolve forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
