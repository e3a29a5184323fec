"""K1's launch forms at the sizes where they exist, against the CPU oracle (exact slot indices).

k1_plan (rsv_elements.hip) launches k1_body_q (rsv_scan.h) grid-stride below ~4.4e8 draws and over its
two-group schedule above; under the schedule the slow iterations (the dense head below index 256 k, the
launch's clipped ends) are dealt round-robin over the first group's waves and the steady units are strided
within the two groups, all from launch-uniform values the host passes (K1Launch).  The cases run at ~1e9
draws, the size the schedule was fitted at (the first group's waves take 12 units each), and at the switch:
every case is one or two launches (< 1 ms each) and one oracle pass.  The batches are index-only
(rsv_sample_indexed, then rsv_fill_slots with k zero keys): no key array exists, and export_state's slot
indices are compared with oracle.algo_r_last_writers, equal in every slot.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03  # all four 32-bit words nonzero and distinct
N9 = 10**9
K_BIG = 1 << 20

# k1_plan's switch: the schedule from 5 * 6144 + 5400 steady units (half windows of 768 level-0 blocks of 16
# indices); at k = 1024 from index 0 the steady units start behind the 16384 dense blocks
UNIT_DRAWS = 768 * 16
SWITCH_UNITS = 5 * 6144 + 5400
HEAD_DRAWS_K1024 = 16384 * 16


@functools.lru_cache(maxsize=None)
def _writers(k, i0, n):
    from oracle import oracle

    w = oracle.algo_r_last_writers(SEED, SID, k, i0, n)
    w.setflags(write=False)
    return w


def _indices_after(cuda, k, i0, n):
    """export_state's slot indices after one index-only batch of n draws from index i0 on a fresh handle."""
    import torch

    from reservoir_amd import Sampler, _native as N

    s = Sampler(k, seed=SEED, stream_id=SID)()
    if i0:
        s.seek(i0)
    offs = np.empty(k, dtype=np.int64)
    N.check(s._L.rsv_sample_indexed(s.handle, n, offs.ctypes.data_as(C.c_void_p)))
    N.check(s._L.rsv_fill_slots(s.handle, np.zeros(k, dtype=np.int64).ctypes.data_as(C.c_void_p)))  # k keys, all 0
    assert s.count == i0 + n
    idx, _, _, _ = s.export_state(cuda)
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    s.close()
    return got


def _check(cuda, k, i0, n, min_winners):
    want = _writers(k, i0, n)
    assert int((want >= 0).sum()) >= min_winners, "the range must hold enough winners to mean something"
    got = _indices_after(cuda, k, i0, n)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (k, i0, n, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("k", [1, 64, 1024, K_BIG])
def test_schedule_from_index_zero(cuda, oracle, k):
    """[0, 1e9 + 7) on a fresh handle: the dense head is 0, 8, 128 and 131072 iterations (k = 2^20: 27 % of
    the launch, ~21 per first-group wave), the last block is clipped, and every slot has a writer."""
    _check(cuda, k, 0, N9 + 7, k)


def test_schedule_lo_clipped_inside_a_block(cuda, oracle):
    """A seek to index 3: the launch's first block is clipped at its low end."""
    _check(cuda, 1024, 3, N9, 1024)


def test_schedule_without_dense_region(cuda, oracle):
    """A seek to 2^30, past 256 k: no head, every unit steady but the clipped tail (~0.66 k winners)."""
    _check(cuda, 1024, 1 << 30, N9, 500)
    _check(cuda, K_BIG, 1 << 30, N9 + 5, 500_000)


def test_schedule_fast_high_block_word(cuda, oracle):
    """A seek to 2^36 + 5: FAST, and the block counter's high word is 1 (~ k 1e9 / 2^36 = 15 k winners)."""
    _check(cuda, K_BIG, (1 << 36) + 5, N9, 10_000)


def test_schedule_non_fast(cuda, oracle):
    """Across 2^40: K1 splits there, and the launch from 2^40 (indices past 2^40: not FAST) takes the
    schedule; and one launch across a multiple of 2^33 (the level-1 counter's high word not uniform)."""
    _check(cuda, K_BIG, (1 << 40) - 1003, N9 + 1003, 500)
    _check(cuda, K_BIG, 3 * (1 << 33) - N9 // 2 - 9, N9, 10_000)


@pytest.mark.parametrize("units", [SWITCH_UNITS - 1, SWITCH_UNITS + 1], ids=["one_unit_below", "one_unit_above"])
def test_schedule_switch(cuda, oracle, units):
    """One unit below the switch (the last grid-stride launch) and one above (the smallest schedule)."""
    _check(cuda, 1024, 0, HEAD_DRAWS_K1024 + units * UNIT_DRAWS, 1024)


def test_grid_stride_launch(cuda, oracle):
    """3e8 draws: the grid-stride form on the same host values."""
    _check(cuda, 1024, 0, 3 * 10**8 + 1, 1024)


_FUSED_CASE = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from oracle import oracle
from reservoir_amd import Sampler
SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
cuda = torch.device("cuda", 0)
torch.cuda.set_device(0)
k, i0, n = 2048, 5, 1 << 27
keys = torch.arange(n, dtype=torch.int32, device=cuda)
s = Sampler(k, seed=SEED, stream_id=SID, key_type="int")()
s.seek(i0)
s.sample_all(keys)
want = oracle.algo_r_last_writers(SEED, SID, k, i0, n)
idx, kk, _, _ = s.export_state(cuda)
torch.cuda.synchronize()
assert (want >= 0).all() and np.array_equal(idx.cpu().numpy(), want)
assert np.array_equal(kk.cpu().numpy(), (want - i0).astype(np.int32))
assert np.array_equal(s.result(), (want - i0).astype(np.int32))
print("fused ok")
"""


def test_fused_form(cuda, oracle):
    """RSV_K1_FUSE=1 (read once per process: a child): 2^27 draws from index 5 at k = 2048 as one
    k1_resolve_publish launch, which takes the same host values."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _FUSED_CASE.format(root=root)], env=dict(os.environ, RSV_K1_FUSE="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "fused ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
