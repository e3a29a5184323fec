"""K1's kernels per form (FAST / general, rsv_scan.h) at the launches tests/test_gpu_k1_schedule.py does not pin,
against the CPU oracle (exact slot indices, empty slots -1).

The host picks k1_last_writer<FAST> / k1_resolve_publish<KeyT, FAST> per launch; a steady half window takes its
append ranks from the wave's LDS word (k1_body_q TOP), so the order of entries inside a wave's queue is the
hardware's -- the winners must not depend on it.  test_gpu_k1_schedule.py pins the two-group schedule at 1e9 draws
in every form and the grid-stride launch from index 0; here:

  * whole steady windows run grid-stride (k1_grid: from 768 * 6144 blocks, ~7.6e7 draws) in the three other
    forms: 8e7 + 3 draws (the last block clipped) from 2^36 + 5 (FAST, block counter high word 1), across a
    multiple of 2^33 (general, the level-1 high word not uniform) and from 2^40 + 3 (general, high word uniform);
  * K1's split at 2^40: (2^40 - 4e7, 8e7) is a FAST launch and a general launch into one winner table;
  * the fused kernel's general form: 2^27 int32 keys from 2^40 + 5, and across 2^33, with RSV_K1_FUSE=1 (a child
    process each).

Each case is one batch (one or two launches) and one oracle pass.  k is chosen per case so that the oracle alone
reports at least 500 winners in the range (counted on the CPU when the cases were fixed: 1189, 3252, 657, 617;
k = 2^23 past 2^40, where 256 k = 2^31 stays far below the start), and the test asserts that count.  The fused
case cannot reach it: the fused kernel takes k <= 2048, and 2048 slots expect 2048 * 2^27 / 2^40 = 0.25 winners
there; with this stream the oracle has exactly one, the test asserts at least one, and every other slot must
come out empty (-1).  So that a missed winner of that kernel shows too, the same launch runs from 2^33 - 2^26
(general: index 2^33 lies inside), where the oracle has 24 winners, asserted as well.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03  # all four 32-bit words nonzero and distinct
N_STRIDE = 8 * 10**7 + 3
K20, K23 = 1 << 20, 1 << 23
WINNERS_2P33 = 24  # the oracle's count for the fused case across 2^33 (counted on the CPU when the case was fixed)


def _indices_after(cuda, k, i0, n):
    """export_state's slot indices after one index-only batch of n draws from index i0 on a fresh handle."""
    import torch

    from reservoir_amd import Sampler, _native as N

    s = Sampler(k, seed=SEED, stream_id=SID)()
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


def _check(cuda, oracle, k, i0, n, min_winners):
    assert 256 * k < i0, "no dense head: every window of the launch is steady but its clipped ends"
    want = oracle.algo_r_last_writers(SEED, SID, k, i0, n)
    winners = int((want >= 0).sum())
    print(f"k={k} i0={i0} n={n}: {winners} winners in the oracle")
    assert winners >= min_winners, "the range must hold enough winners to mean something"
    got = _indices_after(cuda, k, i0, n)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (k, i0, n, bad[:8], got[bad[:8]], want[bad[:8]])
    return want


def test_grid_stride_fast_high_block_word(cuda, oracle):
    """8e7 + 3 draws from 2^36 + 5: grid-stride steady windows in the FAST kernel, block counter high word 1."""
    _check(cuda, oracle, K20, (1 << 36) + 5, N_STRIDE, 500)


def test_grid_stride_general_across_2p33(cuda, oracle):
    """Index 3 * 2^33 lies inside the launch: the general kernel, the level-1 counter's high word per lane."""
    i0 = 3 * (1 << 33) - 4 * 10**7 - 9
    assert i0 < 3 * (1 << 33) < i0 + N_STRIDE
    _check(cuda, oracle, K20, i0, N_STRIDE, 500)


def test_grid_stride_general_past_2p40(cuda, oracle):
    """From 2^40 + 3: the general kernel with a uniform high word (no 32-bit pre-test of a candidate)."""
    _check(cuda, oracle, K23, (1 << 40) + 3, N_STRIDE, 500)


def test_split_at_2p40_fast_then_general(cuda, oracle):
    """(2^40 - 4e7, 8e7): K1 splits at 2^40 -- a FAST launch and a general launch on one handle, one winner table;
    both sides of the split hold winners."""
    i0, n = (1 << 40) - 4 * 10**7, 8 * 10**7
    want = _check(cuda, oracle, K23, i0, n, 500)
    below = int(((want >= 0) & (want < (1 << 40))).sum())
    assert below >= 100 and int((want >= (1 << 40)).sum()) >= 100, below


_FUSED_GENERAL_CASE = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from oracle import oracle
from reservoir_amd import Sampler
SEED, SID = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
cuda = torch.device("cuda", 0)
torch.cuda.set_device(0)
k, i0, n, min_winners = 2048, {i0}, 1 << 27, {min_winners}
keys = torch.arange(n, dtype=torch.int32, device=cuda)
s = Sampler(k, seed=SEED, stream_id=SID, key_type="int")()
s.seek(i0)
s.sample_all(keys)
want = oracle.algo_r_last_writers(SEED, SID, k, i0, n)
won = want >= 0
print("winners", int(won.sum()))
assert int(won.sum()) >= min_winners
idx, kk, _, _ = s.export_state(cuda)
torch.cuda.synchronize()
idx, kk = idx.cpu().numpy(), kk.cpu().numpy()
assert np.array_equal(idx, want), (np.flatnonzero(idx != want)[:8], idx[idx != want][:8])
want_keys = np.where(won, want - i0, 0).astype(np.int32)  # an empty slot's key is zero
assert np.array_equal(kk, want_keys)
assert np.array_equal(s.result(), want_keys)
print("fused general ok")
"""


# (2^40 + 5: the issue's case, one winner in the oracle -- see the module docstring; 2^33 - 2^26: the same kernel
# where 2048 slots expect 2048 * ln((2^33 + 2^26) / (2^33 - 2^26)) = 32 winners and the oracle has 24)
@pytest.mark.parametrize("i0,min_winners", [((1 << 40) + 5, 1), ((1 << 33) - (1 << 26), WINNERS_2P33)],
                         ids=["past_2p40", "across_2p33"])
def test_fused_general_form(i0, min_winners):
    """RSV_K1_FUSE=1 (read once per process: a child): 2^27 int32 keys at k = 2048 as one
    k1_resolve_publish<int, general> launch -- from 2^40 + 5 (no 32-bit pre-test of a candidate) and across 2^33
    (the level-1 high word per lane); slot indices, keys and result() against the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _FUSED_GENERAL_CASE.format(root=root, i0=i0, min_winners=min_winners)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RSV_K1_FUSE="1"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "fused general ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
