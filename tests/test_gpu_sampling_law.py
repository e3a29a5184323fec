"""The samplers against Algorithm R's exact law (tests/sampling_law.py), not against the oracle.

Every other parity test here has the form "the kernel equals the oracle fed the same draws", and the
draws are this project's own draw format R2, restated once in the kernels and once in the oracle.
These tests ask what neither restatement can answer for the other: whether the streams that come out
are fair.  The families, chosen for the index ranges and kernel forms no statistical test reached:

  k1_sparse        K1 index-only, k = 1024, n = 2^26: 99.6 % of the stream lies beyond 256 k, where only
                   a zero level-0 byte is looked at
  k1_past_2pow33   one sampler over 2^33 + 2^21 indices in one indexed batch (no size limit is
                   documented): across 2^32 and a multiple of 2^33, so K1's general launch where
                   k1_sparse's is the FAST one
  k1_adjacent_*    seed or stream_id held, the other at base + t, base + (t << 32), base ^ 2^63: the
                   members shared by consecutive runs (how callers derive ids)
  k1_window_*      k = 2^20 after seek(i0) at 2^36 + 2^33, up to and from 2^40, across 3 x 2^33: a hit there
                   needs b = 0 and the top 16 to 20 bits of L zero, depths no from-zero run reaches
  k2_wave, k2_wg   one launch each: the wave form in its sparse region (k = 4, sparse from 1024 of 4096)
                   and the workgroup form (k = 512, sparse from 2^17 of 2^18)
  java_l           the reference's Algorithm L over java.util.Random
  distinct_*       segmented distinct over the same 1000 keys in 16384 streams seeded seed + stream_base + s

Each statistic's bound follows from the law and alpha = 1e-6 / 44 (44 statistics in this file); the
power of each table at these totals is shown in tests/test_sampling_law_oracle.py, and the oracle's
figures at the same T and seeds are recorded by tools/sampling_law_stats.py in
profiles/sampling_law/.  A failure here is reproduced on the oracle first (same seeds, bit-equal
tables): no bound is widened and no seed replaced.
"""
import os
import sys

import pytest

import sampling_law as SL

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sampling_law_stats as ST  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_iota():
    yield
    if ST._IOTA:
        import torch

        ST._IOTA.clear()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("family", list(SL.GPU_FAMILIES))
def test_family_obeys_the_law(cuda, family):
    fam = SL.GPU_FAMILIES[family]
    tables = ST.run_family(fam, "gpu", cuda)
    stats = SL.evaluate(fam, tables, SL.GPU_ALPHA)
    assert [e["stat"] for e in stats] == list(fam["stats"])
    for e in stats:
        print(family, e)
    assert all(e["ok"] for e in stats), [e for e in stats if not e["ok"]]
