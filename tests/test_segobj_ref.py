"""segobj_ref, the host reference of the segmented object-distinct tests, against itself (CPU only).

What the GPU tests lean on: replaying any arrival-ordered superset of the reference's admissions gives the
reference's heap, element for element -- so a candidate list is right as soon as it is sorted and holds the
admissions -- and the running T the tightness bound is stated against is the brute-force one.
"""
import numpy as np
import pytest
import segobj_ref as R


def _stream(rng, n, values, repeats):
    """n element ids, a share of them repeats of earlier ones, under a hash of `values` distinct values."""
    ids = rng.integers(0, 2**62, size=n, dtype=np.int64)
    if n > 1:
        again = rng.random(n) < repeats
        src = rng.integers(0, np.maximum(np.arange(n), 1))
        ids = np.where(again, ids[src], ids)
    hashed = ids if values is None else ids % values
    return ids, hashed


@pytest.mark.parametrize("k", [1, 2, 7, 64])
@pytest.mark.parametrize("values", [None, 97, 5])
def test_supersets_of_the_admissions_replay_to_the_same_heap(oracle, k, values):
    rng = np.random.default_rng(1000 * k + (values or 0))
    for n in (0, 1, k, k + 1, 700):
        ids, hashed = _stream(rng, n, values, 0.3)
        sh = R.scrambled(oracle, k, 11, 5, hashed, np.array([0, n]))
        adm, want = R.admissions(k, ids, sh)
        assert R.same_replica(R.replay(k, ids, sh, adm), want)
        assert R.same_replica(R.replay(k, ids, sh, np.arange(n)), want)
        for share in (0.05, 0.5):
            extra = np.flatnonzero(rng.random(n) < share)
            sup = np.union1d(adm, extra)  # sorted: arrival order
            assert R.same_replica(R.replay(k, ids, sh, sup), want), (n, share)


def test_replay_continues_a_replica(oracle):
    """Cut in two: the admissions of the second half from the first half's replica."""
    k, n = 16, 900
    ids, hashed = _stream(np.random.default_rng(3), n, 40, 0.3)
    sh = R.scrambled(oracle, k, 2**64 - 3, 9, hashed, np.array([0, n]))
    _, want = R.admissions(k, ids, sh)
    _, v = R.admissions(k, ids[:400], sh[:400])
    _, v = R.admissions(k, ids[400:], sh[400:], v)
    assert R.same_replica(v, want)


@pytest.mark.parametrize("k", [1, 2, 5, 33])
def test_running_T_is_the_brute_force_one(k):
    rng = np.random.default_rng(k)
    for n, span in ((0, 10), (1, 10), (40, 12), (120, 2**40), (90, 60)):
        sh = rng.integers(-span, span, size=n, dtype=np.int64)
        got, want = R.running_T(k, sh), R.running_T_brute(k, sh)
        assert got.tolist() == want.tolist(), (k, n, span)
    # the extremes are hashes like any other
    sh = np.array([R.MAX, -R.MAX - 1, R.MAX, 0, -R.MAX - 1], dtype=np.int64)
    assert R.running_T(k, sh).tolist() == R.running_T_brute(k, sh).tolist()


def test_forms_mirror_the_package():
    from reservoir_amd import batch

    assert tuple((top, w) for top, _, w in R.FORMS) == batch.SEGMENTED_CANDIDATE_BUFFER
    assert [batch.segmented_candidate_buffer(k) for k in (1, 64, 65, 256, 257, 1024, 1025, 4096)] == \
        [256, 256, 512, 512, 2048, 2048, 8192, 8192]
