"""The handle model of tests/handle_model.py against the oracle, and what the committed seed list of
its program generator covers (CPU only; tests/test_gpu_handle_programs.py runs the programs).

The model is the reference of the GPU programs, so it is pinned here from its own side: any cut of a
contiguous stream gives oracle.algo_r / oracle.AlgoL over the concatenated keys, and ranges A and C of
one stream merged with a sibling's range B give oracle.algo_r over A + B + C."""
from collections import Counter

import numpy as np
import pytest

import handle_model as HM


def test_keys_are_the_oracles(oracle):
    assert np.array_equal(HM.keys_range("long", 1000, 500), oracle.splitmix_keys(HM.KEY_BASE + 1000, 500))
    assert np.array_equal(HM.keys_range("int", 7, 50), oracle.splitmix_keys(HM.KEY_BASE + 7, 50).astype(np.int32))
    assert HM.keys_range("bytes24", 3, 9).shape == (9, 24)
    for name in ("identity", "collide", "int"):
        a = HM.distinct_keys(name, 7, 0, 200)
        assert np.array_equal(a[: HM.distinct_period(7)], a[HM.distinct_period(7): 2 * HM.distinct_period(7)])
    c = HM.distinct_keys("collide", 64, 0, 500).view(np.uint64)
    codes = (c ^ (c >> np.uint64(32))) & np.uint64(0xFFFFFFFF)  # Long.hashCode
    assert np.unique(codes).size <= 96 < np.unique(c).size


@pytest.mark.parametrize("k", [1, 7, 64, 300])
def test_contiguous_programs(oracle, k):
    """100 cut patterns per k and engine: the model fed the pieces == the oracle fed the whole."""
    rng = np.random.default_rng(k)
    n = 4 * k + 257
    keys = HM.keys_range("long", 0, n)
    want_r = {}
    for t in range(100):
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 9))))
        cuts = [0] + cuts.tolist() + [int(rng.integers(0, n + 1))]
        cuts = sorted(cuts)
        end = cuts[-1]
        for engine in ("philox_r", "java_l"):
            m = HM.ElementsModel(oracle, engine, k, 5 + t % 3, 9, "long")
            for a, b in zip(cuts, cuts[1:]):
                m.append(b - a)
            if engine == "philox_r":
                want, _ = oracle.algo_r(5 + t % 3, 9, k, keys[:end])
            else:
                ref = oracle.AlgoL(k, 5 + t % 3)
                ref.sample_all(keys[:end])
                want = ref.result()
            assert m.count == end and np.array_equal(m.result(), want), (engine, cuts)
            want_r[engine] = want
    assert set(want_r) == {"philox_r", "java_l"}


@pytest.mark.parametrize("k", [1, 7, 64, 300])
@pytest.mark.parametrize("key_type", ["long", "int", "bytes24"])
def test_seek_and_merge(oracle, k, key_type):
    """A and C on one model, B on its sibling, merged: algo_r over A + B + C (every cut of [0, n))."""
    rng = np.random.default_rng(k + 1)
    for t in range(40):
        n = int(rng.integers(2, 5 * k + 40))
        a, b = sorted(rng.integers(0, n + 1, size=2).tolist())
        m = HM.ElementsModel(oracle, "philox_r", k, 3, t, key_type)
        m.append(a)
        m.seek(b)
        m.append(n - b)
        sib = HM.ElementsModel(oracle, "philox_r", k, 3, t, key_type)
        sib.seek(a)
        sib.append(b - a)
        m.merge(sib.writers, sib.count)
        want = oracle.algo_r_last_writers(3, t, k, 0, n, 1)
        assert m.count == n and np.array_equal(m.writers, want)
        if key_type == "long":
            ref, _ = oracle.algo_r(3, t, k, HM.keys_range("long", 0, n))
            assert np.array_equal(m.result(), ref)
        else:
            assert np.array_equal(m.result(), HM.keys_at(key_type, want[: min(n, k)]))
        # offsets(): the slots a batch changes, as rsv_sample_indexed reports them
        m2 = HM.ElementsModel(oracle, "philox_r", k, 3, t, key_type)
        m2.append(a)
        offs = m2.offsets(n - a)
        before = m2.writers.copy()
        m2.append(n - a)
        assert np.array_equal(np.where(offs >= 0, offs + a, before), m2.writers)


def test_seek_past_k_leaves_zeros(oracle):
    m = HM.ElementsModel(oracle, "philox_r", 100, 1, 0, "long")
    m.append(40)
    m.seek(5000)
    r = m.result()
    assert r.size == 100 and np.array_equal(r[:40], HM.keys_range("long", 0, 40)) and (r[40:] == 0).all()


def test_distinct_model_merge_is_the_unions_bottom_k(oracle):
    for name in ("identity", "int"):
        a = HM.DistinctModel(oracle, name, 64, 4)
        a.append(150)
        b = HM.DistinctModel(oracle, name, 64, 4)
        b.seek(150)
        b.append(400)
        a.merge(b.result(), b.count)
        whole = HM.DistinctModel(oracle, name, 64, 4)
        whole.append(550)
        assert a.count == 550 and np.array_equal(a.result(), whole.result())


# ---- what the committed seed list covers (conditions, not measurements) -----------------------------
FAMILY_STATES = {f: {"fresh", "holding", "staged", "owed", "external", "closed", "taken"} for f in HM.ELEMENT_FAMILIES}
FAMILY_STATES.update({f: {"fresh", "holding", "staged", "closed", "taken"} for f in HM.DISTINCT_FAMILIES})


@pytest.mark.parametrize("family", HM.FAMILIES)
def test_generator_coverage(family):
    states, below, above = set(), Counter(), Counter()
    result_then_sampling = after_recreate = 0
    ks, lens = set(), set()
    for fam, seed in HM.program_ids():
        if fam != family:
            continue
        prog = HM.gen_program(fam, seed)
        assert prog == HM.gen_program(fam, seed)  # a case is replayed by its id
        ks.add(prog["k"])
        lens.add(len(prog["ops"]) - 1)
        seen_result = seen_recreate = False
        rts = aft = False
        for op, before, k, sts in HM.walk(prog):
            states.update(sts)
            (below if before < k else above)[op[0]] += 1
            if op[0] in HM.SAMPLING_OPS and (len(op) < 2 or op[1] > 0) and seen_result and prog["reusable"]:
                rts = True
            if seen_recreate and op[0] != "final":
                aft = True
            seen_result |= op[0] in ("result", "result_device")
            if op[0] == "recreate":
                seen_recreate, seen_result = True, False
        result_then_sampling += rts
        after_recreate += aft
    assert states == FAMILY_STATES[family], states ^ FAMILY_STATES[family]
    assert ks >= set(HM.KS) and (HM.BIG_K in ks) == family.startswith("el-")
    assert min(lens) >= 12 and max(lens) <= 20
    for op in HM.family_ops(family):
        assert below[op] >= 20 and above[op] >= 20, (op, below[op], above[op])
    assert result_then_sampling >= 10 and after_recreate >= 5
