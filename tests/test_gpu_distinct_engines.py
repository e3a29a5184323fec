"""The host contract the three distinct engines share behind the C ABI (Int, Long and byte keys):
the rsv_export_log state machine with its statuses and messages, rsv_retain_log's before / after
sampling rule, every rsv_get_distinct_info field on a fresh, a part-filled and a full handle, and one
export_log -> merge_log round trip against the oracle's RandomValues (Sampler.scala:383-412).

One tiny shape: k = 64, 2,000 elements, the hashes folded to 40 values, so every hash bucket holds
many distinct keys and the set's boundary bucket ties.  Long keys collide under the default
Long.hashCode; Int and 16-byte keys carry a precomputed hash (an 8-byte row per Int key for the
byte-row oracle: equal rows are equal keys).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY_TYPES = ["int", "long", "bytes16"]
K, N, FOLD, SEED = 64, 2000, 40, 5
PART = 30  # a batch that leaves the set part-filled
I64_MIN, I64_MAX = -2**63, 2**63 - 1
OK, E_ILLEGAL_ARGUMENT, E_UNSUPPORTED = 0, 1, 6

MSG_SET = "rsv_export_log needs an RSV_DISTINCT_ORDERED sampler"
MSG_NOT_RETAINED = "rsv_export_log: the candidate log was not retained (rsv_retain_log before sampling)"
MSG_DROPPED = "rsv_export_log: the candidate log was not retained (archive limit, or sampled after a merge)"
MSG_CAP = "rsv_export_log: cap is smaller than the number of candidates (*out_n)"


@functools.lru_cache(maxsize=None)
def _data(key_type):
    """(keys, hashes or None): ~30 % repeats, FOLD hash values"""
    rng = np.random.default_rng(len(key_type))
    ids = np.concatenate([np.arange(1400), rng.integers(0, 1400, N - 1400)])
    rng.shuffle(ids)
    fold = (ids * 7919) % FOLD
    if key_type == "long":  # Long.hashCode = hi ^ lo takes the FOLD values
        hi = (ids * 2654435761) % 2**31
        return (hi << 32) | ((hi ^ fold) & 0xFFFFFFFF), None
    if key_type == "int":
        return ((ids * 2654435761) % 2**32 - 2**31).astype(np.int32), (fold - FOLD // 2).astype(np.int64)
    z = ids.astype(np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15) + np.array([1, 0x632BE59BD9B4E01A], dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    return np.ascontiguousarray(z ^ (z >> np.uint64(31))).view(np.uint8).reshape(N, 16), (fold - FOLD // 2).astype(np.int64)


def _canon(key_type, keys):
    """a set of keys as sorted byte strings (Int keys widened to 8 bytes, as the oracle's rows)"""
    a = np.ascontiguousarray(keys)
    if a.dtype.kind == "V":
        a = a.view(np.uint8)
    if a.dtype == np.uint8:  # byte rows already (the engine's byte keys, every oracle row)
        a = a.reshape(-1, 16 if key_type == "bytes16" else 8)
    else:
        a = a.astype(np.int64).view(np.uint8).reshape(-1, 8)
    return sorted(bytes(r) for r in a)


@functools.lru_cache(maxsize=None)
def _oracle(key_type, n):
    """the reference's set over the first n elements: (canonical keys, scrambled hashes)"""
    from oracle import oracle as O

    keys, hs = _data(key_type)
    if key_type == "long":
        ref = O.Distinct(K, SEED, O.HASH_JAVA_LONG)
        ref.sample_all(keys[:n])
    else:
        width = 16 if key_type == "bytes16" else 8
        rows = keys[:n] if key_type == "bytes16" else keys[:n].astype(np.int64).view(np.uint8).reshape(-1, 8)
        ref = O.DistinctRows(K, SEED, width)
        ref.sample_all(rows, hs[:n])
    got, sh = ref.result()
    return _canon(key_type, got), sh


def _make(key_type, order, retain=False):
    from reservoir_amd import Sampler

    mk = Sampler.distinct(K, seed=SEED, key_type=key_type, order=order, retain_log=retain)
    return mk() if key_type == "long" else mk(hash=lambda b: 0)


def _feed(cuda, s, key_type, lo=0, hi=N):
    import torch

    keys, hs = _data(key_type)
    kd = torch.from_numpy(keys[lo:hi]).to(cuda)
    s.sample_all(kd, hashes=None if hs is None else torch.from_numpy(hs[lo:hi]).to(cuda))


def _export_log_raw(s, cap):
    """rsv_export_log through the raw ABI: (status, *out_n, rsv_last_error())"""
    n = C.c_int64(-1)
    h = np.empty(max(cap, 1), dtype=np.int64)
    k = np.empty(max(cap, 1), dtype=s._dtype)
    hp, kp = (h.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)) if cap else (None, None)
    st = s._L.rsv_export_log(s.handle, I64_MAX, hp, kp, cap, C.byref(n))
    return st, n.value, s._L.rsv_last_error().decode()


@functools.lru_cache(maxsize=None)
def _state_machine(cuda, key_type):
    """every state of rsv_export_log on one key type: step -> (status, *out_n, message)"""
    import torch

    out = {}
    s = _make(key_type, "set")
    _feed(cuda, s, key_type)
    out["set"] = _export_log_raw(s, 0)
    s = _make(key_type, "ordered")
    _feed(cuda, s, key_type)
    out["not_retained"] = _export_log_raw(s, 0)
    s = _make(key_type, "ordered", retain=True)
    _feed(cuda, s, key_type)
    out["count"] = _export_log_raw(s, 0)
    cnt = out["count"][1]
    out["short"] = _export_log_raw(s, cnt // 2)
    out["exact"] = _export_log_raw(s, cnt)
    out["log_entries"] = s.distinct_info()["log_entries"]
    rows = torch.empty((1, s.packed_width), dtype=torch.int64, device=cuda)
    s.export_packed(rows[0])
    s.merge_packed(rows, s.count)
    out["merged"] = _export_log_raw(s, 0)  # readable until the sampler samples again
    _feed(cuda, s, key_type, 0, 100)
    out["dropped"] = _export_log_raw(s, 0)
    out["dropped_info"] = s.distinct_info()["log_retained"]
    return out


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_export_log_state_machine(cuda, key_type):
    r = _state_machine(cuda, key_type)
    assert r["set"][0] == E_UNSUPPORTED and r["set"][2] == MSG_SET
    assert r["not_retained"][0] == E_UNSUPPORTED and r["not_retained"][2] == MSG_NOT_RETAINED
    st, cnt, _ = r["count"]
    assert st == OK and cnt >= K  # cap = 0: the count alone (at least the heap's first fill)
    assert 0 < cnt // 2 < cnt
    assert r["short"][0] == E_ILLEGAL_ARGUMENT and r["short"][1] == cnt and r["short"][2] == MSG_CAP
    assert r["exact"][:2] == (OK, cnt)
    assert r["log_entries"] >= cnt  # an upper bound on the count
    assert r["merged"][:2] == (OK, cnt)
    assert r["dropped"][0] == E_UNSUPPORTED and r["dropped"][2] == MSG_DROPPED
    assert r["dropped_info"] == 0


def test_export_log_messages_equal_across_key_types(cuda):
    runs = [_state_machine(cuda, kt) for kt in KEY_TYPES]
    for step in ("set", "not_retained", "short", "dropped"):
        st = {(r[step][0], r[step][2]) for r in runs}
        assert len(st) == 1, (step, st)


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_retain_log_before_and_after_the_first_sample(cuda, key_type):
    early = _make(key_type, "ordered")
    early.retain_log(True)
    assert early.distinct_info()["log_retained"] == 1
    _feed(cuda, early, key_type, 0, PART)
    assert early.distinct_info()["log_retained"] == 1
    late = _make(key_type, "ordered")
    _feed(cuda, late, key_type, 0, PART)
    late.retain_log(True)  # the earlier candidates are gone
    assert late.distinct_info()["log_retained"] == 0
    assert _export_log_raw(late, 0)[0] == E_UNSUPPORTED


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_distinct_info_fresh_part_filled_full(cuda, key_type):
    s = _make(key_type, "ordered", retain=True)
    assert s.distinct_info() == dict(ordered=1, tied=0, log_retained=1, size=0, max_hash=I64_MIN, log_entries=0,
                                     sched_passes=0, sched_fallbacks=0)
    _feed(cuda, s, key_type, 0, PART)
    part_keys, part_h = _oracle(key_type, PART)
    info = s.distinct_info()
    assert 0 < len(part_keys) < K
    assert info["size"] == len(part_keys) and info["max_hash"] == int(part_h.max())
    assert info["ordered"] == 1 and info["tied"] == 0 and info["log_retained"] == 1
    assert info["log_entries"] >= len(part_keys)  # every distinct element was a candidate
    _feed(cuda, s, key_type, PART, N)
    _, full_h = _oracle(key_type, N)
    info = s.distinct_info()
    assert info["size"] == K and info["max_hash"] == int(full_h.max())
    # FOLD hash values over 1400 distinct keys: the boundary bucket holds more than the set keeps
    assert info["ordered"] == 1 and info["tied"] == 1 and info["log_retained"] == 1
    assert info["log_entries"] >= _export_log_raw(s, 0)[1] >= K
    assert info["sched_passes"] == 0 and info["sched_fallbacks"] == 0  # far too short for a scheduled pass
    u = _make(key_type, "set")
    assert u.distinct_info() == dict(ordered=0, tied=0, log_retained=0, size=0, max_hash=I64_MIN, log_entries=0,
                                     sched_passes=0, sched_fallbacks=0)
    _feed(cuda, u, key_type)
    info = u.distinct_info()
    assert info["ordered"] == 0 and info["log_retained"] == 0 and info["log_entries"] == 0
    assert info["size"] == K and info["max_hash"] == int(full_h.max())


def test_wide_scheduled_pass_is_not_counted(cuda, capfd, monkeypatch):
    """Byte keys report sched_passes = sched_fallbacks = 0 even after a batch that took their
    scheduled pass (test_wide_sched_pass's smallest scheduled case: k = 100, 400,000 rows)."""
    import torch

    from reservoir_amd import Sampler

    monkeypatch.setenv("RSV_WIDE_SCHED_DEBUG", "1")
    k, n = 100, 400_000
    rng = np.random.default_rng(k)
    rows = torch.from_numpy(rng.integers(I64_MIN, I64_MAX, size=(n, 2), dtype=np.int64)).to(cuda)
    hs = torch.from_numpy(rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64)).to(cuda)
    d = Sampler.distinct(k, key_type="bytes16", seed=5)(hash=lambda b: 0)
    assert d.is_ordered
    d.sample_all(rows.view(torch.uint8).reshape(n, 16), hashes=hs)
    info = d.distinct_info()
    assert "[rsv wide sched]" in capfd.readouterr().err  # the pass ran
    assert info["size"] == k and info["sched_passes"] == 0 and info["sched_fallbacks"] == 0


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_log_round_trip_equals_the_oracle(cuda, key_type):
    """export_log -> merge_log into a fresh handle -> result(): the reference's set, tie bucket included"""
    s = _make(key_type, "ordered", retain=True)
    _feed(cuda, s, key_type)
    h, keys = s.export_log()
    t = _make(key_type, "ordered")
    t.merge_log(h, keys, s.count)
    assert t.count == N
    info = t.distinct_info()
    assert info["size"] == K and info["tied"] == 0  # the replica's exact set
    assert _canon(key_type, t.result()) == _oracle(key_type, N)[0]
