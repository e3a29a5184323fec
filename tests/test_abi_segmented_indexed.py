"""rsv_sample_segmented_indexed / _update / _merge validate their arguments before any device call (CPU only):
every status below comes back with NULL pointers, in the order of their keyed siblings without a key width
(k, negative counts, the zero-count RSV_OK returns, NULL buffers; the update's two extra cases B > S without
ids and S == 0)."""
import ctypes as C

import pytest

LIMIT = 15104  # the largest k whose 64-bit winner table fits one workgroup's LDS


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _stateless(L, S=1, k=4, bufs=None):
    return L.rsv_sample_segmented_indexed(bufs, S, k, 0, 0, bufs, bufs, None)


def _update(L, B=1, S=1, k=4, ids=None, bases=None, bufs=None):
    return L.rsv_sample_segmented_indexed_update(bufs, ids, bases, B, S, k, 0, 0, bufs, bufs, bufs, bufs, None)


def _merge(L, P=1, S=1, k=4, bufs=None):
    return L.rsv_sample_segmented_indexed_merge(bufs, bufs, P, S, k, bufs, bufs, bufs, None)


def test_symbols_are_bound_with_the_documented_argtypes(native):
    L = native.load()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    want = {
        "rsv_sample_segmented_indexed": [vp, i64, i32, u64, u64, vp, vp, vp],
        "rsv_sample_segmented_indexed_update": [vp, vp, vp, i64, i64, i32, u64, u64, vp, vp, vp, vp, vp],
        "rsv_sample_segmented_indexed_merge": [vp, vp, i32, i64, i32, vp, vp, vp, vp],
    }
    for name, argtypes in want.items():
        assert name in native.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is i32
        assert list(fn.argtypes) == argtypes, name
    assert L.rsv_abi_version() == 1


def test_header_declares_the_three(native):
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "reservoir_hip.h")).read()
    for name, nargs in (("rsv_sample_segmented_indexed", 8), ("rsv_sample_segmented_indexed_update", 13),
                        ("rsv_sample_segmented_indexed_merge", 9)):
        m = re.search(r"rsv_status " + name + r"\(([^)]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=0, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=0), "OK"),
    (dict(S=0, k=LIMIT + 1), "OK"),                      # the stateless launch takes any k the keyed one takes
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT + 1), "E_NULL_POINTER"),
    (dict(k=1), "E_NULL_POINTER"),
])
def test_stateless_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _stateless(L, **args) == getattr(native, status), args


def test_stateless_checks_each_pointer(native):
    L = native.load()
    buf = C.cast((C.c_int64 * 8)(), C.c_void_p)
    for a in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert L.rsv_sample_segmented_indexed(a[0], 1, 4, 0, 0, a[1], a[2], None) == native.E_NULL_POINTER


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=LIMIT + 1), "E_UNSUPPORTED"),
    (dict(k=LIMIT + 1, B=-1), "E_UNSUPPORTED"),         # k comes before the counts
    (dict(B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0, S=-1), "E_ILLEGAL_ARGUMENT"),            # negative counts come before the zero returns
    (dict(B=2, S=1), "E_ILLEGAL_ARGUMENT"),             # no ids: segment b is row b
    (dict(B=1, S=0), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0), "OK"),
    (dict(B=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT), "E_NULL_POINTER"),
    (dict(k=1), "E_NULL_POINTER"),
])
def test_update_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _update(L, **args) == getattr(native, status), args


def test_update_zero_states_with_ids_is_ok(native):
    """num_states == 0 returns RSV_OK without touching a pointer (with ids, B may exceed it)."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    assert _update(L, B=3, S=0, ids=C.cast(buf, C.c_void_p)) == native.OK


def test_update_more_segments_than_rows_with_ids_reaches_the_buffers(native):
    L = native.load()
    buf = (C.c_int64 * 8)()
    assert _update(L, B=3, S=1, ids=C.cast(buf, C.c_void_p)) == native.E_NULL_POINTER


def test_update_checks_each_pointer(native):
    """offsets, idx, next, hits and hit_counts are all required; stream_ids and bases are not."""
    L = native.load()
    buf = C.cast((C.c_int64 * 8)(), C.c_void_p)
    for missing in range(5):
        a = [buf] * 5
        a[missing] = None
        got = L.rsv_sample_segmented_indexed_update(a[0], None, None, 1, 1, 4, 0, 0, a[1], a[2], a[3], a[4], None)
        assert got == native.E_NULL_POINTER, missing


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=LIMIT + 1), "E_UNSUPPORTED"),
    (dict(k=LIMIT + 1, P=-1), "E_UNSUPPORTED"),
    (dict(P=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0), "OK"),
    (dict(S=0), "OK"),
    (dict(P=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT), "E_NULL_POINTER"),
])
def test_merge_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _merge(L, **args) == getattr(native, status), args


def test_merge_checks_each_pointer(native):
    L = native.load()
    buf = C.cast((C.c_int64 * 8)(), C.c_void_p)
    for missing in range(5):
        a = [buf] * 5
        a[missing] = None
        assert L.rsv_sample_segmented_indexed_merge(a[0], a[1], 1, 1, 4, a[2], a[3], a[4], None) == native.E_NULL_POINTER


def test_limit_is_named(native):
    L = native.load()
    assert _update(L, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "rsv_sample_segmented_indexed_update" in msg
    assert _merge(L, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "rsv_sample_segmented_indexed_merge" in msg


def test_python_mirrors_the_limit(native):
    from reservoir_amd import batch

    assert batch.SegmentedObjectSampler._MAX_K == LIMIT
