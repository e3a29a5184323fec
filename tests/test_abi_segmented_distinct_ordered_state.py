"""rsv_distinct_segmented_ordered_update validates its arguments before any device call (CPU only): every
status below comes back with NULL pointers, in the order rsv_distinct_segmented_update checks its own;
state_hashes_dev is required by name (the heap is ordered by the stored hashes)."""
import ctypes as C

import pytest

FN = "rsv_distinct_segmented_ordered_update"


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _update(L, B=1, S=1, width=8, k=4, kind=1, hashes=None, ids=None, bufs=None, state_hashes="bufs"):
    sh = bufs if state_hashes == "bufs" else state_hashes
    return getattr(L, FN)(bufs, hashes, bufs, ids, B, S, width, k, kind, 0, 0, bufs, sh, bufs, None)


def test_symbol_is_bound(native):
    assert FN in native.EXPORTED_SYMBOLS
    L = native.load()
    assert hasattr(L, FN)
    assert getattr(L, FN).restype is C.c_int32
    assert list(getattr(L, FN).argtypes) == list(L.rsv_distinct_segmented_update.argtypes)
    assert len(getattr(L, FN).argtypes) == 15


def test_header_declares_it(native):
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "reservoir_hip.h")).read()
    assert "rsv_status " + FN + "(" in text


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=4097), "E_UNSUPPORTED"),
    (dict(width=16), "E_UNSUPPORTED"),
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=9), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=2, S=1), "E_ILLEGAL_ARGUMENT"),   # no ids: segment b is row b
    (dict(B=1, S=0), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0), "OK"),
    (dict(B=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=4096, width=4, kind=0), "E_NULL_POINTER"),
    (dict(kind=4), "E_NULL_POINTER"),
])
def test_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _update(L, **args) == getattr(native, status), args


def test_statuses_equal_the_set_update(native):
    """The same bad arguments give the same status as rsv_distinct_segmented_update, check by check."""
    L = native.load()
    for args in (dict(k=0), dict(k=4097), dict(width=16), dict(width=3), dict(kind=9), dict(B=-1), dict(S=-1),
                 dict(B=2, S=1), dict(B=0), dict(), dict(kind=4),
                 dict(k=0, width=3), dict(k=4097, width=16), dict(width=16, kind=9), dict(kind=9, B=-1)):
        a = dict(B=1, S=1, width=8, k=4, kind=1)
        a.update(args)
        want = L.rsv_distinct_segmented_update(None, None, None, None, a["B"], a["S"], a["width"], a["k"], a["kind"],
                                               0, 0, None, None, None, None)
        assert _update(L, **args) == want, args


def test_zero_states_with_ids_is_ok(native):
    """num_states == 0 returns RSV_OK without touching a pointer (with ids, B may exceed it)."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    assert _update(L, B=3, S=0, ids=C.cast(buf, C.c_void_p)) == native.OK


def test_null_state_hashes_is_a_null_pointer(native):
    """Every other buffer given (never dereferenced: the check comes first), state_hashes_dev NULL."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert _update(L, bufs=p, state_hashes=None) == native.E_NULL_POINTER
    assert "state_hashes_dev" in L.rsv_last_error().decode()


def test_precomputed_without_hashes_is_a_null_pointer(native):
    L = native.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert _update(L, kind=native.HASH_PRECOMPUTED, hashes=None, bufs=p) == native.E_NULL_POINTER
    assert "hashes_dev" in L.rsv_last_error().decode() and "state_hashes_dev" not in L.rsv_last_error().decode()


def test_limit_and_byte_keys_name_the_entry_point(native):
    L = native.load()
    assert _update(L, k=4097) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert "4096" in msg and FN + " " in msg + " "
    assert _update(L, width=16) == native.E_UNSUPPORTED
    assert FN + " " in L.rsv_last_error().decode() + " "


def test_abi_version_is_unchanged(native):
    assert native.load().rsv_abi_version() == 1
