"""rsv_distinct_segmented_update / rsv_distinct_segmented_merge validate their arguments before any
device call (CPU only): every status below comes back with NULL pointers, in the order
rsv_distinct_segmented checks its own."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _update(L, B=1, S=1, width=8, k=4, kind=1, hashes=None, ids=None, bufs=None):
    return L.rsv_distinct_segmented_update(bufs, hashes, bufs, ids, B, S, width, k, kind, 0, 0, bufs, bufs, bufs, None)


def _merge(L, P=1, S=1, width=8, k=4, bufs=None):
    return L.rsv_distinct_segmented_merge(bufs, bufs, bufs, P, S, width, k, bufs, bufs, bufs, None)


def test_symbols_are_bound(native):
    L = native.load()
    for name in ("rsv_distinct_segmented_update", "rsv_distinct_segmented_merge"):
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert getattr(L, name).restype is C.c_int32
    assert len(L.rsv_distinct_segmented_update.argtypes) == 15
    assert len(L.rsv_distinct_segmented_merge.argtypes) == 11
    assert L.rsv_abi_version() == 1


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
def test_update_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _update(L, **args) == getattr(native, status), args


def test_update_zero_states_with_ids_is_ok(native):
    """num_states == 0 returns RSV_OK without touching a pointer (with ids, B may exceed it)."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    assert _update(L, B=3, S=0, ids=C.cast(buf, C.c_void_p)) == native.OK


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=4097), "E_UNSUPPORTED"),
    (dict(width=16), "E_UNSUPPORTED"),
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(P=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0), "OK"),
    (dict(S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=4096, width=4), "E_NULL_POINTER"),
])
def test_merge_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _merge(L, **args) == getattr(native, status), args


def test_precomputed_without_hashes_is_a_null_pointer(native):
    """Every other buffer given (never dereferenced: the check comes first), hashes NULL."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert _update(L, kind=native.HASH_PRECOMPUTED, hashes=None, bufs=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


def test_limit_is_named(native):
    L = native.load()
    assert _update(L, k=4097) == native.E_UNSUPPORTED
    assert "4096" in L.rsv_last_error().decode() and "update" in L.rsv_last_error().decode()
    assert _merge(L, k=4097) == native.E_UNSUPPORTED
    assert "4096" in L.rsv_last_error().decode() and "merge" in L.rsv_last_error().decode()
