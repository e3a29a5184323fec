"""rsv_distinct_segmented_ordered validates its arguments before any device call (CPU only): every status
below comes back with NULL pointers, in the order rsv_distinct_segmented checks its own; tied_dev is one
more required buffer."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _call(L, S=1, width=8, k=4, kind=1, hashes=None, bufs=None, tied=None):
    return L.rsv_distinct_segmented_ordered(bufs, hashes, bufs, S, width, k, kind, 0, 0, bufs, None, bufs, tied, None)


def test_symbol_is_bound(native):
    assert "rsv_distinct_segmented_ordered" in native.EXPORTED_SYMBOLS
    L = native.load()
    assert hasattr(L, "rsv_distinct_segmented_ordered")
    assert len(L.rsv_distinct_segmented_ordered.argtypes) == len(L.rsv_distinct_segmented.argtypes) + 1


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=4097), "E_UNSUPPORTED"),
    (dict(width=16), "E_UNSUPPORTED"),
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=9), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=4096, width=4, kind=0), "E_NULL_POINTER"),
    (dict(kind=4), "E_NULL_POINTER"),
])
def test_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _call(L, **args) == getattr(native, status), args


def test_null_tied_is_a_null_pointer(native):
    """Every other buffer given (never dereferenced: the check comes first), tied_dev NULL."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, bufs=p, tied=None) == native.E_NULL_POINTER
    assert "tied_dev" in L.rsv_last_error().decode()


def test_precomputed_without_hashes_is_a_null_pointer(native):
    L = native.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, kind=native.HASH_PRECOMPUTED, hashes=None, bufs=p, tied=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


def test_limit_and_byte_keys_name_the_entry_point(native):
    L = native.load()
    assert _call(L, k=4097) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert "4096" in msg and "rsv_distinct_segmented_ordered" in msg
    assert _call(L, width=16) == native.E_UNSUPPORTED
    assert "rsv_distinct_segmented_ordered" in L.rsv_last_error().decode()


def test_abi_version_is_unchanged(native):
    assert native.load().rsv_abi_version() == 1
