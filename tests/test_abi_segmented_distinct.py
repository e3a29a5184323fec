"""rsv_distinct_segmented validates its arguments before any device call (CPU only): every status
below comes back with NULL pointers, in the order rsv_sample_segmented checks its own."""
import pytest


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _call(L, S=1, width=8, k=4, kind=1, hashes=None, bufs=None):
    return L.rsv_distinct_segmented(bufs, hashes, bufs, S, width, k, kind, 0, 0, bufs, None, bufs, None)


def test_symbol_is_bound(native):
    assert "rsv_distinct_segmented" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), "rsv_distinct_segmented")


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


def test_precomputed_without_hashes_is_a_null_pointer(native):
    """Every other buffer given (never dereferenced: the check comes first), hashes NULL."""
    import ctypes as C

    L = native.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, kind=native.HASH_PRECOMPUTED, hashes=None, bufs=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


def test_limit_is_named(native):
    L = native.load()
    assert _call(L, k=4097) == native.E_UNSUPPORTED
    assert "4096" in L.rsv_last_error().decode()
