"""rsv_distinct_segmented_rows_ordered validates its arguments before any device call (CPU only): every
status tests/test_abi_segmented_distinct_rows.py pins for rsv_distinct_segmented_rows comes back the same
here, in the same order -- k, key_width, hash_kind, num_streams, pointers, alignment -- and tied_dev is one
more required buffer."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


@pytest.fixture(scope="module")
def buf():
    """Host memory standing in for device buffers: the checks come before any dereference."""
    return (C.c_int64 * 8)()


def _call(L, S=1, width=16, k=4, kind=4, rows=None, hashes=None, offsets=None, out=None, counts=None, tied=None):
    return L.rsv_distinct_segmented_rows_ordered(rows, hashes, offsets, S, width, k, kind, 0, 0, out, None, counts,
                                                 tied, None)


def _set_call(L, S=1, width=16, k=4, kind=4, rows=None, hashes=None, offsets=None, out=None, counts=None):
    return L.rsv_distinct_segmented_rows(rows, hashes, offsets, S, width, k, kind, 0, 0, out, None, counts, None)


def test_symbol_is_bound(native):
    assert "rsv_distinct_segmented_rows_ordered" in native.EXPORTED_SYMBOLS
    L = native.load()
    assert hasattr(L, "rsv_distinct_segmented_rows_ordered")
    assert L.rsv_distinct_segmented_rows_ordered.argtypes == L.rsv_distinct_segmented_rows.argtypes + [C.c_void_p]
    assert L.rsv_distinct_segmented_rows_ordered.restype is C.c_int32


# the set call's table: each case passes every check before its own and trips the later ones too (NULL
# buffers, tied_dev among them), so the status that comes back shows the order
_STATUSES = [
    (dict(k=0, width=3, kind=9, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 2, width=8), "E_ILLEGAL_ARGUMENT"),  # above kMaxSize = Int.MaxValue - 2
    (dict(k=4097, width=8, kind=9, S=-1), "E_UNSUPPORTED"),
    (dict(k=4096, width=4, kind=9, S=-1), "E_UNSUPPORTED"),
    (dict(width=8, kind=9, S=-1), "E_UNSUPPORTED"),
    (dict(width=0), "E_ILLEGAL_ARGUMENT"),
    (dict(width=12), "E_ILLEGAL_ARGUMENT"),
    (dict(width=20, kind=1), "E_ILLEGAL_ARGUMENT"),
    (dict(width=264, kind=1), "E_ILLEGAL_ARGUMENT"),
    (dict(width=-16), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=9, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=5, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=1, S=-1), "E_UNSUPPORTED"),  # IDENTITY
    (dict(kind=2, S=-1), "E_UNSUPPORTED"),  # JAVA_LONG
    (dict(kind=3, S=-1), "E_UNSUPPORTED"),  # JAVA_INT
    (dict(kind=0, width=24, S=-1), "E_UNSUPPORTED"),  # DEFAULT is UUID.hashCode: 16 bytes only
    (dict(kind=0, width=256, S=-1), "E_UNSUPPORTED"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=0, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=0), "OK"),  # NULL buffers, tied_dev too: nothing is touched
    (dict(S=0, kind=0, width=16, k=4096), "OK"),
    (dict(S=0, width=256), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(kind=0), "E_NULL_POINTER"),
]


@pytest.mark.parametrize("args,status", _STATUSES)
def test_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _call(L, **args) == getattr(native, status), args
    assert _set_call(L, **args) == getattr(native, status), args  # the table is the set call's


@pytest.mark.parametrize("missing", ["offsets", "out", "counts", "tied"])
@pytest.mark.parametrize("kind", [0, 4])
def test_each_null_buffer(native, buf, missing, kind):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, out=p, counts=p, tied=p)
    bufs[missing] = None
    assert _call(L, kind=kind, **bufs) == native.E_NULL_POINTER


def test_null_tied_names_the_entry_point(native, buf):
    """Every other buffer given (never dereferenced: the check comes first), tied_dev NULL."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, rows=p, hashes=p, offsets=p, out=p, counts=p, tied=None) == native.E_NULL_POINTER
    msg = L.rsv_last_error().decode()
    assert "rsv_distinct_segmented_rows_ordered" in msg and "tied_dev" in msg


def test_precomputed_without_hashes_is_a_null_pointer(native, buf):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, kind=native.HASH_PRECOMPUTED, rows=p, offsets=p, out=p, counts=p, tied=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


@pytest.mark.parametrize("which", ["rows", "out"])
@pytest.mark.parametrize("off", [1, 4])
def test_row_buffers_must_be_8_byte_aligned(native, buf, which, off):
    """The last check, as in the set call: a NULL buffer beside the misaligned one wins, tied_dev included."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, out=p, counts=p, tied=p)
    bufs[which] = C.c_void_p(p.value + off)
    assert _call(L, **bufs) == native.E_ILLEGAL_ARGUMENT
    assert "aligned" in L.rsv_last_error().decode()
    assert _call(L, **dict(bufs, tied=None)) == native.E_NULL_POINTER
    assert _call(L, **dict(bufs, counts=None)) == native.E_NULL_POINTER


def test_limit_and_the_other_entry_point_are_named(native):
    L = native.load()
    assert _call(L, k=4097) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert "4096" in msg and "rsv_distinct_segmented_rows_ordered" in msg
    for width in (4, 8):
        assert _call(L, width=width) == native.E_UNSUPPORTED
        assert "rsv_distinct_segmented_ordered " in L.rsv_last_error().decode() + " "


def test_abi_version_is_unchanged(native):
    assert native.load().rsv_abi_version() == 1
