"""rsv_distinct_segmented_rows validates its arguments before any device call (CPU only): every status
below comes back without a device, in rsv_distinct_segmented's order -- k, key_width, hash_kind,
num_streams, pointers -- and the alignment of the two row buffers last."""
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


def _call(L, S=1, width=16, k=4, kind=4, rows=None, hashes=None, offsets=None, out=None, counts=None):
    return L.rsv_distinct_segmented_rows(rows, hashes, offsets, S, width, k, kind, 0, 0, out, None, counts, None)


def test_symbol_is_bound(native):
    assert "rsv_distinct_segmented_rows" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), "rsv_distinct_segmented_rows")


# each case passes every check before its own and trips the later ones too (NULL buffers): the
# status that comes back shows the order
@pytest.mark.parametrize("args,status", [
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
    (dict(S=0), "OK"),  # NULL buffers: nothing is touched
    (dict(S=0, kind=0, width=16, k=4096), "OK"),
    (dict(S=0, width=256), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(kind=0), "E_NULL_POINTER"),
])
def test_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _call(L, **args) == getattr(native, status), args


@pytest.mark.parametrize("missing", ["offsets", "out", "counts"])
@pytest.mark.parametrize("kind", [0, 4])
def test_each_null_buffer(native, buf, missing, kind):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, out=p, counts=p)
    bufs[missing] = None
    assert _call(L, kind=kind, **bufs) == native.E_NULL_POINTER


def test_precomputed_without_hashes_is_a_null_pointer(native, buf):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, kind=native.HASH_PRECOMPUTED, rows=p, offsets=p, out=p, counts=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


@pytest.mark.parametrize("which", ["rows", "out"])
@pytest.mark.parametrize("off", [1, 4])
def test_row_buffers_must_be_8_byte_aligned(native, buf, which, off):
    """The last check: every buffer given, one of the two row buffers off an 8-byte boundary.  A NULL
    buffer beside it wins (the pointer checks come first)."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, out=p, counts=p)
    bufs[which] = C.c_void_p(p.value + off)
    assert _call(L, **bufs) == native.E_ILLEGAL_ARGUMENT
    assert "aligned" in L.rsv_last_error().decode()
    bufs["counts"] = None
    assert _call(L, **bufs) == native.E_NULL_POINTER


def test_limit_and_the_other_entry_point_are_named(native):
    L = native.load()
    assert _call(L, k=4097) == native.E_UNSUPPORTED
    assert "4096" in L.rsv_last_error().decode()
    for width in (4, 8):
        assert _call(L, width=width) == native.E_UNSUPPORTED
        assert "rsv_distinct_segmented " in L.rsv_last_error().decode() + " "
