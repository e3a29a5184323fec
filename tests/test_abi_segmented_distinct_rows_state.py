"""rsv_distinct_segmented_rows_update / rsv_distinct_segmented_rows_merge validate their arguments before
any device call (CPU only): every status below comes back without a device, in
rsv_distinct_segmented_rows' order -- k, key_width, hash_kind (the update), counts, pointers -- and the
alignment of the row buffers last.  The entry points for 4- and 8-byte keys keep refusing byte keys."""
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


def _update(L, B=1, S=1, width=16, k=4, kind=4, rows=None, hashes=None, offsets=None, ids=None, srows=None,
            shashes=None, scounts=None):
    return L.rsv_distinct_segmented_rows_update(rows, hashes, offsets, ids, B, S, width, k, kind, 0, 0, srows, shashes,
                                                scounts, None)


def _merge(L, P=1, S=1, width=16, k=4, prows=None, phashes=None, pcounts=None, srows=None, shashes=None,
           scounts=None):
    return L.rsv_distinct_segmented_rows_merge(prows, phashes, pcounts, P, S, width, k, srows, shashes, scounts, None)


def test_symbols_are_bound(native):
    L = native.load()
    for name in ("rsv_distinct_segmented_rows_update", "rsv_distinct_segmented_rows_merge"):
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert getattr(L, name).restype is C.c_int32
    assert len(L.rsv_distinct_segmented_rows_update.argtypes) == 15
    assert len(L.rsv_distinct_segmented_rows_merge.argtypes) == 11
    assert L.rsv_abi_version() == 1


# each case passes every check before its own and trips the later ones too (NULL buffers): the
# status that comes back shows the order
@pytest.mark.parametrize("args,status", [
    (dict(k=0, width=3, kind=9, B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 2, width=8), "E_ILLEGAL_ARGUMENT"),  # above kMaxSize = Int.MaxValue - 2
    (dict(k=4097, width=8, kind=9, B=-1), "E_UNSUPPORTED"),
    (dict(k=4096, width=4, kind=9, B=-1), "E_UNSUPPORTED"),
    (dict(width=8, kind=9, S=-1), "E_UNSUPPORTED"),
    (dict(width=0), "E_ILLEGAL_ARGUMENT"),
    (dict(width=12, kind=1), "E_ILLEGAL_ARGUMENT"),
    (dict(width=264, kind=1), "E_ILLEGAL_ARGUMENT"),
    (dict(width=-16), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=9, B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(kind=1, B=-1), "E_UNSUPPORTED"),  # IDENTITY
    (dict(kind=2, B=-1), "E_UNSUPPORTED"),  # JAVA_LONG
    (dict(kind=3, S=-1), "E_UNSUPPORTED"),  # JAVA_INT
    (dict(kind=0, width=24, B=-1), "E_UNSUPPORTED"),  # DEFAULT is UUID.hashCode: 16 bytes only
    (dict(kind=0, width=256, B=-1), "E_UNSUPPORTED"),
    (dict(B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=2, S=1), "E_ILLEGAL_ARGUMENT"),  # no ids: segment b is row b
    (dict(B=1, S=0), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0), "OK"),  # NULL buffers: nothing is touched
    (dict(B=0, S=0), "OK"),
    (dict(B=0, kind=0, width=16, k=4096), "OK"),
    (dict(B=0, width=256), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(kind=0), "E_NULL_POINTER"),
    (dict(k=4096, width=256), "E_NULL_POINTER"),
])
def test_update_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _update(L, **args) == getattr(native, status), args


def test_update_zero_states_with_ids_is_ok(native, buf):
    """num_states == 0 returns RSV_OK without touching a pointer (with ids, B may exceed it)."""
    assert _update(native.load(), B=3, S=0, ids=C.cast(buf, C.c_void_p)) == native.OK


@pytest.mark.parametrize("args,status", [
    (dict(k=0, width=3, P=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=4097, width=8, P=-1), "E_UNSUPPORTED"),
    (dict(width=4, P=-1), "E_UNSUPPORTED"),
    (dict(width=8, S=-1), "E_UNSUPPORTED"),
    (dict(width=12), "E_ILLEGAL_ARGUMENT"),
    (dict(width=264), "E_ILLEGAL_ARGUMENT"),
    (dict(P=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0), "OK"),
    (dict(S=0), "OK"),
    (dict(P=0, width=256, k=4096), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=4096, width=24), "E_NULL_POINTER"),
])
def test_merge_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _merge(L, **args) == getattr(native, status), args


@pytest.mark.parametrize("missing", ["offsets", "srows", "shashes", "scounts"])
@pytest.mark.parametrize("kind", [0, 4])
def test_update_each_null_buffer(native, buf, missing, kind):
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, srows=p, shashes=p, scounts=p)
    bufs[missing] = None
    assert _update(native.load(), kind=kind, **bufs) == native.E_NULL_POINTER


@pytest.mark.parametrize("missing", ["prows", "phashes", "pcounts", "srows", "shashes", "scounts"])
def test_merge_each_null_buffer(native, buf, missing):
    p = C.cast(buf, C.c_void_p)
    bufs = dict(prows=p, phashes=p, pcounts=p, srows=p, shashes=p, scounts=p)
    bufs[missing] = None
    assert _merge(native.load(), **bufs) == native.E_NULL_POINTER


def test_precomputed_without_hashes_is_a_null_pointer(native, buf):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _update(L, kind=native.HASH_PRECOMPUTED, rows=p, offsets=p, srows=p, shashes=p,
                   scounts=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


@pytest.mark.parametrize("which", ["rows", "srows"])
@pytest.mark.parametrize("off", [1, 4])
def test_update_row_buffers_must_be_8_byte_aligned(native, buf, which, off):
    """The last check: every buffer given, the input rows or the state rows off an 8-byte boundary.  A
    NULL buffer beside it wins (the pointer checks come first)."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, srows=p, shashes=p, scounts=p)
    bufs[which] = C.c_void_p(p.value + off)
    assert _update(L, **bufs) == native.E_ILLEGAL_ARGUMENT
    assert "aligned" in L.rsv_last_error().decode()
    bufs["scounts"] = None
    assert _update(L, **bufs) == native.E_NULL_POINTER


@pytest.mark.parametrize("which", ["prows", "srows"])
@pytest.mark.parametrize("off", [1, 4])
def test_merge_row_buffers_must_be_8_byte_aligned(native, buf, which, off):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(prows=p, phashes=p, pcounts=p, srows=p, shashes=p, scounts=p)
    bufs[which] = C.c_void_p(p.value + off)
    assert _merge(L, **bufs) == native.E_ILLEGAL_ARGUMENT
    assert "aligned" in L.rsv_last_error().decode()
    bufs["scounts"] = None
    assert _merge(L, **bufs) == native.E_NULL_POINTER


def test_limit_and_the_other_entry_points_are_named(native):
    L = native.load()
    assert _update(L, k=4097) == native.E_UNSUPPORTED
    assert "4096" in L.rsv_last_error().decode() and "rows_update" in L.rsv_last_error().decode()
    assert _merge(L, k=4097) == native.E_UNSUPPORTED
    assert "4096" in L.rsv_last_error().decode() and "rows_merge" in L.rsv_last_error().decode()
    for width in (4, 8):
        assert _update(L, width=width) == native.E_UNSUPPORTED
        assert "rsv_distinct_segmented_update " in L.rsv_last_error().decode() + " "
        assert _merge(L, width=width) == native.E_UNSUPPORTED
        assert "rsv_distinct_segmented_merge " in L.rsv_last_error().decode() + " "


def test_long_key_entry_points_still_refuse_byte_keys(native):
    """rsv_distinct_segmented_update / _merge at width 16: E_UNSUPPORTED as before, with NULL buffers."""
    L = native.load()
    assert L.rsv_distinct_segmented_update(None, None, None, None, 1, 1, 16, 4, 1, 0, 0, None, None, None,
                                           None) == native.E_UNSUPPORTED
    assert L.rsv_distinct_segmented_merge(None, None, None, 1, 1, 16, 4, None, None, None, None) == native.E_UNSUPPORTED
