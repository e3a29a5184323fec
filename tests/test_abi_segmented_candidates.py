"""rsv_distinct_segmented_candidates validates its arguments before any device call (CPU only): every status
below comes back without a device, in K5's order -- k, the k limit, the counts and cap, nothing to do, the
pointers, set_sizes / max_hashes together."""
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


def _call(L, B=1, S=1, k=4, cap=8, hashes=None, offsets=None, ids=None, sh=None, sc=None, sizes=None, maxh=None,
          pos=None, hs=None, counts=None):
    return L.rsv_distinct_segmented_candidates(hashes, offsets, ids, B, S, k, 0, 0, sh, sc, sizes, maxh, pos, hs, cap,
                                               counts, None)


def test_symbol_is_bound(native):
    L = native.load()
    name = "rsv_distinct_segmented_candidates"
    assert name in native.EXPORTED_SYMBOLS
    assert hasattr(L, name)
    assert getattr(L, name).restype is C.c_int32
    assert len(L.rsv_distinct_segmented_candidates.argtypes) == 17
    assert L.rsv_abi_version() == 1


# each case passes every check before its own and trips the later ones too (NULL buffers, one of the two
# bound tensors): the status that comes back shows the order
@pytest.mark.parametrize("args,status", [
    (dict(k=0, B=-1, cap=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 2), "E_ILLEGAL_ARGUMENT"),  # above kMaxSize = Int.MaxValue - 2
    (dict(k=4097, B=-1, cap=0), "E_UNSUPPORTED"),
    (dict(k=4097, S=-1), "E_UNSUPPORTED"),
    (dict(B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(cap=0), "E_ILLEGAL_ARGUMENT"),
    (dict(cap=-9, B=0), "E_ILLEGAL_ARGUMENT"),  # before "nothing to do"
    (dict(B=2, S=1), "E_ILLEGAL_ARGUMENT"),  # no ids: segment b is row b
    (dict(B=1, S=0), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0), "OK"),  # NULL buffers: nothing is touched
    (dict(B=0, S=0), "OK"),
    (dict(B=0, k=4096, cap=1), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=4096), "E_NULL_POINTER"),
    (dict(k=1, cap=1), "E_NULL_POINTER"),
])
def test_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _call(L, **args) == getattr(native, status), args


def test_null_buffers_come_before_the_bound_pair(native, buf):
    """One of set_sizes / max_hashes with NULL buffers beside it: the pointer check fires first."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _call(L, sizes=p) == native.E_NULL_POINTER
    assert _call(L, maxh=p) == native.E_NULL_POINTER


@pytest.mark.parametrize("missing", ["offsets", "sh", "sc", "pos", "hs", "counts"])
def test_each_null_buffer(native, buf, missing):
    p = C.cast(buf, C.c_void_p)
    bufs = dict(hashes=p, offsets=p, sh=p, sc=p, pos=p, hs=p, counts=p)
    bufs[missing] = None
    assert _call(native.load(), **bufs) == native.E_NULL_POINTER


@pytest.mark.parametrize("given", ["sizes", "maxh"])
def test_exactly_one_of_the_bound_pair_is_illegal(native, buf, given):
    """The last check: every buffer given, and one of set_sizes_dev / max_hashes_dev without the other."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(hashes=p, offsets=p, sh=p, sc=p, pos=p, hs=p, counts=p)
    bufs[given] = p
    assert _call(L, **bufs) == native.E_ILLEGAL_ARGUMENT
    err = L.rsv_last_error().decode()
    assert "set_sizes_dev" in err and "max_hashes_dev" in err


def test_limit_names_the_entry_point(native):
    L = native.load()
    assert _call(L, k=4097) == native.E_UNSUPPORTED
    err = L.rsv_last_error().decode()
    assert "4096" in err and "rsv_distinct_segmented_candidates" in err
