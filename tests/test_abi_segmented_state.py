"""rsv_sample_segmented_update / rsv_sample_segmented_merge validate their arguments before any device
call (CPU only): every status below comes back with NULL pointers, in the order rsv_sample_segmented
checks its own (k, key_width, negative counts, the zero-count RSV_OK returns, NULL buffers), with the
two extra cases of rsv_distinct_segmented_update (B > S without ids, S == 0)."""
import ctypes as C

import pytest

LIMIT = 15104  # the largest k whose 64-bit winner table fits one workgroup's LDS


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _update(L, B=1, S=1, width=8, k=4, ids=None, bases=None, bufs=None):
    return L.rsv_sample_segmented_update(bufs, bufs, ids, bases, B, S, width, k, 0, 0, bufs, bufs, bufs, None)


def _merge(L, P=1, S=1, width=8, k=4, bufs=None):
    return L.rsv_sample_segmented_merge(bufs, bufs, bufs, P, S, width, k, bufs, bufs, bufs, None)


def test_symbols_are_bound(native):
    L = native.load()
    for name in ("rsv_sample_segmented_update", "rsv_sample_segmented_merge"):
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert getattr(L, name).restype is C.c_int32
    assert len(L.rsv_sample_segmented_update.argtypes) == 14
    assert len(L.rsv_sample_segmented_merge.argtypes) == 11
    assert L.rsv_abi_version() == 1


def test_limit_is_mirrored(native):
    from reservoir_amd import batch

    assert batch._SEG_SAMPLE_STATE_MAX_K == LIMIT


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=LIMIT + 1), "E_UNSUPPORTED"),
    (dict(k=LIMIT + 1, width=3), "E_UNSUPPORTED"),      # k comes before key_width
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(width=16), "E_ILLEGAL_ARGUMENT"),
    (dict(width=3, B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0, S=-1), "E_ILLEGAL_ARGUMENT"),            # negative counts come before the zero returns
    (dict(B=2, S=1), "E_ILLEGAL_ARGUMENT"),             # no ids: segment b is row b
    (dict(B=1, S=0), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0), "OK"),
    (dict(B=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT, width=4), "E_NULL_POINTER"),
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
    """With ids B may exceed S: the call gets as far as the NULL-buffer check."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    assert _update(L, B=3, S=1, ids=C.cast(buf, C.c_void_p)) == native.E_NULL_POINTER


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=LIMIT + 1), "E_UNSUPPORTED"),
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(width=16), "E_ILLEGAL_ARGUMENT"),
    (dict(P=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0), "OK"),
    (dict(S=0), "OK"),
    (dict(P=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT, width=4), "E_NULL_POINTER"),
])
def test_merge_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _merge(L, **args) == getattr(native, status), args


def test_limit_is_named(native):
    L = native.load()
    assert _update(L, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "rsv_sample_segmented_update" in msg
    assert _merge(L, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "rsv_sample_segmented_merge" in msg
