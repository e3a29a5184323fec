"""rsv_group_by_stream, rsv_sample_segmented_update_indirect and rsv_sample_segmented_rows_update_indirect are bound
with their documented argument lists and validate their arguments before any device call (CPU only).  The grouping
pass checks, in this order: offsets_dev, order_dev and ids_dev (the last two only with n > 0) for NULL, n and
num_states, id_width, then the limit on n; each message names the parameter or the limit.  The indirect updates return
the statuses of the direct ones, plus RSV_E_NULL_POINTER for a NULL order_dev.  (n = 0 -> RSV_OK writes the offsets,
which takes a device: tests/test_gpu_group_by_stream.py.)"""
import ctypes as C

import pytest

LIMIT = 15104  # the resumed forms: the largest k whose 64-bit winner table fits one workgroup's LDS
NMAX = 2**31 - 1


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


@pytest.fixture(scope="module")
def buf():
    """A host buffer's address: a non-NULL pointer for calls that fail before any pointer is used."""
    mem = (C.c_int64 * 8)()
    return C.cast(mem, C.c_void_p), mem


def _group(L, ids=None, width=8, n=1, S=1, offsets=None, order=None):
    return L.rsv_group_by_stream(ids, width, n, S, offsets, order, None)


def _indirect(L, rows=False, n=1, order=None, B=1, S=1, width=None, k=4, bufs=None):
    fn = L.rsv_sample_segmented_rows_update_indirect if rows else L.rsv_sample_segmented_update_indirect
    width = (16 if rows else 8) if width is None else width
    return fn(bufs, n, order, bufs, None, None, B, S, width, k, 0, 0, bufs, bufs, bufs, None)


def _direct(L, rows=False, B=1, S=1, width=None, k=4, bufs=None):
    fn = L.rsv_sample_segmented_rows_update if rows else L.rsv_sample_segmented_update
    width = (16 if rows else 8) if width is None else width
    return fn(bufs, bufs, None, None, B, S, width, k, 0, 0, bufs, bufs, bufs, None)


def test_symbols_are_bound(native):
    L = native.load()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    for name in ("rsv_group_by_stream", "rsv_sample_segmented_update_indirect",
                 "rsv_sample_segmented_rows_update_indirect"):
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert getattr(L, name).restype is i32
    assert L.rsv_group_by_stream.argtypes == [vp, i32, i64, i64, vp, vp, vp]
    indirect = [vp, i64, vp, vp, vp, vp, i64, i64, i32, i32, u64, u64, vp, vp, vp, vp]
    assert L.rsv_sample_segmented_update_indirect.argtypes == indirect
    assert L.rsv_sample_segmented_rows_update_indirect.argtypes == indirect
    assert L.rsv_abi_version() == 1


def test_python_surface_exists():
    from reservoir_amd import batch

    assert callable(batch.group_by_stream)
    for cls in (batch.SegmentedSampler, batch.SegmentedSamplerRows, batch.SegmentedDistinct,
                batch.SegmentedDistinctOrdered, batch.SegmentedDistinctRows, batch.SegmentedDistinctRowsOrdered):
        assert callable(getattr(cls, "update_by_id"))


def test_group_statuses_in_order(native, buf):
    """Every status of the issue, each with everything that a later check would reject also wrong."""
    L = native.load()
    p, _ = buf
    E = native

    def msg():
        return L.rsv_last_error().decode()

    # NULL offsets_dev first, whatever else is wrong
    assert _group(L, ids=None, width=3, n=-1, S=0, offsets=None, order=None) == E.E_NULL_POINTER
    assert "offsets_dev" in msg()
    # then order_dev, then ids_dev, with n > 0 only
    assert _group(L, ids=None, width=3, n=NMAX + 1, S=0, offsets=p, order=None) == E.E_NULL_POINTER
    assert "order_dev" in msg()
    assert _group(L, ids=None, width=3, n=NMAX + 1, S=0, offsets=p, order=p) == E.E_NULL_POINTER
    assert "ids_dev" in msg()
    # n < 0 and num_states < 1 (NULL order_dev / ids_dev are fine without elements)
    assert _group(L, width=3, n=-1, S=0, offsets=p) == E.E_ILLEGAL_ARGUMENT
    assert "negative n" in msg()
    assert _group(L, width=3, n=-1, S=5, offsets=p) == E.E_ILLEGAL_ARGUMENT
    assert _group(L, width=3, n=0, S=0, offsets=p) == E.E_ILLEGAL_ARGUMENT
    assert "num_states" in msg()
    assert _group(L, ids=p, width=3, n=NMAX + 1, S=-4, offsets=p, order=p) == E.E_ILLEGAL_ARGUMENT
    assert "num_states" in msg()
    # id_width, before the limit on n and before the n == 0 return
    for w in (0, 3, 2, 16, -8):
        assert _group(L, ids=p, width=w, n=NMAX + 1, S=1, offsets=p, order=p) == E.E_UNSUPPORTED, w
        assert "id_width" in msg()
        assert _group(L, width=w, n=0, S=1, offsets=p) == E.E_UNSUPPORTED, w
        assert "id_width" in msg()
    # the limit on n, named
    for w in (4, 8):
        assert _group(L, ids=p, width=w, n=NMAX + 1, S=1, offsets=p, order=p) == E.E_UNSUPPORTED
        assert "2147483647" in msg() and "id_width" not in msg()
        assert _group(L, ids=p, width=w, n=2**40, S=1, offsets=p, order=p) == E.E_UNSUPPORTED
        assert "2147483647" in msg()


@pytest.mark.parametrize("rows", [False, True])
def test_indirect_statuses_are_the_direct_ones(native, buf, rows):
    L = native.load()
    p, _ = buf
    cases = [dict(k=0), dict(k=LIMIT + 1), dict(width=3), dict(k=0, width=3), dict(k=LIMIT + 1, width=3),
             dict(B=-1), dict(S=-1), dict(B=2, S=1), dict(B=0), dict(B=0, S=0), dict(), dict(k=LIMIT),
             dict(width=4 if not rows else 24)]
    if rows:
        cases += [dict(width=8), dict(width=4), dict(width=20), dict(width=264)]
    for args in cases:
        want = _direct(L, rows=rows, **args)
        assert _indirect(L, rows=rows, order=p, **args) == want, args
    # the statuses the issue names, spelled out
    assert _indirect(L, rows=rows, order=p, k=0) == native.E_ILLEGAL_ARGUMENT
    assert _indirect(L, rows=rows, order=p, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "_update_indirect" in msg
    assert _indirect(L, rows=rows, order=p, width=3) == native.E_ILLEGAL_ARGUMENT
    assert _indirect(L, rows=rows, order=p) == native.E_NULL_POINTER  # the other buffers


def test_rows_indirect_rejects_width_8(native, buf):
    L = native.load()
    p, _ = buf
    assert _indirect(L, rows=True, order=p, width=8) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert "rsv_sample_segmented_rows_update_indirect" in msg and "rsv_sample_segmented_update_indirect " in msg


@pytest.mark.parametrize("rows", [False, True])
def test_indirect_null_order(native, buf, rows):
    """order_dev NULL with every other buffer present: RSV_E_NULL_POINTER naming it; nothing is launched."""
    L = native.load()
    p, _ = buf
    assert _indirect(L, rows=rows, order=None, bufs=p) == native.E_NULL_POINTER
    assert "order_dev" in L.rsv_last_error().decode()
    assert _indirect(L, rows=rows, order=None, bufs=p, B=0) == native.OK  # nothing to do comes first, as in the direct call
    assert _indirect(L, rows=rows, order=p, bufs=p, n=-1) == native.E_ILLEGAL_ARGUMENT
