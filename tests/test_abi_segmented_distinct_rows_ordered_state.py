"""rsv_distinct_segmented_rows_ordered_update validates its arguments before any device call (CPU only): every
status below comes back without a device and equals rsv_distinct_segmented_rows_update's for the same bad
arguments -- k, key_width, hash_kind, counts, pointers, alignment, in that order -- and state_slots_dev, the one
parameter the set form does not have, is required by name behind the other buffers."""
import ctypes as C
import os
import re

import pytest

FN = "rsv_distinct_segmented_rows_ordered_update"
SET_FN = "rsv_distinct_segmented_rows_update"


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


@pytest.fixture(scope="module")
def buf():
    """Host memory standing in for device buffers: the checks come before any dereference."""
    return (C.c_int64 * 8)()


def _ordered(L, B=1, S=1, width=16, k=4, kind=4, rows=None, hashes=None, offsets=None, ids=None, srows=None,
             shashes=None, sslots=None, scounts=None):
    return getattr(L, FN)(rows, hashes, offsets, ids, B, S, width, k, kind, 0, 0, srows, shashes, sslots, scounts, None)


def _set(L, B=1, S=1, width=16, k=4, kind=4, rows=None, hashes=None, offsets=None, ids=None, srows=None,
         shashes=None, sslots=None, scounts=None):
    return getattr(L, SET_FN)(rows, hashes, offsets, ids, B, S, width, k, kind, 0, 0, srows, shashes, scounts, None)


def test_symbol_is_bound_and_declared(native):
    L = native.load()
    assert FN in native.EXPORTED_SYMBOLS
    assert hasattr(L, FN)
    f = getattr(L, FN)
    assert f.restype is C.c_int32
    assert len(f.argtypes) == 16
    set_types = getattr(L, SET_FN).argtypes
    assert f.argtypes == set_types[:13] + [C.c_void_p] + set_types[13:]  # state_slots_dev behind state_hashes_dev
    assert L.rsv_abi_version() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "reservoir_hip.h")).read()
    m = re.search(r"rsv_status " + FN + r"\(([^;]*)\);", header)
    assert m, "the header does not declare " + FN
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 16
    assert params[13] == "int32_t* state_slots_dev" and params[12] == "int64_t* state_hashes_dev"
    assert params[14] == "int64_t* state_counts_dev" and params[15] == "void* hip_stream"


# each case passes every check before its own and trips the later ones too (NULL buffers): the status that comes
# back shows the order, and the set form is asked the same
CASES = [
    dict(k=0, width=3, kind=9, B=-1),
    dict(k=-3),
    dict(k=2**31 - 2, width=8),  # above kMaxSize = Int.MaxValue - 2
    dict(k=4097, width=8, kind=9, B=-1),
    dict(k=4096, width=4, kind=9, B=-1),
    dict(width=8, kind=9, S=-1),
    dict(width=0),
    dict(width=12, kind=1),
    dict(width=264, kind=1),
    dict(width=-16),
    dict(kind=9, B=-1),
    dict(kind=-1),
    dict(kind=1, B=-1),  # IDENTITY
    dict(kind=2, B=-1),  # JAVA_LONG
    dict(kind=3, S=-1),  # JAVA_INT
    dict(kind=0, width=24, B=-1),  # DEFAULT is UUID.hashCode: 16 bytes only
    dict(kind=0, width=256, B=-1),
    dict(B=-1),
    dict(S=-1),
    dict(B=2, S=1),  # no ids: segment b is row b
    dict(B=1, S=0),
    dict(B=0),  # NULL buffers: nothing is touched
    dict(B=0, S=0),
    dict(B=0, kind=0, width=16, k=4096),
    dict(B=0, width=256),
    dict(),
    dict(kind=0),
    dict(k=4096, width=256),
]
STATUS = ["E_ILLEGAL_ARGUMENT"] * 3 + ["E_UNSUPPORTED"] * 3 + ["E_ILLEGAL_ARGUMENT"] * 6 + ["E_UNSUPPORTED"] * 5 + \
    ["E_ILLEGAL_ARGUMENT"] * 4 + ["OK"] * 4 + ["E_NULL_POINTER"] * 3


@pytest.mark.parametrize("args,status", list(zip(CASES, STATUS)))
def test_statuses_without_a_device_are_the_set_forms(native, args, status):
    L = native.load()
    got = _ordered(L, **args)
    assert got == getattr(native, status), args
    assert got == _set(L, **args), args


def test_zero_states_with_ids_is_ok(native, buf):
    assert _ordered(native.load(), B=3, S=0, ids=C.cast(buf, C.c_void_p)) == native.OK


@pytest.mark.parametrize("missing", ["offsets", "srows", "shashes", "sslots", "scounts"])
@pytest.mark.parametrize("kind", [0, 4])
def test_each_null_buffer(native, buf, missing, kind):
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, srows=p, shashes=p, sslots=p, scounts=p)
    bufs[missing] = None
    assert _ordered(native.load(), kind=kind, **bufs) == native.E_NULL_POINTER
    if missing != "sslots":
        assert _set(native.load(), kind=kind, **bufs) == native.E_NULL_POINTER


def test_state_slots_null_names_the_parameter_behind_the_other_buffers(native, buf):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _ordered(L, rows=p, hashes=p, offsets=p, srows=p, shashes=p, scounts=p) == native.E_NULL_POINTER
    msg = L.rsv_last_error().decode()
    assert "state_slots_dev" in msg and FN in msg
    # another NULL buffer beside it is reported first, without the name
    assert _ordered(L, rows=p, hashes=p, offsets=p, srows=p, shashes=None, scounts=p) == native.E_NULL_POINTER
    assert "state_slots_dev" not in L.rsv_last_error().decode()
    # and it comes before the precomputed hashes and the alignment
    assert _ordered(L, rows=C.c_void_p(p.value + 1), offsets=p, srows=p, shashes=p, scounts=p) == native.E_NULL_POINTER
    assert "state_slots_dev" in L.rsv_last_error().decode()


def test_precomputed_without_hashes_is_a_null_pointer(native, buf):
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    assert _ordered(L, kind=native.HASH_PRECOMPUTED, rows=p, offsets=p, srows=p, shashes=p, sslots=p,
                    scounts=p) == native.E_NULL_POINTER
    assert "hashes" in L.rsv_last_error().decode()


@pytest.mark.parametrize("which", ["rows", "srows"])
@pytest.mark.parametrize("off", [1, 4])
def test_row_buffers_must_be_8_byte_aligned(native, buf, which, off):
    """The last check: every buffer given, the input rows or the state rows off an 8-byte boundary.  A NULL buffer
    beside it wins (the pointer checks come first)."""
    L = native.load()
    p = C.cast(buf, C.c_void_p)
    bufs = dict(rows=p, hashes=p, offsets=p, srows=p, shashes=p, sslots=p, scounts=p)
    bufs[which] = C.c_void_p(p.value + off)
    assert _ordered(L, **bufs) == native.E_ILLEGAL_ARGUMENT == _set(L, **bufs)
    assert "aligned" in L.rsv_last_error().decode()
    bufs["scounts"] = None
    assert _ordered(L, **bufs) == native.E_NULL_POINTER


def test_limit_and_the_long_counterpart_are_named(native):
    L = native.load()
    assert _ordered(L, k=4097) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert "4096" in msg and FN in msg
    for width in (4, 8):
        assert _ordered(L, width=width) == native.E_UNSUPPORTED
        assert "rsv_distinct_segmented_ordered_update " in L.rsv_last_error().decode() + " "


def test_long_key_ordered_update_still_refuses_byte_keys(native):
    L = native.load()
    assert L.rsv_distinct_segmented_ordered_update(None, None, None, None, 1, 1, 16, 4, 1, 0, 0, None, None, None,
                                                   None) == native.E_UNSUPPORTED
