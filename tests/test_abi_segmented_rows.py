"""rsv_sample_segmented_rows / _rows_update / _rows_merge validate their arguments before any device call
(CPU only): every status below comes back with NULL pointers, in the order of their Long-key
counterparts (k, key_width, negative counts, the zero-count RSV_OK returns, NULL buffers).  key_width 4
or 8 is RSV_E_UNSUPPORTED and names the Long-key entry point; any other width outside the multiples of
8 in 16..256 is RSV_E_ILLEGAL_ARGUMENT."""
import ctypes as C

import pytest

LIMIT = 15104  # the resumed forms: the largest k whose 64-bit winner table fits one workgroup's LDS
KMAX = 2**31 - 3  # the stateless form: Sampler.scala's maxSampleSize limit


@pytest.fixture(scope="module")
def native():
    from reservoir_amd import _native

    return _native


def _sample(L, S=1, width=16, k=4, bufs=None):
    return L.rsv_sample_segmented_rows(bufs, bufs, S, width, k, 0, 0, bufs, bufs, None)


def _update(L, B=1, S=1, width=16, k=4, ids=None, bases=None, bufs=None):
    return L.rsv_sample_segmented_rows_update(bufs, bufs, ids, bases, B, S, width, k, 0, 0, bufs, bufs, bufs, None)


def _merge(L, P=1, S=1, width=16, k=4, bufs=None):
    return L.rsv_sample_segmented_rows_merge(bufs, bufs, bufs, P, S, width, k, bufs, bufs, bufs, None)


NAMES = ("rsv_sample_segmented_rows", "rsv_sample_segmented_rows_update", "rsv_sample_segmented_rows_merge")

# one row per width the issue names: status and, for 4 and 8, the Long-key entry point in the message
WIDTHS = [(4, "E_UNSUPPORTED"), (8, "E_UNSUPPORTED"), (12, "E_ILLEGAL_ARGUMENT"), (264, "E_ILLEGAL_ARGUMENT"),
          (0, "E_ILLEGAL_ARGUMENT")]


def test_symbols_are_bound(native):
    L = native.load()
    for name in NAMES:
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert getattr(L, name).restype is C.c_int32
    assert len(L.rsv_sample_segmented_rows.argtypes) == 10
    assert len(L.rsv_sample_segmented_rows_update.argtypes) == 14
    assert len(L.rsv_sample_segmented_rows_merge.argtypes) == 11
    assert L.rsv_abi_version() == 1


def test_limit_is_mirrored(native):
    from reservoir_amd import batch

    assert batch._SEG_SAMPLE_STATE_MAX_K == LIMIT
    assert hasattr(batch, "SegmentedSamplerRows") and hasattr(batch, "sample_segmented_rows")


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=0, width=8), "E_ILLEGAL_ARGUMENT"),         # k comes before key_width
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(width=20), "E_ILLEGAL_ARGUMENT"),
    (dict(width=-16), "E_ILLEGAL_ARGUMENT"),
    (dict(width=8, S=-1), "E_UNSUPPORTED"),             # key_width comes before the counts
    (dict(width=12, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=0), "OK"),
    (dict(S=0, width=256, k=KMAX), "OK"),               # the stateless form takes k up to kMaxSize
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT + 1), "E_NULL_POINTER"),              # no 15104 limit without state
    (dict(k=KMAX, width=24), "E_NULL_POINTER"),
    (dict(width=256), "E_NULL_POINTER"),
])
def test_sample_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _sample(L, **args) == getattr(native, status), args


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=2**31 - 1), "E_ILLEGAL_ARGUMENT"),
    (dict(k=LIMIT + 1), "E_UNSUPPORTED"),
    (dict(k=LIMIT + 1, width=3), "E_UNSUPPORTED"),      # k comes before key_width
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(width=20), "E_ILLEGAL_ARGUMENT"),
    (dict(width=8, B=-1), "E_UNSUPPORTED"),             # key_width comes before the counts
    (dict(width=3, B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0, S=-1), "E_ILLEGAL_ARGUMENT"),            # negative counts come before the zero returns
    (dict(B=2, S=1), "E_ILLEGAL_ARGUMENT"),             # no ids: segment b is row b
    (dict(B=1, S=0), "E_ILLEGAL_ARGUMENT"),
    (dict(B=0), "OK"),
    (dict(B=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT, width=256), "E_NULL_POINTER"),
    (dict(k=1, width=24), "E_NULL_POINTER"),
])
def test_update_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _update(L, **args) == getattr(native, status), args


def test_update_zero_states_with_ids_is_ok(native):
    """num_states == 0 returns RSV_OK without touching a pointer (with ids, B may exceed it)."""
    L = native.load()
    buf = (C.c_int64 * 8)()
    assert _update(L, B=3, S=0, ids=C.cast(buf, C.c_void_p)) == native.OK
    assert _update(L, B=3, S=1, ids=C.cast(buf, C.c_void_p)) == native.E_NULL_POINTER


@pytest.mark.parametrize("args,status", [
    (dict(k=0), "E_ILLEGAL_ARGUMENT"),
    (dict(k=-3), "E_ILLEGAL_ARGUMENT"),
    (dict(k=LIMIT + 1), "E_UNSUPPORTED"),
    (dict(k=LIMIT + 1, width=3), "E_UNSUPPORTED"),
    (dict(width=3), "E_ILLEGAL_ARGUMENT"),
    (dict(width=20), "E_ILLEGAL_ARGUMENT"),
    (dict(width=8, P=-1), "E_UNSUPPORTED"),
    (dict(P=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0, S=-1), "E_ILLEGAL_ARGUMENT"),
    (dict(P=0), "OK"),
    (dict(S=0), "OK"),
    (dict(P=0, S=0), "OK"),
    (dict(), "E_NULL_POINTER"),
    (dict(k=LIMIT, width=256), "E_NULL_POINTER"),
])
def test_merge_statuses_without_a_device(native, args, status):
    L = native.load()
    assert _merge(L, **args) == getattr(native, status), args


@pytest.mark.parametrize("width,status", WIDTHS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_widths(native, which, width, status):
    """Widths 4, 8, 12, 264 and 0 at each entry point; 4 and 8 name the Long-key entry point to use."""
    L = native.load()
    call = (_sample, _update, _merge)[which]
    assert call(L, width=width) == getattr(native, status), (which, width)
    if status == "E_UNSUPPORTED":
        msg = L.rsv_last_error().decode()
        long_name = NAMES[which].replace("_rows", "")
        assert NAMES[which] in msg and long_name + " " in msg, msg


@pytest.mark.parametrize("width", list(range(16, 257, 8)))
def test_every_legal_width_reaches_the_buffers(native, width):
    L = native.load()
    for call in (_sample, _update, _merge):
        assert call(L, width=width) == native.E_NULL_POINTER, width


def test_limit_is_named(native):
    L = native.load()
    assert _update(L, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "rsv_sample_segmented_rows_update" in msg
    assert _merge(L, k=LIMIT + 1) == native.E_UNSUPPORTED
    msg = L.rsv_last_error().decode()
    assert str(LIMIT) in msg and "rsv_sample_segmented_rows_merge" in msg
