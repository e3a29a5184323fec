"""Stateless batch entry points of the HIP engine over device tensors.

torch is used only for device memory and streams (plumbing); the compute runs in
libreservoir_hip.so.  Every function raises if the engine is unavailable.

    sample_segmented  -- K2: S independent samplers in one launch (one wave per stream)
    distinct_segmented -- K5: S independent Sampler.distinct streams in one launch (bottom-k per stream)
    distinct_segmented_rows -- K5 over fixed-width byte keys (UUIDs): rows in, the winning rows out
    SegmentedDistinct -- K5 resumed: the same S streams as caller-held state, advanced by one launch
                         per micro-batch (update) and combined across launches, GPUs and ranks (merge)
    SegmentedDistinctRows -- K5 resumed over byte keys: the rows move inside the caller-held state (update, merge)
    SegmentedSampler  -- K2 resumed: S Sampler.apply streams as caller-held state (keys, idx, next), fed in
                         pieces from any start index (update) and combined per slot by largest index (merge)
    sample_segmented_rows -- K2 over fixed-width byte keys (UUIDs): rows in, each slot's winning row out
    SegmentedSamplerRows -- K2 resumed over byte keys: state (rows, idx, next), update and merge as SegmentedSampler
    replay_events     -- K1': apply the reference's Algorithm-L eviction events on the GPU
    export_draws      -- the per-element draw sequence j_i of draw format R2
"""
from __future__ import annotations

import ctypes as C

from . import _native as N


def _stream_ptr(torch, device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def sample_segmented(keys, offsets, k: int, seed: int, stream_base: int = 0):
    """Sample each of S streams keys[offsets[s]:offsets[s+1]] independently (Algorithm R).

    Returns (out[S, k], counts[S]) device tensors; stream s is bit-identical to a single
    "philox_r" Sampler with stream_id = stream_base + s fed the same keys.
    """
    import torch

    L = N.load()
    if not (keys.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("keys and offsets must be device tensors")
    if keys.dtype not in (torch.int64, torch.int32) or offsets.dtype != torch.int64:
        raise N.IllegalArgumentException("keys must be int64/int32 and offsets int64")
    keys = keys.contiguous()
    offsets = offsets.contiguous()
    S = offsets.numel() - 1
    # the kernel writes every slot (empty ones as 0) and every count: no zero-fill (at C3's shape
    # torch.zeros was a 512 MB memset beside the 1.7 ms launch)
    out = torch.empty((max(S, 0), k), dtype=keys.dtype, device=keys.device)
    counts = torch.empty(max(S, 0), dtype=torch.int64, device=keys.device)
    if S <= 0:
        return out, counts
    N.check(L.rsv_sample_segmented(
        C.c_void_p(keys.data_ptr()), C.c_void_p(offsets.data_ptr()), S, keys.element_size(), k,
        seed & (2**64 - 1), stream_base & (2**64 - 1), C.c_void_p(out.data_ptr()),
        C.c_void_p(counts.data_ptr()), _stream_ptr(torch, keys.device)))
    return out, counts


_SEG_HASH = {"default": N.HASH_DEFAULT, "identity": N.HASH_IDENTITY, "java_long": N.HASH_JAVA_LONG,
             "java_int": N.HASH_JAVA_INT}
_SEG_DISTINCT_MAX_K = 4096  # rsv_internal.h kSegDistinctMaxK


def _segd_inputs(torch, keys, offsets, hashes, state=None):
    """keys / offsets / hashes of a K5 call, checked and contiguous (state: the SegmentedDistinct they feed)."""
    if not (keys.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("keys and offsets must be device tensors")
    if state is None:
        if keys.dtype not in (torch.int64, torch.int32) or offsets.dtype != torch.int64:
            raise N.IllegalArgumentException("keys must be int64/int32 and offsets int64")
    else:
        if keys.dtype != state.keys.dtype or offsets.dtype != torch.int64:
            raise N.IllegalArgumentException("keys must have the state's dtype and offsets must be int64")
        if keys.device != state.keys.device or offsets.device != state.keys.device:
            raise N.IllegalArgumentException("keys and offsets must live on the state's device")
        if state._kind == N.HASH_PRECOMPUTED:
            if hashes is None:
                raise N.NullPointerException("hash='precomputed' needs hashes=")
        elif hashes is not None:
            raise N.IllegalArgumentException("hashes= needs hash='precomputed'")
    if hashes is not None:
        if not hashes.is_cuda or hashes.dtype != torch.int64 or hashes.numel() != keys.numel():
            raise N.IllegalArgumentException("hashes must be an int64 device tensor, one per key")
        # an empty tensor has no address; the engine wants one for precomputed hashes
        hashes = hashes.contiguous() if hashes.numel() else torch.empty(1, dtype=torch.int64, device=keys.device)
    return keys.contiguous(), offsets.contiguous(), hashes


def _check_stream_ids(torch, stream_ids, S: int) -> None:
    """The row ids of one update: inside [0, S) and distinct, verified on the device (one host wait)."""
    if S <= 0:
        return
    B = stream_ids.numel()
    outside = (stream_ids < 0) | (stream_ids >= S)
    seen = torch.zeros(S, dtype=torch.int32, device=stream_ids.device)
    seen.index_add_(0, stream_ids.clamp(0, S - 1), torch.ones(B, dtype=torch.int32, device=stream_ids.device))
    bad = torch.stack([outside.any(), (seen > 1).any()]).cpu()  # the one host wait
    if bool(bad[0]):
        raise N.IllegalArgumentException(f"stream_ids outside [0, {S})")
    if bool(bad[1]):
        raise N.IllegalArgumentException("stream_ids repeat a row within one update")


def distinct_segmented(keys, offsets, k: int, seed: int, stream_base: int = 0, hash: str = "default", hashes=None):
    """Distinct-sample each of S streams keys[offsets[s]:offsets[s+1]] independently (bottom-k).

    Returns (out_keys[S, k], out_hashes[S, k], counts[S]) device tensors.  Stream s holds the
    min(k, distinct) keys with the smallest (scrambled hash, key), ascending, slots beyond counts[s]
    zero: what a single Sampler.distinct(k, seed=seed + stream_base + s, order="set") fed the same
    keys holds.  hash: "default" | "identity" | "java_long" | "java_int"; hashes= (one int64 per
    key, a device tensor) means precomputed hashes.  1 <= k <= 4096.
    """
    import torch

    L = N.load()
    keys, offsets, hashes = _segd_inputs(torch, keys, offsets, hashes)
    if hashes is not None:
        kind = N.HASH_PRECOMPUTED
    elif hash in _SEG_HASH:
        kind = _SEG_HASH[hash]
    else:
        raise N.IllegalArgumentException(f"unknown hash {hash!r}")
    S = offsets.numel() - 1
    # the kernel writes every slot (empty ones as 0) and every count: no zero-fill
    kk = max(int(k), 0)
    out = torch.empty((max(S, 0), kk), dtype=keys.dtype, device=keys.device)
    out_h = torch.empty((max(S, 0), kk), dtype=torch.int64, device=keys.device)
    counts = torch.empty(max(S, 0), dtype=torch.int64, device=keys.device)
    if S <= 0:
        return out, out_h, counts
    N.check(L.rsv_distinct_segmented(
        C.c_void_p(keys.data_ptr()), C.c_void_p(hashes.data_ptr()) if hashes is not None else None,
        C.c_void_p(offsets.data_ptr()), S, keys.element_size(), k, kind, seed & (2**64 - 1),
        stream_base & (2**64 - 1), C.c_void_p(out.data_ptr()), C.c_void_p(out_h.data_ptr()),
        C.c_void_p(counts.data_ptr()), _stream_ptr(torch, keys.device)))
    return out, out_h, counts


def _segd_rows_inputs(torch, rows, offsets, hash, hashes):
    """rows / offsets / hashes of a K5 call over byte keys, checked and contiguous."""
    if not (rows.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("rows and offsets must be device tensors")
    if rows.dim() != 2 or offsets.dtype != torch.int64:
        raise N.IllegalArgumentException("rows must be 2-D (one key per row) and offsets int64")
    if hashes is None and hash == "precomputed":
        raise N.NullPointerException("hash='precomputed' needs hashes=")
    if hashes is None and hash != "default":
        raise N.IllegalArgumentException(f"unknown hash {hash!r}")
    if hashes is not None:
        if not hashes.is_cuda or hashes.dtype != torch.int64 or hashes.numel() != rows.shape[0]:
            raise N.IllegalArgumentException("hashes must be an int64 device tensor, one per row")
        # an empty tensor has no address; the engine wants one for precomputed hashes
        hashes = hashes.contiguous() if hashes.numel() else torch.empty(1, dtype=torch.int64, device=rows.device)
    return rows.contiguous(), offsets.contiguous(), hashes


def distinct_segmented_rows(rows, offsets, k: int, seed: int, stream_base: int = 0, hash: str = "default", hashes=None):
    """distinct_segmented over fixed-width byte keys (java.util.UUID, case classes of primitives).

    rows: a contiguous 2-D device tensor whose rows hold W bytes, W a multiple of 8 in 16..256 -- uint8
    (n, W) is the documented form, int64 (n, W / 8) is the same memory; offsets count rows.  Two rows
    are one element iff all their bytes are equal.  hash="default": java.util.UUID.hashCode of 16-byte
    rows [mostSigBits | leastSigBits]; hash="precomputed" (or just hashes=): one int64 per row, equal
    rows carrying equal hashes.  Returns (out_rows uint8 [S, k, W], out_hashes int64 [S, k], counts
    int64 [S]) device tensors: stream s holds the min(k, distinct) rows with the smallest (scrambled
    hash, row as little-endian unsigned 64-bit words), ascending, rows and hashes beyond counts[s]
    zero -- the set a single Sampler.distinct(k, key_type="bytesW", seed=seed + stream_base + s,
    order="set") fed the same rows holds.  1 <= k <= 4096.
    """
    import torch

    L = N.load()
    rows, offsets, hashes = _segd_rows_inputs(torch, rows, offsets, hash, hashes)
    W = rows.shape[1] * rows.element_size()
    S = offsets.numel() - 1
    # the kernel writes every row block (zeros beyond the count) and every count: no zero-fill
    kk = max(int(k), 0)
    out = torch.empty((max(S, 0), kk, W), dtype=torch.uint8, device=rows.device)
    out_h = torch.empty((max(S, 0), kk), dtype=torch.int64, device=rows.device)
    counts = torch.empty(max(S, 0), dtype=torch.int64, device=rows.device)
    if S <= 0:
        return out, out_h, counts
    N.check(L.rsv_distinct_segmented_rows(
        C.c_void_p(rows.data_ptr()), C.c_void_p(hashes.data_ptr()) if hashes is not None else None,
        C.c_void_p(offsets.data_ptr()), S, W, k, N.HASH_PRECOMPUTED if hashes is not None else N.HASH_DEFAULT,
        seed & (2**64 - 1), stream_base & (2**64 - 1), C.c_void_p(out.data_ptr()), C.c_void_p(out_h.data_ptr()),
        C.c_void_p(counts.data_ptr()), _stream_ptr(torch, rows.device)))
    return out, out_h, counts


class SegmentedDistinct:
    """S long-lived Sampler.distinct streams advanced by one launch per batch (K5 resumed).

    The state is three device tensors in distinct_segmented's layout: keys (S, k), hashes (S, k),
    counts (S,); row s holds counts[s] entries ascending by (scrambled hash, key) and is seeded like
    a single Sampler.distinct(k, seed=seed + stream_base + s, order="set").  Fed a stream in any
    number of update() calls, a row ends bit-identical to distinct_segmented over the whole stream.
    Only the counts are zero-filled: a row with count 0 is empty whatever its slots hold, and every
    row an update writes has zeros beyond its count.  hash="precomputed": update(hashes=...).
    Everything runs on torch's current stream.
    """

    def __init__(self, num_streams: int, k: int, seed: int, stream_base: int = 0, hash: str = "default",
                 dtype=None, device=None):
        import torch

        N.load()
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int64, torch.int32):
            raise N.IllegalArgumentException("keys must be int64/int32")
        if hash == "precomputed":
            self._kind = N.HASH_PRECOMPUTED
        elif hash in _SEG_HASH:
            self._kind = _SEG_HASH[hash]
        else:
            raise N.IllegalArgumentException(f"unknown hash {hash!r}")
        if num_streams < 0:
            raise N.IllegalArgumentException("negative stream count")
        if k <= 0:
            raise N.IllegalArgumentException("k out of range")
        if k > _SEG_DISTINCT_MAX_K:
            raise N.ReservoirError(
                f"SegmentedDistinct holds k <= {_SEG_DISTINCT_MAX_K} per stream; use separate handles beyond")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise N.IllegalArgumentException("the state lives on the device")
        self.num_streams, self.k = int(num_streams), int(k)
        self.seed, self.stream_base = seed & (2**64 - 1), stream_base & (2**64 - 1)
        self.keys = torch.empty((self.num_streams, self.k), dtype=dtype, device=dev)
        self.hashes = torch.empty((self.num_streams, self.k), dtype=torch.int64, device=dev)
        self.counts = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)

    def update(self, keys, offsets, stream_ids=None, hashes=None, check_ids: bool = True):
        """Segment b = keys[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        The ids of one call must be distinct and inside [0, num_streams).  check_ids=True verifies
        that on the device before the launch (one host wait) and raises IllegalArgumentException;
        check_ids=False keeps the call stream-ordered and leaves the contract to the caller.
        Rows that no segment names, or whose segment is empty, are not touched.  Returns self.
        """
        import torch

        L = N.load()
        keys, offsets, hashes = _segd_inputs(torch, keys, offsets, hashes, state=self)
        B = offsets.numel() - 1
        if B <= 0:
            return self
        if stream_ids is not None:
            if not stream_ids.is_cuda or stream_ids.dtype != torch.int64 or stream_ids.numel() != B:
                raise N.IllegalArgumentException("stream_ids must be an int64 device tensor, one per segment")
            stream_ids = stream_ids.contiguous()
            if check_ids:
                _check_stream_ids(torch, stream_ids, self.num_streams)
        N.check(L.rsv_distinct_segmented_update(
            C.c_void_p(keys.data_ptr()), C.c_void_p(hashes.data_ptr()) if hashes is not None else None,
            C.c_void_p(offsets.data_ptr()), C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
            B, self.num_streams, keys.element_size(), self.k, self._kind, self.seed, self.stream_base,
            C.c_void_p(self.keys.data_ptr()), C.c_void_p(self.hashes.data_ptr()), C.c_void_p(self.counts.data_ptr()),
            _stream_ptr(torch, self.keys.device)))
        return self

    def merge(self, part_keys, part_hashes=None, part_counts=None):
        """Row s becomes the bottom-k of (row s u row s of every part).

        merge(part_keys, part_hashes, part_counts): tensors (P, S, k), (P, S, k), (P, S) -- or (S, k),
        (S, k), (S,) for one part -- e.g. an all-gather of every rank's state tensors; or
        merge(other, ...) with SegmentedDistinct objects.  All parts must come from this state's
        seed, stream_base and hash: their hashes are taken as stored.  Returns self.
        """
        import torch

        L = N.load()
        if isinstance(part_keys, SegmentedDistinct):
            others = [part_keys] + [o for o in (part_hashes, part_counts) if o is not None]
            for o in others:
                if not isinstance(o, SegmentedDistinct) or (o.num_streams, o.k, o.seed, o.stream_base, o._kind) != (
                        self.num_streams, self.k, self.seed, self.stream_base, self._kind):
                    raise N.IllegalArgumentException("merge needs states of the same shape, seed, stream_base and hash")
            if len(others) == 1:
                part_keys, part_hashes, part_counts = others[0].keys, others[0].hashes, others[0].counts
            else:
                part_keys = torch.stack([o.keys for o in others])
                part_hashes = torch.stack([o.hashes for o in others])
                part_counts = torch.stack([o.counts for o in others])
        if part_hashes is None or part_counts is None:
            raise N.NullPointerException("merge needs part_keys, part_hashes and part_counts")
        S, k = self.num_streams, self.k
        if part_keys.dim() == 2:
            part_keys, part_hashes, part_counts = part_keys[None], part_hashes[None], part_counts[None]
        P = part_keys.shape[0]
        if tuple(part_keys.shape) != (P, S, k) or tuple(part_hashes.shape) != (P, S, k) or tuple(part_counts.shape) != (P, S):
            raise N.IllegalArgumentException(f"parts must be shaped (P, {S}, {k}), (P, {S}, {k}), (P, {S})")
        if part_keys.dtype != self.keys.dtype or part_hashes.dtype != torch.int64 or part_counts.dtype != torch.int64:
            raise N.IllegalArgumentException("part keys must have the state's dtype, hashes and counts must be int64")
        dev = self.keys.device
        if part_keys.device != dev or part_hashes.device != dev or part_counts.device != dev:
            raise N.IllegalArgumentException("parts must live on the state's device")
        if P == 0 or S == 0:
            return self
        part_keys, part_hashes, part_counts = part_keys.contiguous(), part_hashes.contiguous(), part_counts.contiguous()
        N.check(L.rsv_distinct_segmented_merge(
            C.c_void_p(part_keys.data_ptr()), C.c_void_p(part_hashes.data_ptr()), C.c_void_p(part_counts.data_ptr()),
            P, S, part_keys.element_size(), k, C.c_void_p(self.keys.data_ptr()), C.c_void_p(self.hashes.data_ptr()),
            C.c_void_p(self.counts.data_ptr()), _stream_ptr(torch, dev)))
        return self


class SegmentedDistinctRows:
    """SegmentedDistinct over fixed-width byte keys (java.util.UUID, case classes of primitives).

    The state is three device tensors in distinct_segmented_rows' layout: rows uint8 (S, k, width),
    hashes int64 (S, k), counts int64 (S,); row s holds counts[s] entries ascending by (scrambled
    hash, row as little-endian unsigned 64-bit words) and is seeded like a single
    Sampler.distinct(k, key_type="bytesW", seed=seed + stream_base + s, order="set").  Fed a stream in
    any number of update() calls, a row ends bit-identical to distinct_segmented_rows over the whole
    stream.  Only the counts are zero-filled: a row with count 0 is empty whatever its slots hold, and
    the update that first writes a row zeroes it beyond its count.  width: a multiple of 8 in 16..256.
    hash="default" is UUID.hashCode (width 16 only); hash="precomputed": update(hashes=...).
    Everything runs on torch's current stream.
    """

    def __init__(self, num_streams: int, k: int, width: int, seed: int, stream_base: int = 0, hash: str = "default",
                 device=None):
        import torch

        N.load()
        if hash not in ("default", "precomputed"):
            raise N.IllegalArgumentException(f"unknown hash {hash!r}")
        if num_streams < 0:
            raise N.IllegalArgumentException("negative stream count")
        if k <= 0:
            raise N.IllegalArgumentException("k out of range")
        if k > _SEG_DISTINCT_MAX_K:
            raise N.ReservoirError(
                f"SegmentedDistinctRows holds k <= {_SEG_DISTINCT_MAX_K} per stream; use separate handles beyond")
        if width in (4, 8):
            raise N.ReservoirError("SegmentedDistinctRows takes byte keys; SegmentedDistinct takes 4- and 8-byte keys")
        if width < 16 or width > 256 or width % 8:
            raise N.IllegalArgumentException("width must be a multiple of 8 in 16..256")
        if hash == "default" and width != 16:
            raise N.ReservoirError("hash='default' is UUID.hashCode: width 16 only")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise N.IllegalArgumentException("the state lives on the device")
        self.num_streams, self.k, self.width = int(num_streams), int(k), int(width)
        self.seed, self.stream_base = seed & (2**64 - 1), stream_base & (2**64 - 1)
        self._hash = hash
        self.rows = torch.empty((self.num_streams, self.k, self.width), dtype=torch.uint8, device=dev)
        self.hashes = torch.empty((self.num_streams, self.k), dtype=torch.int64, device=dev)
        self.counts = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)

    def update(self, rows, offsets, stream_ids=None, hashes=None, check_ids: bool = True):
        """Segment b = rows[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        rows: uint8 (n, width) or int64 (n, width / 8), as distinct_segmented_rows takes them; they must
        not overlap the state.  stream_ids and check_ids as SegmentedDistinct.update.  Rows that no
        segment names, or whose segment is empty, are not touched.  Returns self.
        """
        import torch

        L = N.load()
        if hashes is not None and self._hash != "precomputed":
            raise N.IllegalArgumentException("hashes= needs hash='precomputed'")
        rows, offsets, hashes = _segd_rows_inputs(torch, rows, offsets, self._hash, hashes)
        if rows.shape[1] * rows.element_size() != self.width:
            raise N.IllegalArgumentException(f"rows must hold {self.width} bytes each")
        if rows.device != self.rows.device or offsets.device != self.rows.device:
            raise N.IllegalArgumentException("rows and offsets must live on the state's device")
        B = offsets.numel() - 1
        if B <= 0:
            return self
        if stream_ids is not None:
            if not stream_ids.is_cuda or stream_ids.dtype != torch.int64 or stream_ids.numel() != B:
                raise N.IllegalArgumentException("stream_ids must be an int64 device tensor, one per segment")
            stream_ids = stream_ids.contiguous()
            if check_ids:
                _check_stream_ids(torch, stream_ids, self.num_streams)
        N.check(L.rsv_distinct_segmented_rows_update(
            C.c_void_p(rows.data_ptr()), C.c_void_p(hashes.data_ptr()) if hashes is not None else None,
            C.c_void_p(offsets.data_ptr()), C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
            B, self.num_streams, self.width, self.k, N.HASH_PRECOMPUTED if hashes is not None else N.HASH_DEFAULT,
            self.seed, self.stream_base, C.c_void_p(self.rows.data_ptr()), C.c_void_p(self.hashes.data_ptr()),
            C.c_void_p(self.counts.data_ptr()), _stream_ptr(torch, self.rows.device)))
        return self

    def merge(self, part_rows, part_hashes=None, part_counts=None):
        """Row s becomes the bottom-k of (row s u row s of every part).

        merge(part_rows, part_hashes, part_counts): tensors (P, S, k, width), (P, S, k), (P, S) -- or
        (S, k, width), (S, k), (S,) for one part -- e.g. an all-gather of every rank's state tensors;
        or merge(other, ...) with SegmentedDistinctRows objects.  All parts must come from this
        state's seed, stream_base and hash: their hashes are taken as stored.  Returns self.
        """
        import torch

        L = N.load()
        if isinstance(part_rows, SegmentedDistinctRows):
            others = [part_rows] + [o for o in (part_hashes, part_counts) if o is not None]
            mine = (self.num_streams, self.k, self.width, self.seed, self.stream_base, self._hash)
            for o in others:
                if not isinstance(o, SegmentedDistinctRows) or (
                        o.num_streams, o.k, o.width, o.seed, o.stream_base, o._hash) != mine:
                    raise N.IllegalArgumentException(
                        "merge needs states of the same shape, width, seed, stream_base and hash")
            if len(others) == 1:
                part_rows, part_hashes, part_counts = others[0].rows, others[0].hashes, others[0].counts
            else:
                part_rows = torch.stack([o.rows for o in others])
                part_hashes = torch.stack([o.hashes for o in others])
                part_counts = torch.stack([o.counts for o in others])
        if part_hashes is None or part_counts is None:
            raise N.NullPointerException("merge needs part_rows, part_hashes and part_counts")
        S, k, W = self.num_streams, self.k, self.width
        if part_rows.dim() == 3:
            part_rows, part_hashes, part_counts = part_rows[None], part_hashes[None], part_counts[None]
        P = part_rows.shape[0]
        if part_rows.dtype != torch.uint8 or part_hashes.dtype != torch.int64 or part_counts.dtype != torch.int64:
            raise N.IllegalArgumentException("part rows must be uint8, hashes and counts int64")
        if (tuple(part_rows.shape) != (P, S, k, W) or tuple(part_hashes.shape) != (P, S, k)
                or tuple(part_counts.shape) != (P, S)):
            raise N.IllegalArgumentException(f"parts must be shaped (P, {S}, {k}, {W}), (P, {S}, {k}), (P, {S})")
        dev = self.rows.device
        if part_rows.device != dev or part_hashes.device != dev or part_counts.device != dev:
            raise N.IllegalArgumentException("parts must live on the state's device")
        if P == 0 or S == 0:
            return self
        part_rows, part_hashes, part_counts = part_rows.contiguous(), part_hashes.contiguous(), part_counts.contiguous()
        N.check(L.rsv_distinct_segmented_rows_merge(
            C.c_void_p(part_rows.data_ptr()), C.c_void_p(part_hashes.data_ptr()), C.c_void_p(part_counts.data_ptr()),
            P, S, W, k, C.c_void_p(self.rows.data_ptr()), C.c_void_p(self.hashes.data_ptr()),
            C.c_void_p(self.counts.data_ptr()), _stream_ptr(torch, dev)))
        return self


_SEG_SAMPLE_STATE_MAX_K = 15104  # rsv_internal.h kSegSampleStateMaxK


class SegmentedSampler:
    """S long-lived Sampler.apply streams advanced by one launch per batch (K2 resumed).

    The state is three device tensors: keys (S, k); idx (S, k), the global index of each slot's
    last writer, -1 for an empty slot; next (S,), one past the highest index a row has consumed.
    Row s draws like a single "philox_r" Sampler with stream_id = stream_base + s.  Per slot the
    largest index wins, so a row fed its stream in any number of update() calls -- in order, or out
    of order with bases= -- or assembled by merge() from states that each saw a part of the stream,
    ends with the keys sample_segmented gives over the whole stream.  Only idx and next are filled:
    a slot with idx -1 is empty whatever its key holds.  Everything runs on torch's current stream.
    """

    def __init__(self, num_streams: int, k: int, seed: int, stream_base: int = 0, dtype=None, device=None):
        import torch

        N.load()
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int64, torch.int32):
            raise N.IllegalArgumentException("keys must be int64/int32")
        if num_streams < 0:
            raise N.IllegalArgumentException("negative stream count")
        if k <= 0:
            raise N.IllegalArgumentException("k out of range")
        if k > _SEG_SAMPLE_STATE_MAX_K:
            raise N.ReservoirError(
                f"SegmentedSampler holds k <= {_SEG_SAMPLE_STATE_MAX_K} per stream; use separate handles beyond")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise N.IllegalArgumentException("the state lives on the device")
        self.num_streams, self.k = int(num_streams), int(k)
        self.seed, self.stream_base = seed & (2**64 - 1), stream_base & (2**64 - 1)
        self.keys = torch.empty((self.num_streams, self.k), dtype=dtype, device=dev)
        self.idx = torch.full((self.num_streams, self.k), -1, dtype=torch.int64, device=dev)
        self.next = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)

    @property
    def counts(self):
        """Filled slots per row: min(k, elements seen) once a row's pieces cover a prefix of its stream."""
        return (self.idx >= 0).sum(1)

    def update(self, keys, offsets, stream_ids=None, bases=None, check_ids: bool = True):
        """Segment b = keys[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        The segment's first element has global index bases[b] (None: the row's next).  The ids of
        one call must be distinct and inside [0, num_streams).  check_ids=True verifies that on the
        device before the launch (one host wait) and raises IllegalArgumentException;
        check_ids=False keeps the call stream-ordered and leaves the contract to the caller (ids
        outside the range, negative bases and empty segments are then skipped).  Rows that no
        segment names are not touched.  Returns self.
        """
        import torch

        L = N.load()
        if not (keys.is_cuda and offsets.is_cuda):
            raise N.IllegalArgumentException("keys and offsets must be device tensors")
        if keys.dtype != self.keys.dtype or offsets.dtype != torch.int64:
            raise N.IllegalArgumentException("keys must have the state's dtype and offsets must be int64")
        dev = self.keys.device
        if keys.device != dev or offsets.device != dev:
            raise N.IllegalArgumentException("keys and offsets must live on the state's device")
        keys, offsets = keys.contiguous(), offsets.contiguous()
        B = offsets.numel() - 1
        if B <= 0:
            return self
        for name, t in (("stream_ids", stream_ids), ("bases", bases)):
            if t is not None and (not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or t.device != dev):
                raise N.IllegalArgumentException(f"{name} must be an int64 device tensor, one per segment")
        if stream_ids is not None:
            stream_ids = stream_ids.contiguous()
            if check_ids:
                _check_stream_ids(torch, stream_ids, self.num_streams)
        if bases is not None:
            bases = bases.contiguous()
        N.check(L.rsv_sample_segmented_update(
            C.c_void_p(keys.data_ptr()), C.c_void_p(offsets.data_ptr()),
            C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
            C.c_void_p(bases.data_ptr()) if bases is not None else None,
            B, self.num_streams, keys.element_size(), self.k, self.seed, self.stream_base,
            C.c_void_p(self.keys.data_ptr()), C.c_void_p(self.idx.data_ptr()), C.c_void_p(self.next.data_ptr()),
            _stream_ptr(torch, dev)))
        return self

    def merge(self, part_keys, part_idx=None, part_next=None):
        """Per slot the largest idx among row s and row s of every part wins; next takes the max.

        merge(part_keys, part_idx, part_next): tensors (P, S, k), (P, S, k), (P, S) -- or (S, k),
        (S, k), (S,) for one part -- e.g. an all-gather of every rank's state tensors; or
        merge(other, ...) with SegmentedSampler objects.  All parts must come from this state's
        seed and stream_base.  Returns self.
        """
        import torch

        L = N.load()
        if isinstance(part_keys, SegmentedSampler):
            others = [part_keys] + [o for o in (part_idx, part_next) if o is not None]
            for o in others:
                if not isinstance(o, SegmentedSampler) or (o.num_streams, o.k, o.seed, o.stream_base) != (
                        self.num_streams, self.k, self.seed, self.stream_base):
                    raise N.IllegalArgumentException("merge needs states of the same shape, seed and stream_base")
            if len(others) == 1:
                part_keys, part_idx, part_next = others[0].keys, others[0].idx, others[0].next
            else:
                part_keys = torch.stack([o.keys for o in others])
                part_idx = torch.stack([o.idx for o in others])
                part_next = torch.stack([o.next for o in others])
        if part_idx is None or part_next is None:
            raise N.NullPointerException("merge needs part_keys, part_idx and part_next")
        S, k = self.num_streams, self.k
        if part_keys.dim() == 2:
            part_keys, part_idx, part_next = part_keys[None], part_idx[None], part_next[None]
        P = part_keys.shape[0]
        if tuple(part_keys.shape) != (P, S, k) or tuple(part_idx.shape) != (P, S, k) or tuple(part_next.shape) != (P, S):
            raise N.IllegalArgumentException(f"parts must be shaped (P, {S}, {k}), (P, {S}, {k}), (P, {S})")
        if part_keys.dtype != self.keys.dtype or part_idx.dtype != torch.int64 or part_next.dtype != torch.int64:
            raise N.IllegalArgumentException("part keys must have the state's dtype, idx and next must be int64")
        dev = self.keys.device
        if part_keys.device != dev or part_idx.device != dev or part_next.device != dev:
            raise N.IllegalArgumentException("parts must live on the state's device")
        if P == 0 or S == 0:
            return self
        part_keys, part_idx, part_next = part_keys.contiguous(), part_idx.contiguous(), part_next.contiguous()
        N.check(L.rsv_sample_segmented_merge(
            C.c_void_p(part_keys.data_ptr()), C.c_void_p(part_idx.data_ptr()), C.c_void_p(part_next.data_ptr()),
            P, S, part_keys.element_size(), k, C.c_void_p(self.keys.data_ptr()), C.c_void_p(self.idx.data_ptr()),
            C.c_void_p(self.next.data_ptr()), _stream_ptr(torch, dev)))
        return self


def _seg_rows_inputs(torch, rows, offsets):
    """rows / offsets of a K2 call over byte keys, checked and contiguous; returns (rows, offsets, width)."""
    if not (rows.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("rows and offsets must be device tensors")
    if rows.dim() != 2 or rows.dtype not in (torch.uint8, torch.int64) or offsets.dtype != torch.int64:
        raise N.IllegalArgumentException("rows must be 2-D uint8 or int64 (one key per row) and offsets int64")
    return rows.contiguous(), offsets.contiguous(), rows.shape[1] * rows.element_size()


def _check_rows_width(what: str, long_what: str, width: int) -> None:
    if width in (4, 8):
        raise N.ReservoirError(f"{what} takes byte keys; {long_what} takes 4- and 8-byte keys")
    if width < 16 or width > 256 or width % 8:
        raise N.IllegalArgumentException("width must be a multiple of 8 in 16..256")


def sample_segmented_rows(rows, offsets, k: int, seed: int, stream_base: int = 0):
    """sample_segmented over fixed-width byte keys (java.util.UUID, case classes of primitives).

    rows: a contiguous 2-D device tensor whose rows hold W bytes, W a multiple of 8 in 16..256 -- uint8
    (n, W) is the documented form, int64 (n, W / 8) is the same memory; offsets count rows.  Returns
    (out uint8 [S, k, W], counts int64 [S]) device tensors: slot j of stream s holds the row at the
    slot's last writer (row j of the stream where no replacement hit it, zeros for j >= counts[s]) --
    bit-identical to a single Sampler(k, key_type="bytesW", engine="philox_r", stream_id=stream_base + s)
    fed the same rows.  No row is read before its stream's winners are known.
    """
    import torch

    L = N.load()
    rows, offsets, W = _seg_rows_inputs(torch, rows, offsets)
    S = offsets.numel() - 1
    # the kernel writes every slot (empty ones as zeros) and every count: no zero-fill
    kk = max(int(k), 0)
    out = torch.empty((max(S, 0), kk, W), dtype=torch.uint8, device=rows.device)
    counts = torch.empty(max(S, 0), dtype=torch.int64, device=rows.device)
    if S <= 0:
        return out, counts
    N.check(L.rsv_sample_segmented_rows(
        C.c_void_p(rows.data_ptr()), C.c_void_p(offsets.data_ptr()), S, W, k, seed & (2**64 - 1),
        stream_base & (2**64 - 1), C.c_void_p(out.data_ptr()), C.c_void_p(counts.data_ptr()),
        _stream_ptr(torch, rows.device)))
    return out, counts


class SegmentedSamplerRows:
    """SegmentedSampler over fixed-width byte keys (java.util.UUID, case classes of primitives).

    The state is three device tensors: rows uint8 (S, k, width); idx (S, k), the global index of each
    slot's last writer, -1 for an empty slot; next (S,).  Row s draws like a single "philox_r"
    Sampler(k, key_type="bytesW") with stream_id = stream_base + s, and per slot the largest index wins:
    fed its stream in any number of update() calls -- in order, or out of order with bases= -- or
    assembled by merge(), a row ends with the rows sample_segmented_rows gives over the whole stream.
    Only idx and next are filled: a slot with idx -1 is empty whatever its row holds.  width: a multiple
    of 8 in 16..256.  Everything runs on torch's current stream.
    """

    def __init__(self, num_streams: int, k: int, width: int, seed: int, stream_base: int = 0, device=None):
        import torch

        N.load()
        if num_streams < 0:
            raise N.IllegalArgumentException("negative stream count")
        if k <= 0:
            raise N.IllegalArgumentException("k out of range")
        if k > _SEG_SAMPLE_STATE_MAX_K:
            raise N.ReservoirError(
                f"SegmentedSamplerRows holds k <= {_SEG_SAMPLE_STATE_MAX_K} per stream; use separate handles beyond")
        _check_rows_width("SegmentedSamplerRows", "SegmentedSampler", width)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise N.IllegalArgumentException("the state lives on the device")
        self.num_streams, self.k, self.width = int(num_streams), int(k), int(width)
        self.seed, self.stream_base = seed & (2**64 - 1), stream_base & (2**64 - 1)
        self.rows = torch.empty((self.num_streams, self.k, self.width), dtype=torch.uint8, device=dev)
        self.idx = torch.full((self.num_streams, self.k), -1, dtype=torch.int64, device=dev)
        self.next = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)

    @property
    def counts(self):
        """Filled slots per row: min(k, elements seen) once a row's pieces cover a prefix of its stream."""
        return (self.idx >= 0).sum(1)

    def update(self, rows, offsets, stream_ids=None, bases=None, check_ids: bool = True):
        """Segment b = rows[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        rows: uint8 (n, width) or int64 (n, width / 8), as sample_segmented_rows takes them; they must
        not overlap the state.  stream_ids, bases and check_ids as SegmentedSampler.update.  Rows that
        no segment names are not touched.  Returns self.
        """
        import torch

        L = N.load()
        rows, offsets, W = _seg_rows_inputs(torch, rows, offsets)
        if W != self.width:
            raise N.IllegalArgumentException(f"rows must hold {self.width} bytes each")
        dev = self.rows.device
        if rows.device != dev or offsets.device != dev:
            raise N.IllegalArgumentException("rows and offsets must live on the state's device")
        B = offsets.numel() - 1
        if B <= 0:
            return self
        for name, t in (("stream_ids", stream_ids), ("bases", bases)):
            if t is not None and (not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or t.device != dev):
                raise N.IllegalArgumentException(f"{name} must be an int64 device tensor, one per segment")
        if stream_ids is not None:
            stream_ids = stream_ids.contiguous()
            if check_ids:
                _check_stream_ids(torch, stream_ids, self.num_streams)
        if bases is not None:
            bases = bases.contiguous()
        N.check(L.rsv_sample_segmented_rows_update(
            C.c_void_p(rows.data_ptr()), C.c_void_p(offsets.data_ptr()),
            C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
            C.c_void_p(bases.data_ptr()) if bases is not None else None,
            B, self.num_streams, W, self.k, self.seed, self.stream_base,
            C.c_void_p(self.rows.data_ptr()), C.c_void_p(self.idx.data_ptr()), C.c_void_p(self.next.data_ptr()),
            _stream_ptr(torch, dev)))
        return self

    def merge(self, part_rows, part_idx=None, part_next=None):
        """Per slot the largest idx among row s and row s of every part wins; next takes the max.

        merge(part_rows, part_idx, part_next): tensors (P, S, k, width), (P, S, k), (P, S) -- or
        (S, k, width), (S, k), (S,) for one part -- e.g. an all-gather of every rank's state tensors; or
        merge(other, ...) with SegmentedSamplerRows objects.  All parts must come from this state's
        seed and stream_base.  Returns self.
        """
        import torch

        L = N.load()
        if isinstance(part_rows, SegmentedSamplerRows):
            others = [part_rows] + [o for o in (part_idx, part_next) if o is not None]
            mine = (self.num_streams, self.k, self.width, self.seed, self.stream_base)
            for o in others:
                if not isinstance(o, SegmentedSamplerRows) or (
                        o.num_streams, o.k, o.width, o.seed, o.stream_base) != mine:
                    raise N.IllegalArgumentException("merge needs states of the same shape, width, seed and stream_base")
            if len(others) == 1:
                part_rows, part_idx, part_next = others[0].rows, others[0].idx, others[0].next
            else:
                part_rows = torch.stack([o.rows for o in others])
                part_idx = torch.stack([o.idx for o in others])
                part_next = torch.stack([o.next for o in others])
        if part_idx is None or part_next is None:
            raise N.NullPointerException("merge needs part_rows, part_idx and part_next")
        S, k, W = self.num_streams, self.k, self.width
        if part_rows.dim() == 3:
            part_rows, part_idx, part_next = part_rows[None], part_idx[None], part_next[None]
        P = part_rows.shape[0]
        if part_rows.dtype != torch.uint8 or part_idx.dtype != torch.int64 or part_next.dtype != torch.int64:
            raise N.IllegalArgumentException("part rows must be uint8, idx and next int64")
        if (tuple(part_rows.shape) != (P, S, k, W) or tuple(part_idx.shape) != (P, S, k)
                or tuple(part_next.shape) != (P, S)):
            raise N.IllegalArgumentException(f"parts must be shaped (P, {S}, {k}, {W}), (P, {S}, {k}), (P, {S})")
        dev = self.rows.device
        if part_rows.device != dev or part_idx.device != dev or part_next.device != dev:
            raise N.IllegalArgumentException("parts must live on the state's device")
        if P == 0 or S == 0:
            return self
        part_rows, part_idx, part_next = part_rows.contiguous(), part_idx.contiguous(), part_next.contiguous()
        N.check(L.rsv_sample_segmented_rows_merge(
            C.c_void_p(part_rows.data_ptr()), C.c_void_p(part_idx.data_ptr()), C.c_void_p(part_next.data_ptr()),
            P, S, W, k, C.c_void_p(self.rows.data_ptr()), C.c_void_p(self.idx.data_ptr()),
            C.c_void_p(self.next.data_ptr()), _stream_ptr(torch, dev)))
        return self


def replay_events(keys, base_index: int, ev_pos, ev_slot, k: int, reservoir=None):
    """Apply (1-based position, slot) eviction events to the keys at [base, base+n)."""
    import torch

    L = N.load()
    keys = keys.contiguous()
    if reservoir is None:
        reservoir = torch.zeros(k, dtype=keys.dtype, device=keys.device)
    ev_pos = ev_pos.to(device=keys.device, dtype=torch.int64).contiguous()
    ev_slot = ev_slot.to(device=keys.device, dtype=torch.int32).contiguous()
    N.check(L.rsv_replay_events(
        C.c_void_p(keys.data_ptr()), keys.numel(), keys.element_size(), base_index,
        C.c_void_p(ev_pos.data_ptr()), C.c_void_p(ev_slot.data_ptr()), ev_pos.numel(), k,
        C.c_void_p(reservoir.data_ptr()), _stream_ptr(torch, keys.device)))
    return reservoir


def export_draws(seed: int, stream_id: int, i0: int, n: int, device=None):
    """j_i for i in [i0, i0+n) as a uint64-valued int64 device tensor."""
    import torch

    L = N.load()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    N.check(L.rsv_export_draws(seed & (2**64 - 1), stream_id & (2**64 - 1), i0, n,
                               C.c_void_p(out.data_ptr()), _stream_ptr(torch, dev)))
    return out
