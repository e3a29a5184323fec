"""Stateless batch entry points of the HIP engine over device tensors.

torch is used only for device memory and streams (plumbing); the compute runs in
libreservoir_hip.so.  Every function raises if the engine is unavailable.

    sample_segmented  -- K2: S independent samplers in one launch (one wave per stream)
    distinct_segmented -- K5: S independent Sampler.distinct streams in one launch (bottom-k per stream)
    distinct_segmented_rows -- K5 over fixed-width byte keys (UUIDs): rows in, the winning rows out
    distinct_segmented_rows_ordered -- the same in the reference's order (exact under UUID.hashCode's ties)
    SegmentedDistinct -- K5 resumed: the same S streams as caller-held state, advanced by one launch
                         per micro-batch (update) and combined across launches, GPUs and ranks (merge)
    SegmentedDistinctOrdered -- the ordered form resumed: the state rows are the reference's heap arrays (update)
    SegmentedDistinctRows -- K5 resumed over byte keys: the rows move inside the caller-held state (update, merge)
    SegmentedDistinctRowsOrdered -- the ordered form resumed over byte keys: the heap arrays hold (hash, slot) and
                         the rows stay in their slots of the caller-held state (update)
    distinct_segmented_candidates -- Sampler.distinct for any B over S streams: hashes in, candidate positions out
    SegmentedObjectDistinct -- the same as live state: a hash shadow per row on the device, a RandomValues
                         replica per row on the host, one candidate launch per batch (update)
    SegmentedSampler  -- K2 resumed: S Sampler.apply streams as caller-held state (keys, idx, next), fed in
                         pieces from any start index (update) and combined per slot by largest index (merge)
    sample_segmented_rows -- K2 over fixed-width byte keys (UUIDs): rows in, each slot's winning row out
    SegmentedSamplerRows -- K2 resumed over byte keys: state (rows, idx, next), update and merge as SegmentedSampler
    sample_segmented_indexed -- K2 without keys: the streams' lengths in, each slot's winning index out; streams
                         longer than the split length are taken in pieces over the whole device
    sample_segmented_objects -- Sampler.apply for any B over S streams: the same launch, the elements picked on the host
    SegmentedObjectSampler -- the same as live state: (idx, next) on the device, a slot list per row on the host,
                         one launch per batch that reports the replaced slots (update), and merge by source part
    group_by_stream   -- a micro-batch tagged by substream in arrival order to the dense CSR (offsets, order) over
                         all rows, on the device; update_by_id(data, ids) on the element and distinct states is that
                         pass and their update in one call (the element samplers read only their winners, through order)
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


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def group_by_stream(ids, num_streams: int):
    """Group a micro-batch by substream on the device: ids in arrival order in, the dense CSR out.

    ids: a 1-D int64 or int32 device tensor, ids[i] the state row of the batch's i-th element.  Returns
    (offsets int64 (num_streams + 1,), order int32 (n,)) on ids' device: order[offsets[r]:offsets[r+1]] are the
    batch positions of row r's elements in arrival order (empty for a row the batch does not name), ids outside
    [0, num_streams) are dropped -- offsets[num_streams] elements are kept -- and their positions follow in
    order[offsets[num_streams]:], in arrival order, so order is a permutation of [0, n).  The same input gives
    the same tensors.  Runs on torch's current stream without a host wait.
    """
    import torch

    L = N.load()
    if not ids.is_cuda:
        raise N.IllegalArgumentException("ids must be a device tensor")
    if ids.dtype not in (torch.int64, torch.int32) or ids.dim() != 1:
        raise N.IllegalArgumentException("ids must be a 1-D int64/int32 tensor")
    if num_streams < 1:
        raise N.IllegalArgumentException("num_streams must be at least 1")
    ids = ids.contiguous()
    n = ids.numel()
    offsets = torch.empty(int(num_streams) + 1, dtype=torch.int64, device=ids.device)
    order = torch.empty(n, dtype=torch.int32, device=ids.device)
    with torch.cuda.device(ids.device):  # the pass allocates its scratch on the current device
        N.check(L.rsv_group_by_stream(_ptr(ids) if n else None, ids.element_size(), n, int(num_streams), _ptr(offsets),
                                      _ptr(order) if n else None, _stream_ptr(torch, ids.device)))
    return offsets, order


def _segd_kind(hash, precomputed: bool) -> int:
    """The hash kind of a K5 call over 4- and 8-byte keys."""
    if precomputed:
        return N.HASH_PRECOMPUTED
    if hash in _SEG_HASH:
        return _SEG_HASH[hash]
    raise N.IllegalArgumentException(f"unknown hash {hash!r}")


def _segd_stateless(torch, fn, data, hashes, offsets, width, k, kind, seed, stream_base, out_dtype, ordered):
    """The outputs and the native call (fn) of the four stateless K5 functions.  data: keys, or rows of `width`
    bytes each, for which out is (S, k, width); ordered: a fourth output, tied (S,) int32."""
    S = offsets.numel() - 1
    # the kernel writes every slot or row block (zeros beyond the count) and every count: no zero-fill
    kk = max(int(k), 0)
    out = torch.empty((max(S, 0), kk) + ((width,) if data.dim() == 2 else ()), dtype=out_dtype, device=data.device)
    res = [out, torch.empty((max(S, 0), kk), dtype=torch.int64, device=data.device),
           torch.empty(max(S, 0), dtype=torch.int64, device=data.device)]
    if ordered:
        res.append(torch.empty(max(S, 0), dtype=torch.int32, device=data.device))
    if S > 0:
        N.check(fn(_ptr(data), _ptr(hashes), _ptr(offsets), S, width, k, kind, seed & (2**64 - 1),
                   stream_base & (2**64 - 1), *(_ptr(t) for t in res), _stream_ptr(torch, data.device)))
    return tuple(res)


def _segd_keys_stateless(fn, keys, offsets, k, seed, stream_base, hash, hashes, ordered):
    import torch

    keys, offsets, hashes = _segd_inputs(torch, keys, offsets, hashes)
    kind = _segd_kind(hash, hashes is not None)
    return _segd_stateless(torch, fn, keys, hashes, offsets, keys.element_size(), k, kind, seed, stream_base,
                           keys.dtype, ordered)


def distinct_segmented(keys, offsets, k: int, seed: int, stream_base: int = 0, hash: str = "default", hashes=None):
    """Distinct-sample each of S streams keys[offsets[s]:offsets[s+1]] independently (bottom-k).

    Returns (out_keys[S, k], out_hashes[S, k], counts[S]) device tensors.  Stream s holds the
    min(k, distinct) keys with the smallest (scrambled hash, key), ascending, slots beyond counts[s]
    zero: what a single Sampler.distinct(k, seed=seed + stream_base + s, order="set") fed the same
    keys holds.  hash: "default" | "identity" | "java_long" | "java_int"; hashes= (one int64 per
    key, a device tensor) means precomputed hashes.  1 <= k <= 4096.
    """
    return _segd_keys_stateless(N.load().rsv_distinct_segmented, keys, offsets, k, seed, stream_base, hash, hashes, False)


def distinct_segmented_ordered(keys, offsets, k: int, seed: int, stream_base: int = 0, hash: str = "default",
                               hashes=None):
    """distinct_segmented in the reference's order: exact for any hash, the tie bucket included.

    Returns (out_keys[S, k], out_hashes[S, k], counts[S], tied[S]) device tensors (tied int32).  Stream s
    holds the set a single Sampler.distinct(k, seed=seed + stream_base + s, order="ordered") fed the same
    keys in the same order holds -- the reference's RandomValues -- written ascending by (scrambled hash,
    key), slots beyond counts[s] zero.  tied[s] is 1 iff the set is full and a distinct key outside the
    bottom-k by (hash, key) has the set's maximum hash; where it is 0 the row is distinct_segmented's.
    hash / hashes and k as distinct_segmented.
    """
    return _segd_keys_stateless(N.load().rsv_distinct_segmented_ordered, keys, offsets, k, seed, stream_base, hash,
                                hashes, True)


def _rows_inputs(torch, rows, offsets, dtypes=None):
    """rows / offsets of a call over byte keys (dtypes: the row dtypes it takes, None: any), checked and
    contiguous; returns (rows, offsets, width)."""
    if not (rows.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("rows and offsets must be device tensors")
    if rows.dim() != 2 or (dtypes and rows.dtype not in dtypes) or offsets.dtype != torch.int64:
        what = "uint8 or int64 " if dtypes else ""
        raise N.IllegalArgumentException(f"rows must be 2-D {what}(one key per row) and offsets int64")
    return rows.contiguous(), offsets.contiguous(), rows.shape[1] * rows.element_size()


def _segd_rows_inputs(torch, rows, offsets, hash, hashes):
    """rows / offsets / hashes of a K5 call over byte keys, checked and contiguous."""
    rows, offsets, _ = _rows_inputs(torch, rows, offsets)
    if hashes is None and hash == "precomputed":
        raise N.NullPointerException("hash='precomputed' needs hashes=")
    if hashes is None and hash != "default":
        raise N.IllegalArgumentException(f"unknown hash {hash!r}")
    if hashes is not None:
        if not hashes.is_cuda or hashes.dtype != torch.int64 or hashes.numel() != rows.shape[0]:
            raise N.IllegalArgumentException("hashes must be an int64 device tensor, one per row")
        # an empty tensor has no address; the engine wants one for precomputed hashes
        hashes = hashes.contiguous() if hashes.numel() else torch.empty(1, dtype=torch.int64, device=rows.device)
    return rows, offsets, hashes


def _segd_rows_stateless(fn, rows, offsets, k, seed, stream_base, hash, hashes, ordered):
    import torch

    rows, offsets, hashes = _segd_rows_inputs(torch, rows, offsets, hash, hashes)
    kind = N.HASH_PRECOMPUTED if hashes is not None else N.HASH_DEFAULT
    return _segd_stateless(torch, fn, rows, hashes, offsets, rows.shape[1] * rows.element_size(), k, kind, seed,
                           stream_base, torch.uint8, ordered)


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
    return _segd_rows_stateless(N.load().rsv_distinct_segmented_rows, rows, offsets, k, seed, stream_base, hash, hashes,
                                False)


def distinct_segmented_rows_ordered(rows, offsets, k: int, seed: int, stream_base: int = 0, hash: str = "default",
                                    hashes=None):
    """distinct_segmented_rows in the reference's order: exact for any hash, the tie bucket included.

    rows, offsets, hash / hashes and k as distinct_segmented_rows.  Returns (out_rows uint8 [S, k, W],
    out_hashes int64 [S, k], counts int64 [S], tied int32 [S]) device tensors.  Stream s holds the set a
    single Sampler.distinct(k, key_type="bytesW", seed=seed + stream_base + s, order="ordered") fed the same
    rows in the same order holds -- the reference's RandomValues over byte keys -- written ascending by
    (scrambled hash, row words), rows and hashes beyond counts[s] zero.  tied[s] is 1 iff the set is full and
    a distinct row outside the bottom-k by (hash, row) has the set's maximum hash; where it is 0 the row
    block is distinct_segmented_rows'.  Under the default hash of 16-byte rows (UUID.hashCode, 32 bits) ties
    are what this call is for.
    """
    return _segd_rows_stateless(N.load().rsv_distinct_segmented_rows_ordered, rows, offsets, k, seed, stream_base, hash,
                                hashes, True)


def _check_rows_width(what: str, long_what: str, width: int) -> None:
    if width in (4, 8):
        raise N.ReservoirError(f"{what} takes byte keys; {long_what} takes 4- and 8-byte keys")
    if width < 16 or width > 256 or width % 8:
        raise N.IllegalArgumentException("width must be a multiple of 8 in 16..256")


class _SegmentedState:
    """What the caller-held states share: the constructor's checks, the segment side of update() and
    the argument handling of merge().  A subclass names its tensors (_TENSORS: the payload keys (S, k) or
    rows (S, k, width) first, then the per-slot tensors -- one, or two where the slots hold references -- and the
    per-row tensor; merge() is for the classes with three), itself and its cap on k for the messages (_NAME,
    _MAX_K; _LONG: a rows class's counterpart for 4- and 8-byte keys), what merge(other) compares (_identity(),
    _SAME in the message), and makes its own native calls."""

    _NAME = _LONG = _SAME = ""
    _TENSORS: tuple = ()
    _MAX_K = 0

    def _check_width(self, width) -> None:
        if width is not None:  # a rows class
            _check_rows_width(self._NAME, self._LONG, width)
            self.width = int(width)

    def _init_state(self, torch, num_streams, k, seed, stream_base, device, width=None):
        """The checks every constructor ends with; returns the state's device."""
        if num_streams < 0:
            raise N.IllegalArgumentException("negative stream count")
        if k <= 0:
            raise N.IllegalArgumentException("k out of range")
        if k > self._MAX_K:
            raise N.ReservoirError(
                f"{self._NAME} holds k <= {self._MAX_K} per stream; use separate handles beyond")
        self._check_width(width)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise N.IllegalArgumentException("the state lives on the device")
        self.num_streams, self.k = int(num_streams), int(k)
        self.seed, self.stream_base = seed & (2**64 - 1), stream_base & (2**64 - 1)
        return dev

    def _state(self):
        return [getattr(self, name) for name in self._TENSORS]

    def _key_width(self) -> int:
        return self.width if self._TENSORS[0] == "rows" else self.keys.element_size()

    def _check_same_device(self, data, offsets) -> None:
        """The payload of an update against the state: its row width (the rows classes) and its device."""
        if data.dim() == 2 and self._TENSORS[0] == "rows" and data.shape[1] * data.element_size() != self.width:
            raise N.IllegalArgumentException(f"rows must hold {self.width} bytes each")
        dev = self._state()[0].device
        if data.device != dev or offsets.device != dev:
            raise N.IllegalArgumentException(f"{self._TENSORS[0]} and offsets must live on the state's device")

    def _segments(self, torch, offsets, check_ids, stream_ids, **per_segment):
        """The segment side of an update: None if there is no segment, else [B, stream_ids, ...] with
        stream_ids and the optional per-segment tensor (bases=) checked, contiguous, and the ids verified."""
        B = offsets.numel() - 1
        if B <= 0:
            return None
        dev = self._state()[0].device
        out = [B]
        for name, t in dict(stream_ids=stream_ids, **per_segment).items():
            if t is not None:
                if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B or t.device != dev:
                    raise N.IllegalArgumentException(f"{name} must be an int64 device tensor, one per segment")
                t = t.contiguous()
            out.append(t)
        if stream_ids is not None and check_ids:
            _check_stream_ids(torch, out[1], self.num_streams)
        return out

    def _group(self, torch, data, ids):
        """The id side of an update_by_id: data (keys or rows in arrival order) and ids checked against the state,
        then group_by_stream over the state's rows; None if there is nothing to feed."""
        what = self._TENSORS[0]
        if not (data.is_cuda and ids.is_cuda):
            raise N.IllegalArgumentException(f"{what} and ids must be device tensors")
        if ids.dtype not in (torch.int64, torch.int32) or ids.dim() != 1:
            raise N.IllegalArgumentException("ids must be a 1-D int64/int32 tensor")
        dev = self._state()[0].device
        if data.device != dev or ids.device != dev:
            raise N.IllegalArgumentException(f"{what} and ids must live on the state's device")
        if data.dim() < 1 or data.shape[0] != ids.numel():
            raise N.IllegalArgumentException(f"ids must hold one id per element of {what}")
        if self.num_streams == 0 or ids.numel() == 0:
            return None
        return group_by_stream(ids, self.num_streams)

    def _merge(self, torch, fn, cls, parts):
        """merge() of every class: parts = (payload, per-slot, per-row) tensors, stacked (P, ...) or one part
        without the leading axis, or up to three states of class cls; fn is the native merge."""
        names = self._TENSORS
        if isinstance(parts[0], cls):
            others = [o for o in parts if o is not None]
            for o in others:
                if not isinstance(o, cls) or o._identity() != self._identity():
                    raise N.IllegalArgumentException(f"merge needs states of the same shape, {self._SAME}")
            if len(others) == 1:
                parts = others[0]._state()
            else:
                parts = [torch.stack([getattr(o, name) for o in others]) for name in names]
        if parts[1] is None or parts[2] is None:
            raise N.NullPointerException(f"merge needs part_{names[0]}, part_{names[1]} and part_{names[2]}")
        mine = self._state()
        if parts[0].dim() == mine[0].dim():
            parts = [p[None] for p in parts]
        P = parts[0].shape[0]
        rows = names[0] == "rows"

        def check_shapes():
            if any(tuple(p.shape) != (P,) + tuple(m.shape) for p, m in zip(parts, mine)):
                want = ", ".join("(P, " + ", ".join(str(n) for n in m.shape) + ")" for m in mine)
                raise N.IllegalArgumentException(f"parts must be shaped {want}")

        if not rows:  # (the rows classes look at the dtypes first)
            check_shapes()
        if parts[0].dtype != mine[0].dtype or parts[1].dtype != torch.int64 or parts[2].dtype != torch.int64:
            raise N.IllegalArgumentException(
                f"part rows must be uint8, {names[1]} and {names[2]} int64" if rows else
                f"part keys must have the state's dtype, {names[1]} and {names[2]} must be int64")
        if rows:
            check_shapes()
        dev = mine[0].device
        if any(p.device != dev for p in parts):
            raise N.IllegalArgumentException("parts must live on the state's device")
        if P == 0 or self.num_streams == 0:
            return self
        parts = [p.contiguous() for p in parts]
        N.check(fn(*(C.c_void_p(p.data_ptr()) for p in parts), P, self.num_streams, self._key_width(), self.k,
                   *(C.c_void_p(m.data_ptr()) for m in mine), _stream_ptr(torch, dev)))
        return self


class _DistinctState(_SegmentedState):
    """What the four K5 states share: the cap on k, the allocation of the state (_TENSORS[0], the payload, by the
    subclass's base; hashes int64 and, where there are any, slots int32, (S, k); only the counts zero-filled) and the
    native call of update(), whose entry points (_UPDATE) take the state's tensors last, in _TENSORS' order."""

    _MAX_K = _SEG_DISTINCT_MAX_K
    _UPDATE = ""

    def _alloc(self, torch, dev, payload_shape, payload_dtype) -> None:
        setattr(self, self._TENSORS[0], torch.empty(payload_shape, dtype=payload_dtype, device=dev))
        for name in self._TENSORS[1:-1]:
            dtype = torch.int32 if name == "slots" else torch.int64
            setattr(self, name, torch.empty((self.num_streams, self.k), dtype=dtype, device=dev))
        self.counts = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)

    def _launch_update(self, torch, data, hashes, offsets, check_ids, stream_ids, kind):
        seg = self._segments(torch, offsets, check_ids, stream_ids)
        if seg is None:
            return self
        B, stream_ids = seg
        state = self._state()
        N.check(getattr(N.load(), self._UPDATE)(
            _ptr(data), _ptr(hashes), _ptr(offsets), _ptr(stream_ids), B, self.num_streams, self._key_width(), self.k,
            kind, self.seed, self.stream_base, *(_ptr(t) for t in state), _stream_ptr(torch, state[0].device)))
        return self

    def update_by_id(self, data, ids, hashes=None):
        """The batch in arrival order, element i into row ids[i]: group_by_stream, one gather, then update().

        data: the keys or rows update() takes, in arrival order; ids: int64 or int32, one per element; hashes as
        update() takes them, one per element in arrival order.  The distinct kernels read every key of a segment,
        so the keys (and hashes) are moved once, by index_select through the grouping's order; update() then runs
        over the dense CSR -- every row a segment, the empty ones skipped -- with check_ids=False: nothing can
        repeat, and elements whose id lies outside [0, num_streams) are dropped (they ride along behind the last
        offset and are never read).  Within a row the elements keep their arrival order.  No host wait.
        Returns self.
        """
        import torch

        grouped = self._group(torch, data, ids)
        if grouped is None:
            return self
        offsets, order = grouped
        if hashes is not None:
            if not hashes.is_cuda or hashes.dim() != 1 or hashes.numel() != ids.numel() or hashes.device != ids.device:
                raise N.IllegalArgumentException("hashes must be a device tensor on the state's device, one per element")
            hashes = hashes.index_select(0, order)
        return self.update(data.index_select(0, order), offsets, None, hashes, check_ids=False)


class _DistinctKeysState(_DistinctState):
    """The two states over 4- and 8-byte keys: hash parsing, dtype check, allocation; update() but for its docstring."""

    _TENSORS = ("keys", "hashes", "counts")

    def __init__(self, num_streams: int, k: int, seed: int, stream_base: int = 0, hash: str = "default",
                 dtype=None, device=None):
        import torch

        N.load()
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int64, torch.int32):
            raise N.IllegalArgumentException("keys must be int64/int32")
        self._kind = _segd_kind(hash, hash == "precomputed")
        dev = self._init_state(torch, num_streams, k, seed, stream_base, device)
        self._alloc(torch, dev, (self.num_streams, self.k), dtype)

    def _update(self, keys, offsets, stream_ids, hashes, check_ids):
        import torch

        N.load()
        keys, offsets, hashes = _segd_inputs(torch, keys, offsets, hashes, state=self)
        return self._launch_update(torch, keys, hashes, offsets, check_ids, stream_ids, self._kind)


class _DistinctRowsState(_DistinctState):
    """The two states over byte keys: the hash check, _check_width, allocation; update() but for its docstring."""

    def _check_width(self, width) -> None:
        super()._check_width(width)
        if self._hash == "default" and width != 16:
            raise N.ReservoirError("hash='default' is UUID.hashCode: width 16 only")

    def __init__(self, num_streams: int, k: int, width: int, seed: int, stream_base: int = 0, hash: str = "default",
                 device=None):
        import torch

        N.load()
        if hash not in ("default", "precomputed"):
            raise N.IllegalArgumentException(f"unknown hash {hash!r}")
        self._hash = hash
        dev = self._init_state(torch, num_streams, k, seed, stream_base, device, width)
        self._alloc(torch, dev, (self.num_streams, self.k, self.width), torch.uint8)

    def _update(self, rows, offsets, stream_ids, hashes, check_ids):
        import torch

        N.load()
        if hashes is not None and self._hash != "precomputed":
            raise N.IllegalArgumentException("hashes= needs hash='precomputed'")
        rows, offsets, hashes = _segd_rows_inputs(torch, rows, offsets, self._hash, hashes)
        self._check_same_device(rows, offsets)
        return self._launch_update(torch, rows, hashes, offsets, check_ids, stream_ids,
                                   N.HASH_PRECOMPUTED if hashes is not None else N.HASH_DEFAULT)


class SegmentedDistinct(_DistinctKeysState):
    """S long-lived Sampler.distinct streams advanced by one launch per batch (K5 resumed).

    The state is three device tensors in distinct_segmented's layout: keys (S, k), hashes (S, k),
    counts (S,); row s holds counts[s] entries ascending by (scrambled hash, key) and is seeded like
    a single Sampler.distinct(k, seed=seed + stream_base + s, order="set").  Fed a stream in any
    number of update() calls, a row ends bit-identical to distinct_segmented over the whole stream.
    Only the counts are zero-filled: a row with count 0 is empty whatever its slots hold, and every
    row an update writes has zeros beyond its count.  hash="precomputed": update(hashes=...).
    Everything runs on torch's current stream.
    """

    _NAME, _UPDATE = "SegmentedDistinct", "rsv_distinct_segmented_update"
    _SAME = "seed, stream_base and hash"

    def _identity(self):
        return self.num_streams, self.k, self.seed, self.stream_base, self._kind

    def update(self, keys, offsets, stream_ids=None, hashes=None, check_ids: bool = True):
        """Segment b = keys[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        The ids of one call must be distinct and inside [0, num_streams).  check_ids=True verifies
        that on the device before the launch (one host wait) and raises IllegalArgumentException;
        check_ids=False keeps the call stream-ordered and leaves the contract to the caller.
        Rows that no segment names, or whose segment is empty, are not touched.  Returns self.
        """
        return self._update(keys, offsets, stream_ids, hashes, check_ids)

    def merge(self, part_keys, part_hashes=None, part_counts=None):
        """Row s becomes the bottom-k of (row s u row s of every part).

        merge(part_keys, part_hashes, part_counts): tensors (P, S, k), (P, S, k), (P, S) -- or (S, k),
        (S, k), (S,) for one part -- e.g. an all-gather of every rank's state tensors; or
        merge(other, ...) with SegmentedDistinct objects.  All parts must come from this state's
        seed, stream_base and hash: their hashes are taken as stored.  Returns self.
        """
        import torch

        L = N.load()
        return self._merge(torch, L.rsv_distinct_segmented_merge, SegmentedDistinct, (part_keys, part_hashes, part_counts))


class SegmentedDistinctOrdered(_DistinctKeysState):
    """S long-lived Sampler.distinct streams in the reference's order, advanced by one launch per batch.

    What SegmentedDistinct is for the set order, for order="ordered": exact for any hash, the tie bucket included.
    The state is three device tensors keys (S, k), hashes (S, k), counts (S,), and row s is the reference's
    RandomValues itself: counts[s] entries in scala 2.13 mutable.PriorityQueue array order (entry j of the
    1-indexed queue in slot j - 1, its scrambled hash beside it), seeded like a single
    Sampler.distinct(k, seed=seed + stream_base + s, order="ordered").  Fed a stream in any number of update()
    calls, a row is the array the reference holds after the same elements in the same order.  This is NOT
    SegmentedDistinct's layout: a sorted row is not a valid ordered state, and the two kinds of state must not be
    mixed; result() gives the rows sorted.  Only the counts are zero-filled: a row with count 0 is empty whatever
    its slots hold, and every row an update writes has zeros beyond its count.  hash="precomputed":
    update(hashes=...).  There is no merge.  Everything runs on torch's current stream.
    """

    _NAME, _UPDATE = "SegmentedDistinctOrdered", "rsv_distinct_segmented_ordered_update"

    def update(self, keys, offsets, stream_ids=None, hashes=None, check_ids: bool = True):
        """Segment b = keys[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b), in arrival order.

        The ids of one call must be distinct and inside [0, num_streams).  check_ids=True verifies
        that on the device before the launch (one host wait) and raises IllegalArgumentException;
        check_ids=False keeps the call stream-ordered and leaves the contract to the caller.
        Rows that no segment names, or whose segment is empty, are not touched, and a row in which
        nothing was admitted is not written.  Returns self.
        """
        return self._update(keys, offsets, stream_ids, hashes, check_ids)

    def result(self):
        """(keys (S, k), hashes (S, k), counts (S,)) in distinct_segmented_ordered's layout: every row ascending
        by (scrambled hash, key), zeros beyond its count.  New tensors; the state is left as it is."""
        import torch

        counts = self.counts.clamp(0, self.k)
        valid = torch.arange(self.k, device=self.keys.device)[None, :] < counts[:, None]
        # by key, then stably by hash, then stably the valid entries first: ascending by (h, key) in front
        order = torch.argsort(self.keys.masked_fill(~valid, 0), dim=1, stable=True)
        order = order.gather(1, torch.argsort(self.hashes.gather(1, order), dim=1, stable=True))
        order = order.gather(1, torch.argsort((~valid).gather(1, order).to(torch.int8), dim=1, stable=True))
        keep = valid.gather(1, order)
        zero_k = torch.zeros((), dtype=self.keys.dtype, device=self.keys.device)
        zero_h = torch.zeros((), dtype=torch.int64, device=self.keys.device)
        return (torch.where(keep, self.keys.gather(1, order), zero_k),
                torch.where(keep, self.hashes.gather(1, order), zero_h), counts)

    def merge(self, *parts, **kw):
        """Not provided: two heaps over parts of a stream do not determine the reference's heap over the whole."""
        raise N.ReservoirError(
            "SegmentedDistinctOrdered has no merge: two heaps over disjoint parts of a stream do not determine the "
            "reference's heap over the whole stream; SegmentedDistinct.merge combines states in the set order")


class SegmentedDistinctRows(_DistinctRowsState):
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

    _NAME, _LONG, _UPDATE = "SegmentedDistinctRows", "SegmentedDistinct", "rsv_distinct_segmented_rows_update"
    _TENSORS, _SAME = ("rows", "hashes", "counts"), "width, seed, stream_base and hash"

    def _identity(self):
        return self.num_streams, self.k, self.width, self.seed, self.stream_base, self._hash

    def update(self, rows, offsets, stream_ids=None, hashes=None, check_ids: bool = True):
        """Segment b = rows[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        rows: uint8 (n, width) or int64 (n, width / 8), as distinct_segmented_rows takes them; they must
        not overlap the state.  stream_ids and check_ids as SegmentedDistinct.update.  Rows that no
        segment names, or whose segment is empty, are not touched.  Returns self.
        """
        return self._update(rows, offsets, stream_ids, hashes, check_ids)

    def merge(self, part_rows, part_hashes=None, part_counts=None):
        """Row s becomes the bottom-k of (row s u row s of every part).

        merge(part_rows, part_hashes, part_counts): tensors (P, S, k, width), (P, S, k), (P, S) -- or
        (S, k, width), (S, k), (S,) for one part -- e.g. an all-gather of every rank's state tensors;
        or merge(other, ...) with SegmentedDistinctRows objects.  All parts must come from this
        state's seed, stream_base and hash: their hashes are taken as stored.  Returns self.
        """
        import torch

        L = N.load()
        return self._merge(torch, L.rsv_distinct_segmented_rows_merge, SegmentedDistinctRows,
                           (part_rows, part_hashes, part_counts))


class SegmentedDistinctRowsOrdered(_DistinctRowsState):
    """SegmentedDistinctOrdered over fixed-width byte keys (java.util.UUID, case classes of primitives).

    What SegmentedDistinctRows is for the set order, for order="ordered": exact for any hash, UUID.hashCode's 32
    bits included.  The state is four device tensors, and row s is the reference's RandomValues itself, its queue's
    array holding references as on the JVM: hashes int64 (S, k) and slots int32 (S, k) are counts[s] entries in
    scala 2.13 mutable.PriorityQueue array order (entry j of the 1-indexed queue at position j - 1), and the row of
    the entry at position p is rows[s, slots[s, p]]; rows uint8 (S, k, width) is storage whose order means nothing;
    counts int64 (S,).  An admission that grows the heap from n entries takes slot n, one into a full heap takes the
    slot of the root it evicts, so no surviving row ever moves and the whole state is a function of what a row was
    fed, in that order, however it was cut into update() calls.  Row s is seeded like a single
    Sampler.distinct(k, key_type="bytesW", seed=seed + stream_base + s, order="ordered").  This is NOT
    SegmentedDistinctRows' layout, and the two kinds of state must not be mixed; result() gives the rows sorted.
    Only the counts are zero-filled: a row with count 0 is empty whatever the rest holds.  width: a multiple of 8 in
    16..256.  hash="default" is UUID.hashCode (width 16 only); hash="precomputed": update(hashes=...).  There is no
    merge.  Everything runs on torch's current stream.
    """

    _NAME, _LONG = "SegmentedDistinctRowsOrdered", "SegmentedDistinctOrdered"
    _TENSORS, _UPDATE = ("rows", "hashes", "slots", "counts"), "rsv_distinct_segmented_rows_ordered_update"

    def update(self, rows, offsets, stream_ids=None, hashes=None, check_ids: bool = True):
        """Segment b = rows[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b), in arrival order.

        rows: uint8 (n, width) or int64 (n, width / 8), as distinct_segmented_rows takes them; they must
        not overlap the state.  stream_ids and check_ids as SegmentedDistinct.update.  Rows that no
        segment names, or whose segment is empty, are not touched, and a row in which nothing was admitted
        is not written.  Returns self.
        """
        return self._update(rows, offsets, stream_ids, hashes, check_ids)

    def result(self):
        """(rows uint8 (S, k, width), hashes (S, k), counts (S,)) in distinct_segmented_rows_ordered's layout: every
        row block ascending by (scrambled hash, words as unsigned little-endian 64-bit values, word 0 first), zeros
        beyond its count.  New tensors; the state is left as it is, and nothing waits for the device."""
        import torch

        S, k, W8 = self.num_streams, self.k, self.width // 8
        dev = self.rows.device
        counts = self.counts.clamp(0, k)
        valid = torch.arange(k, device=dev)[None, :] < counts[:, None]
        # the rows in array order; unsigned order of a word = signed order of the word with its top bit flipped
        slots = self.slots.clamp(0, k - 1).to(torch.int64)
        words = self.rows.view(torch.int64).gather(1, slots[:, :, None].expand(S, k, W8))
        ordw = (words ^ torch.iinfo(torch.int64).min).masked_fill(~valid[:, :, None], 0)
        # stably by the last word up to word 0, then by hash, then the valid entries first
        order = torch.arange(k, device=dev)[None, :].expand(S, k)
        for w in range(W8 - 1, -1, -1):
            order = order.gather(1, torch.argsort(ordw[:, :, w].gather(1, order), dim=1, stable=True))
        order = order.gather(1, torch.argsort(self.hashes.gather(1, order), dim=1, stable=True))
        order = order.gather(1, torch.argsort((~valid).gather(1, order).to(torch.int8), dim=1, stable=True))
        keep = valid.gather(1, order)
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        out = torch.where(keep[:, :, None], words.gather(1, order[:, :, None].expand(S, k, W8)), zero)
        return (out.contiguous().view(torch.uint8).reshape(S, k, self.width),
                torch.where(keep, self.hashes.gather(1, order), zero), counts)

    def merge(self, *parts, **kw):
        """Not provided: two heaps over parts of a stream do not determine the reference's heap over the whole."""
        raise N.ReservoirError(
            "SegmentedDistinctRowsOrdered has no merge: two heaps over disjoint parts of a stream do not determine the "
            "reference's heap over the whole stream; SegmentedDistinctRows.merge combines states in the set order")


# rsv_segdistinct.hip, segcand_kernel: (largest k of the form, its candidate buffer).  A bound lags the exact running
# one by at most one buffer of candidates.
SEGMENTED_CANDIDATE_BUFFER = ((64, 256), (256, 512), (1024, 2048), (4096, 8192))


def segmented_candidate_buffer(k: int) -> int:
    return next(w for top, w in SEGMENTED_CANDIDATE_BUFFER if k <= top)


def segmented_candidate_cap(k: int, longest: int) -> int:
    """The default cap of a candidate launch from k and the longest segment: a fresh stream of n distinct hashes
    admits about k (1 + ln(n / k)) elements, the lazy bound adds about one buffer (measured: 578 candidates per
    stream against 312 admissions at n = 4096, k = 64, 24 272 against 17 208 at n = 2^17, k = 4096), and a quarter
    on top covers the spread between streams; never more than the segment holds.  Too small only costs a rerun of
    the segments that overflowed."""
    import math

    longest = max(int(longest), 1)
    want = int(1.25 * (k * (1.0 + math.log(max(longest / k, 1.0))) + segmented_candidate_buffer(k)))
    return max(1, min(longest, (want + 7) & ~7))


def distinct_segmented_candidates(hashes, offsets, k: int, seed: int, stream_base: int = 0, cap=None, stream_ids=None,
                                  state=None):
    """The hash-only candidate pass of Sampler.distinct for any B over S segments in one launch.

    hashes: int64 device tensor, hash(map(x)) per element; offsets int64 (B + 1,).  state: None (stateless: one
    empty row per segment, and no stream_ids) or (shadow_hashes (S, k), shadow_counts (S,), set_sizes (S,) | None,
    max_hashes (S,) | None), int64 device tensors of which the launch advances the first two in place.  Segment b goes into row stream_ids[b] (None: row b).  cap: candidates
    stored per segment; None takes segmented_candidate_cap(k, longest segment), which reads the offsets (one host
    wait).  Returns (pos (B, cap), hs (B, cap), counts (B,)) device tensors: the first min(counts[b], cap) entries
    of row b are the absolute positions, ascending, and scrambled hashes of the elements RandomValues seeded
    seed + stream_base + row could still admit; counts[b] > cap means segment b overflowed, its row was left as it
    was and a rerun with cap >= counts[b] returns exactly counts[b] candidates.  1 <= k <= 4096.
    """
    import torch

    L = N.load()
    if not (hashes.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("hashes and offsets must be device tensors")
    if hashes.dtype != torch.int64 or offsets.dtype != torch.int64 or hashes.dim() != 1:
        raise N.IllegalArgumentException("hashes must be 1-d int64 and offsets int64")
    dev = hashes.device
    offsets = offsets.contiguous()
    B = max(offsets.numel() - 1, 0)
    # an empty tensor has no address
    hashes = hashes.contiguous() if hashes.numel() else torch.empty(1, dtype=torch.int64, device=dev)
    if state is None:
        if stream_ids is not None:
            raise N.IllegalArgumentException("stream_ids= needs state=")
        state = (torch.empty((B, max(int(k), 0)), dtype=torch.int64, device=dev),
                 torch.zeros(B, dtype=torch.int64, device=dev), None, None)
    sh, sc, sizes, maxh = state
    if (sizes is None) != (maxh is None):
        raise N.IllegalArgumentException("set_sizes and max_hashes come together")
    S = sc.numel()
    for t, shape in ((sh, (S, k)), (sc, (S,)), (sizes, (S,)), (maxh, (S,)), (stream_ids, (B,))):
        if t is not None and (not t.is_cuda or t.dtype != torch.int64 or t.device != dev or tuple(t.shape) != shape
                              or not t.is_contiguous()):
            raise N.IllegalArgumentException("state and stream_ids must be contiguous int64 tensors on the hashes' "
                                             "device, shaped (S, k), (S,), (S,), (S,) and (B,)")
    if cap is None:
        cap = segmented_candidate_cap(k, int((offsets[1:] - offsets[:-1]).max()) if B else 1)
    cap = int(cap)
    pos = torch.empty((B, max(cap, 0)), dtype=torch.int64, device=dev)
    hs = torch.empty((B, max(cap, 0)), dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int64, device=dev)
    N.check(L.rsv_distinct_segmented_candidates(
        _ptr(hashes), _ptr(offsets), _ptr(stream_ids), B, S, k, seed & (2**64 - 1), stream_base & (2**64 - 1),
        _ptr(sh) if S else None, _ptr(sc) if S else None, _ptr(sizes), _ptr(maxh), _ptr(pos), _ptr(hs), cap,
        _ptr(counts), _stream_ptr(torch, dev)))
    return pos, hs, counts


class SegmentedObjectDistinct:
    """S long-lived Sampler.distinct streams over any hashable B (str, tuple, dataclass), one launch per batch.

    The engine reads hash(map(x)) only and returns per stream the positions the reference could still admit
    (distinct_segmented_candidates); one exact replica per row (values.RandomValues: heap, set, maxHash) is
    replayed over those elements alone.  Row r equals a single Sampler.distinct(k, key_type="object",
    seed=seed + stream_base + r) handle fed the same elements.  State: shadow_hashes (S, k), shadow_counts (S,),
    set_sizes (S,), max_hashes (S,) on the device, and the replicas on the host, created when a row is first named.
    map_fn: applied to the candidates only (None: the elements are the B's).  cap: candidates stored per segment
    (None: segmented_candidate_cap per batch).
    """

    def __init__(self, num_streams: int, k: int, seed: int, stream_base: int = 0, map_fn=None, cap=None, device=None):
        import torch

        from .values import LONG_MIN

        N.load()
        if num_streams < 0:
            raise N.IllegalArgumentException("negative stream count")
        if k <= 0:
            raise N.IllegalArgumentException("k out of range")
        if k > _SEG_DISTINCT_MAX_K:
            raise N.ReservoirError(
                f"SegmentedObjectDistinct holds k <= {_SEG_DISTINCT_MAX_K} per stream; use separate handles beyond")
        if cap is not None and cap < 1:
            raise N.IllegalArgumentException("cap must be at least 1")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise N.IllegalArgumentException("the state lives on the device")
        self.num_streams, self.k = int(num_streams), int(k)
        self.seed, self.stream_base = seed & (2**64 - 1), stream_base & (2**64 - 1)
        self._map, self._cap = map_fn, cap
        self.shadow_hashes = torch.empty((self.num_streams, self.k), dtype=torch.int64, device=dev)
        self.shadow_counts = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)
        self.set_sizes = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)
        self.max_hashes = torch.full((self.num_streams,), LONG_MIN, dtype=torch.int64, device=dev)
        self._values: dict = {}
        self._candidates = self._launches = self._reruns = 0

    def _state(self):
        return self.shadow_hashes, self.shadow_counts, self.set_sizes, self.max_hashes

    def _launch(self, torch, hashes, offsets, ids, cap):
        """One launch; returns per segment (positions, hashes) as host lists, None where the segment overflowed,
        and the counts."""
        pos, hs, counts = distinct_segmented_candidates(hashes, offsets, self.k, self.seed, self.stream_base, cap=cap,
                                                        stream_ids=ids, state=self._state())
        self._launches += 1
        cnt = counts.cpu()  # the first read-back
        fits = counts <= cap
        keep = (torch.arange(cap, device=pos.device)[None, :] < counts[:, None]) & fits[:, None]
        p, h = pos[keep].cpu().tolist(), hs[keep].cpu().tolist()  # the second
        out, a = [], 0
        for c in cnt.tolist():
            if c > cap:
                out.append(None)
            else:
                out.append((p[a:a + c], h[a:a + c]))
                a += c
        return out, cnt

    def update(self, elements, hashes, offsets, stream_ids=None, check_ids: bool = True):
        """Segment b = elements[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        elements: indexable; hashes: one int64 per element, hash(map(x)), a numpy array or a CUDA tensor; offsets
        and stream_ids: int64, numpy or tensors.  One launch over the batch, one read-back of the counts and one of
        the candidates; segments that overflowed cap are rerun once with the count they reported.  Every candidate
        is mapped before any replica changes; if that throws, the shadow rows the batch named are put back from a
        copy taken before the launch, the replicas are left as they were and the exception propagates: the batch
        never came.  ids as SegmentedDistinct.update.  Returns self.
        """
        import numpy as np
        import torch

        from .values import RandomValues

        dev = self.shadow_counts.device

        def on_device(t, what):
            return _host_or_device_i64(torch, t, what, dev)

        hashes, offsets = on_device(hashes, "hashes"), on_device(offsets, "offsets")
        B = offsets.numel() - 1
        if hashes.numel() != len(elements):
            raise N.IllegalArgumentException("one hash per element")
        if B <= 0 or self.num_streams == 0:
            return self
        if stream_ids is None:
            if B > self.num_streams:
                raise N.IllegalArgumentException("more segments than streams without stream_ids")
            ids = None
            rows = torch.arange(B, dtype=torch.int64)
        else:
            ids = on_device(stream_ids, "stream_ids")
            if ids.numel() != B:
                raise N.IllegalArgumentException("stream_ids must be an int64 tensor, one per segment")
            if check_ids:
                _check_stream_ids(torch, ids, self.num_streams)
            rows = ids.cpu()
        offs = offsets.cpu()
        lens = offs[1:] - offs[:-1]
        named = rows[(rows >= 0) & (rows < self.num_streams) & (lens > 0)]
        if named.numel() == 0:
            return self
        named_dev = named.to(dev)
        saved = self.shadow_hashes[named_dev], self.shadow_counts[named_dev]  # (indexing copies)
        cap = self._cap if self._cap is not None else segmented_candidate_cap(self.k, int(lens.max()))
        try:
            got, cnt = self._launch(torch, hashes, offsets, ids, cap)
            over = [b for b, g in enumerate(got) if g is None]
            if over:
                # the overflowed segments alone, each followed by the gap up to the next one under an id no
                # row has (the kernel skips it before it addresses anything)
                self._reruns += len(over)
                ob = torch.tensor(over, dtype=torch.int64)
                o2 = torch.stack([offs[ob], offs[ob + 1]], dim=1).reshape(-1)
                i2 = torch.stack([rows[ob], torch.full_like(ob, -1)], dim=1).reshape(-1)[:-1]
                again, _ = self._launch(torch, hashes, o2.to(dev), i2.to(dev), int(cnt[ob].max()))
                for j, b in enumerate(over):
                    got[b] = again[2 * j]
                    if got[b] is None:
                        raise N.ReservoirError("a rerun with the reported count overflowed: the state rows changed "
                                               "between the two launches")
            mp = self._map
            mapped = [[elements[i] if mp is None else mp(elements[i]) for i in g[0]] for g in got]
        except BaseException:
            self.shadow_hashes[named_dev] = saved[0]
            self.shadow_counts[named_dev] = saved[1]
            raise
        touched, sizes, maxh = [], [], []
        for b, (g, es) in enumerate(zip(got, mapped)):
            if not es:
                continue
            r = int(rows[b])
            v = self._values.get(r)
            if v is None:
                v = self._values[r] = RandomValues(self.k)
            for e, h in zip(es, g[1]):
                v.sample(e, h)
            self._candidates += len(es)
            touched.append(r)
            sizes.append(v.size)
            maxh.append(v.max_hash)
        if touched:
            t = torch.tensor(touched, dtype=torch.int64).to(dev)
            self.set_sizes[t] = torch.tensor(sizes, dtype=torch.int64).to(dev)
            self.max_hashes[t] = torch.tensor(maxh, dtype=torch.int64).to(dev)
        return self

    def result(self, r: int) -> list:
        """Row r's distinct elements, ascending by scrambled hash (RandomValues.result())."""
        if r < 0 or r >= self.num_streams:
            raise N.IllegalArgumentException(f"row outside [0, {self.num_streams})")
        v = self._values.get(int(r))
        return v.result() if v is not None else []

    def results(self) -> list:
        return [self.result(r) for r in range(self.num_streams)]

    def replica(self, r: int):
        """Row r's RandomValues, or None while no candidate of the row has been replayed."""
        return self._values.get(int(r))

    def info(self) -> dict:
        """What the engine returned so far: candidates replayed, launches made, segments rerun after an overflow."""
        return {"candidates": self._candidates, "launches": self._launches, "reruns": self._reruns}


_SEG_SAMPLE_STATE_MAX_K = 15104  # rsv_internal.h kSegSampleStateMaxK


class SegmentedSampler(_SegmentedState):
    """S long-lived Sampler.apply streams advanced by one launch per batch (K2 resumed).

    The state is three device tensors: keys (S, k); idx (S, k), the global index of each slot's
    last writer, -1 for an empty slot; next (S,), one past the highest index a row has consumed.
    Row s draws like a single "philox_r" Sampler with stream_id = stream_base + s.  Per slot the
    largest index wins, so a row fed its stream in any number of update() calls -- in order, or out
    of order with bases= -- or assembled by merge() from states that each saw a part of the stream,
    ends with the keys sample_segmented gives over the whole stream.  Only idx and next are filled:
    a slot with idx -1 is empty whatever its key holds.  Everything runs on torch's current stream.
    """

    _NAME, _TENSORS, _MAX_K = "SegmentedSampler", ("keys", "idx", "next"), _SEG_SAMPLE_STATE_MAX_K
    _SAME = "seed and stream_base"

    def _identity(self):
        return self.num_streams, self.k, self.seed, self.stream_base

    def __init__(self, num_streams: int, k: int, seed: int, stream_base: int = 0, dtype=None, device=None):
        import torch

        N.load()
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int64, torch.int32):
            raise N.IllegalArgumentException("keys must be int64/int32")
        dev = self._init_state(torch, num_streams, k, seed, stream_base, device)
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
        self._check_same_device(keys, offsets)
        keys, offsets = keys.contiguous(), offsets.contiguous()
        seg = self._segments(torch, offsets, check_ids, stream_ids, bases=bases)
        if seg is None:
            return self
        B, stream_ids, bases = seg
        N.check(L.rsv_sample_segmented_update(
            C.c_void_p(keys.data_ptr()), C.c_void_p(offsets.data_ptr()),
            C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
            C.c_void_p(bases.data_ptr()) if bases is not None else None,
            B, self.num_streams, keys.element_size(), self.k, self.seed, self.stream_base,
            C.c_void_p(self.keys.data_ptr()), C.c_void_p(self.idx.data_ptr()), C.c_void_p(self.next.data_ptr()),
            _stream_ptr(torch, self.keys.device)))
        return self

    def update_by_id(self, keys, ids):
        """The batch in arrival order, keys[i] into row ids[i]: group_by_stream, then one update launch.

        keys: a 1-D tensor of the state's dtype; ids: int64 or int32, one per key.  The grouping's order stands
        between the launch and the keys: only the at most k winning keys per row are read, through it, and no key
        is moved.  Every row continues at its own next, in arrival order.  There is no host wait and nothing to
        check: a row cannot repeat, and keys whose id lies outside [0, num_streams) are dropped.  Returns self.
        """
        import torch

        L = N.load()
        if not (keys.is_cuda and ids.is_cuda):
            raise N.IllegalArgumentException("keys and ids must be device tensors")
        if keys.dtype != self.keys.dtype or keys.dim() != 1:
            raise N.IllegalArgumentException("keys must be 1-D and have the state's dtype")
        grouped = self._group(torch, keys, ids)
        if grouped is None:
            return self
        offsets, order = grouped
        keys = keys.contiguous()
        S = self.num_streams
        N.check(L.rsv_sample_segmented_update_indirect(
            _ptr(keys), keys.numel(), _ptr(order), _ptr(offsets), None, None, S, S, keys.element_size(), self.k,
            self.seed, self.stream_base, _ptr(self.keys), _ptr(self.idx), _ptr(self.next),
            _stream_ptr(torch, self.keys.device)))
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
        return self._merge(torch, L.rsv_sample_segmented_merge, SegmentedSampler, (part_keys, part_idx, part_next))


SPLIT_LEN_DEFAULT = 1 << 18  # rsv_segmented.hip kSplitLenDefault (RSV_K2_SPLIT_LEN overrides it; 0: no split)


def sample_segmented_indexed(offsets, k: int, seed: int, stream_base: int = 0):
    """Sampler.apply over S streams whose elements stay with the caller: only their lengths reach the device.

    offsets: int64 device tensor (S + 1,); stream s has offsets[s+1] - offsets[s] elements.  Returns
    (idx[S, k], counts[S]) device tensors: idx[s, j] is the stream-relative index of the element slot j holds
    (-1: the slot is empty), counts[s] = min(len, k).  Stream s draws like a single "philox_r" Sampler with
    stream_id = stream_base + s.  Streams longer than the split length (RSV_K2_SPLIT_LEN) are taken in pieces
    over the whole device; the result does not depend on it.
    """
    import torch

    L = N.load()
    if not offsets.is_cuda or offsets.dtype != torch.int64:
        raise N.IllegalArgumentException("offsets must be an int64 device tensor")
    offsets = offsets.contiguous()
    S = offsets.numel() - 1
    idx = torch.empty((max(S, 0), k), dtype=torch.int64, device=offsets.device)  # (every slot is written)
    counts = torch.empty(max(S, 0), dtype=torch.int64, device=offsets.device)
    if S <= 0:
        return idx, counts
    N.check(L.rsv_sample_segmented_indexed(
        _ptr(offsets), S, k, seed & (2**64 - 1), stream_base & (2**64 - 1), _ptr(idx), _ptr(counts),
        _stream_ptr(torch, offsets.device)))
    return idx, counts


def _host_or_device_i64(torch, t, what, dev):
    """A 1-d int64 numpy array or tensor as a contiguous tensor on dev."""
    import numpy as np

    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int64))
    if t.dtype != torch.int64 or t.dim() != 1:
        raise N.IllegalArgumentException(f"{what} must be 1-d int64")
    return t.to(dev).contiguous()


def sample_segmented_objects(elements, offsets, k: int, seed: int, stream_base: int = 0, map_fn=None):
    """Sampler.apply for any B over S streams in one launch: stream s = elements[offsets[s]:offsets[s+1]].

    elements: indexable; offsets: int64, a numpy array or a tensor.  Returns a list of S lists, each stream's
    filled slots in slot order; map_fn runs on those elements only.  Stream s equals a single
    Sampler(k, seed=seed, stream_id=stream_base + s, key_type="object")(map_fn) fed the same elements.
    """
    import torch

    dev = offsets.device if hasattr(offsets, "is_cuda") and offsets.is_cuda else torch.device(
        "cuda", torch.cuda.current_device())
    offsets = _host_or_device_i64(torch, offsets, "offsets", dev)
    idx, _ = sample_segmented_indexed(offsets, k, seed, stream_base)
    starts = offsets.cpu().tolist()
    out = []
    for s, row in enumerate(idx.cpu().tolist()):
        picked = [elements[starts[s] + i] for i in row if i >= 0]
        out.append(picked if map_fn is None else [map_fn(e) for e in picked])
    return out


class SegmentedObjectSampler(_SegmentedState):
    """S long-lived Sampler.apply streams over any B (str, tuple, dataclass), one launch per batch.

    The engine sees the segments' lengths only.  The state is idx (S, k) and next (S,) on the device --
    SegmentedSampler's state without keys -- and one Python slot list per row on the host, created when a row
    is first named.  update() reads back, for each slot a segment replaced, the position of its new element
    inside the segment (hits) and stores map_fn(element) there; merge() reads back the part each slot came
    from (src).  Row r equals a single Sampler(k, seed=seed, stream_id=stream_base + r,
    key_type="object")(map_fn) fed the same elements.  Everything runs on torch's current stream.
    """

    _NAME, _TENSORS, _MAX_K = "SegmentedObjectSampler", ("idx", "next"), _SEG_SAMPLE_STATE_MAX_K
    _SAME = "seed and stream_base"
    _EMPTY = object()  # a slot no element has reached (map_fn may return None)

    def _identity(self):
        return self.num_streams, self.k, self.seed, self.stream_base

    def __init__(self, num_streams: int, k: int, seed: int, stream_base: int = 0, map_fn=None, device=None):
        import torch

        N.load()
        dev = self._init_state(torch, num_streams, k, seed, stream_base, device)
        self._map = map_fn
        self.idx = torch.full((self.num_streams, self.k), -1, dtype=torch.int64, device=dev)
        self.next = torch.zeros(self.num_streams, dtype=torch.int64, device=dev)
        self._slots: dict = {}

    @property
    def counts(self):
        """Filled slots per row (a device tensor)."""
        return (self.idx >= 0).sum(1)

    def update(self, elements, offsets, stream_ids=None, bases=None, check_ids: bool = True):
        """Segment b = elements[offsets[b]:offsets[b+1]] into row stream_ids[b] (None: row b).

        elements: indexable; offsets, stream_ids and bases: int64, numpy arrays or tensors.  bases, ids and the
        skipped segments as SegmentedSampler.update.  One launch; the hits are compacted on the device and read
        back once as (segment, slot, position).  Every hit element is mapped before any slot list changes: if
        the launch, the read-back or map_fn raises, the named rows' idx and next are put back from a copy taken
        before the launch, the slot lists are left as they were and the exception propagates: the batch never
        came.  last_hit_counts keeps the launch's hit_counts (B,) on the device.  Returns self.
        """
        import torch

        L = N.load()
        dev = self.idx.device
        offsets = _host_or_device_i64(torch, offsets, "offsets", dev)
        if stream_ids is not None:
            stream_ids = _host_or_device_i64(torch, stream_ids, "stream_ids", dev)
        if bases is not None:
            bases = _host_or_device_i64(torch, bases, "bases", dev)
        if stream_ids is None and offsets.numel() - 1 > self.num_streams:
            raise N.IllegalArgumentException("more segments than streams without stream_ids")
        seg = self._segments(torch, offsets, check_ids, stream_ids, bases=bases)
        if seg is None or self.num_streams == 0:
            return self
        B, stream_ids, bases = seg
        rows = stream_ids if stream_ids is not None else torch.arange(B, dtype=torch.int64, device=dev)
        # (ids the kernel skips fall on a row that then keeps what it has)
        named = rows.clamp(0, self.num_streams - 1)
        saved = self.idx[named], self.next[named]  # (indexing copies)
        hits = torch.empty((B, self.k), dtype=torch.int64, device=dev)
        hit_counts = torch.empty(B, dtype=torch.int64, device=dev)
        try:
            N.check(L.rsv_sample_segmented_indexed_update(
                _ptr(offsets), _ptr(stream_ids), _ptr(bases), B, self.num_streams, self.k, self.seed,
                self.stream_base, _ptr(self.idx), _ptr(self.next), _ptr(hits), _ptr(hit_counts),
                _stream_ptr(torch, dev)))
            at = (hits >= 0).nonzero()
            b, j = at[:, 0], at[:, 1]
            pos = hits[b, j]
            # the one read-back: (segment, slot, position), with the row and the element they name
            got = torch.stack([b, j, pos, rows[b], offsets[b] + pos]).cpu().tolist()
            mp = self._map
            mapped = [elements[e] if mp is None else mp(elements[e]) for e in got[4]]
        except BaseException:
            self.idx[named] = saved[0]
            self.next[named] = saved[1]
            raise
        self.last_hit_counts = hit_counts
        for r, j, v in zip(got[3], got[1], mapped):
            self._row(r)[j] = v
        return self

    def _row(self, r: int) -> list:
        lst = self._slots.get(r)
        if lst is None:
            lst = self._slots[r] = [self._EMPTY] * self.k
        return lst

    def result(self, r: int) -> list:
        """Row r's filled slots in slot order."""
        if r < 0 or r >= self.num_streams:
            raise N.IllegalArgumentException(f"row outside [0, {self.num_streams})")
        return [v for v in self._slots.get(int(r), ()) if v is not self._EMPTY]

    def results(self) -> list:
        return [self.result(r) for r in range(self.num_streams)]

    def merge(self, *others):
        """Per slot the largest idx among row r and row r of every other state wins, and the slot takes that
        state's element; next takes the max.  others: SegmentedObjectSampler objects of this state's shape, seed
        and stream_base.  One launch, one read-back of the part each slot came from.  Returns self."""
        import torch

        L = N.load()
        for o in others:
            if not isinstance(o, SegmentedObjectSampler) or o._identity() != self._identity():
                raise N.IllegalArgumentException(f"merge needs states of the same shape, {self._SAME}")
        dev = self.idx.device
        if any(o.idx.device != dev for o in others):
            raise N.IllegalArgumentException("parts must live on the state's device")
        if not others or self.num_streams == 0:
            return self
        part_idx = torch.stack([o.idx for o in others]).contiguous()
        part_next = torch.stack([o.next for o in others]).contiguous()
        src = torch.empty((self.num_streams, self.k), dtype=torch.int32, device=dev)
        N.check(L.rsv_sample_segmented_indexed_merge(
            _ptr(part_idx), _ptr(part_next), len(others), self.num_streams, self.k, _ptr(self.idx), _ptr(self.next),
            _ptr(src), _stream_ptr(torch, dev)))
        at = (src >= 0).nonzero()
        got = torch.stack([at[:, 0], at[:, 1], src[at[:, 0], at[:, 1]].to(torch.int64)]).cpu().tolist()
        for r, j, p in zip(*got):
            self._row(r)[j] = others[p]._slots[r][j]
        return self


def _seg_rows_inputs(torch, rows, offsets):
    """rows / offsets of a K2 call over byte keys, checked and contiguous; returns (rows, offsets, width)."""
    return _rows_inputs(torch, rows, offsets, (torch.uint8, torch.int64))


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


class SegmentedSamplerRows(_SegmentedState):
    """SegmentedSampler over fixed-width byte keys (java.util.UUID, case classes of primitives).

    The state is three device tensors: rows uint8 (S, k, width); idx (S, k), the global index of each
    slot's last writer, -1 for an empty slot; next (S,).  Row s draws like a single "philox_r"
    Sampler(k, key_type="bytesW") with stream_id = stream_base + s, and per slot the largest index wins:
    fed its stream in any number of update() calls -- in order, or out of order with bases= -- or
    assembled by merge(), a row ends with the rows sample_segmented_rows gives over the whole stream.
    Only idx and next are filled: a slot with idx -1 is empty whatever its row holds.  width: a multiple
    of 8 in 16..256.  Everything runs on torch's current stream.
    """

    _NAME, _LONG, _MAX_K = "SegmentedSamplerRows", "SegmentedSampler", _SEG_SAMPLE_STATE_MAX_K
    _TENSORS, _SAME = ("rows", "idx", "next"), "width, seed and stream_base"

    def _identity(self):
        return self.num_streams, self.k, self.width, self.seed, self.stream_base

    def __init__(self, num_streams: int, k: int, width: int, seed: int, stream_base: int = 0, device=None):
        import torch

        N.load()
        dev = self._init_state(torch, num_streams, k, seed, stream_base, device, width)
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
        self._check_same_device(rows, offsets)
        seg = self._segments(torch, offsets, check_ids, stream_ids, bases=bases)
        if seg is None:
            return self
        B, stream_ids, bases = seg
        N.check(L.rsv_sample_segmented_rows_update(
            C.c_void_p(rows.data_ptr()), C.c_void_p(offsets.data_ptr()),
            C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
            C.c_void_p(bases.data_ptr()) if bases is not None else None,
            B, self.num_streams, W, self.k, self.seed, self.stream_base,
            C.c_void_p(self.rows.data_ptr()), C.c_void_p(self.idx.data_ptr()), C.c_void_p(self.next.data_ptr()),
            _stream_ptr(torch, self.rows.device)))
        return self

    def update_by_id(self, rows, ids):
        """The batch in arrival order, rows[i] into row ids[i] of the state: as SegmentedSampler.update_by_id.

        rows: uint8 (n, width) or int64 (n, width / 8), as update() takes them; ids: int64 or int32, one per
        row.  Only the at most k winning rows per state row are read, through the grouping's order.  No host wait;
        rows whose id lies outside [0, num_streams) are dropped.  Returns self.
        """
        import torch

        L = N.load()
        if not (rows.is_cuda and ids.is_cuda):
            raise N.IllegalArgumentException("rows and ids must be device tensors")
        if rows.dim() != 2 or rows.dtype not in (torch.uint8, torch.int64):
            raise N.IllegalArgumentException("rows must be 2-D uint8 or int64 (one key per row)")
        if rows.shape[1] * rows.element_size() != self.width:
            raise N.IllegalArgumentException(f"rows must hold {self.width} bytes each")
        grouped = self._group(torch, rows, ids)
        if grouped is None:
            return self
        offsets, order = grouped
        rows = rows.contiguous()
        S = self.num_streams
        N.check(L.rsv_sample_segmented_rows_update_indirect(
            _ptr(rows), rows.shape[0], _ptr(order), _ptr(offsets), None, None, S, S, self.width, self.k,
            self.seed, self.stream_base, _ptr(self.rows), _ptr(self.idx), _ptr(self.next),
            _stream_ptr(torch, self.rows.device)))
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
        return self._merge(torch, L.rsv_sample_segmented_rows_merge, SegmentedSamplerRows,
                           (part_rows, part_idx, part_next))


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
