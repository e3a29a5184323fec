"""``Sampler.distinct[A, B]`` for any ``B`` (a str, a tuple, a dataclass: anything hashable) over the
HIP engine's hash-only candidate pass -- the Python counterpart of
bindings/scala/core/.../gpu/ObjectDistinct.scala.

The engine never sees a ``B``.  It reads ``hash(map(x))`` (8 bytes per element) and returns the
batch positions the reference could still admit (rsv_distinct_candidates, include/reservoir_hip.h);
the exact ``RandomValues`` replica (reservoir_amd/values.py: heap, set, maxHash) is replayed over
those elements only, and its size and maxHash go back to the engine with the commit.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Iterable

import numpy as np

from . import _native as N
from ._native import IllegalArgumentException, IllegalStateException
from .values import RandomValues


def _as_long(v) -> int:
    """``hash: B => Long``: wrap a Python int to a signed 64-bit value."""
    v = int(v) & (2**64 - 1)
    return v - 2**64 if v >= 2**63 else v


class ObjectDistinct:
    """A distinct sampler whose elements stay on the host (one index-only C-ABI handle)."""

    _BATCH = 65536  # elements buffered by sample() per engine batch

    def __init__(self, max_sample_size: int, map_fn: Callable, hash_fn: Callable, *, reusable: bool,
                 seed: int | None = None, device: int | None = None):
        from .sampler import _fresh_seed

        self._L = N.load()
        self._map = map_fn
        self._hash = hash_fn
        self._k = max_sample_size
        self._reusable = bool(reusable)
        cfg = N.RsvConfig()
        N.check(self._L.rsv_config_init(C.byref(cfg)))
        cfg.kind = N.KIND_DISTINCT
        cfg.max_sample_size = max_sample_size
        cfg.key_width = 8  # ignored: the handle never holds keys
        cfg.reusable = 1 if reusable else 0
        cfg.hash_kind = N.HASH_PRECOMPUTED
        cfg.device = -1 if device is None else int(device)
        cfg.seed = (_fresh_seed() if seed is None else int(seed)) & (2**64 - 1)
        self.seed = cfg.seed
        h = C.c_void_p()
        N.check(self._L.rsv_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._stream = int(self._L.rsv_get_stream(h) or 0)
        self._values = RandomValues(max_sample_size)
        self._elems: list = []   # sample(): mapped elements and their hashes, not yet sent
        self._hashes: list = []
        self._final_count = 0
        self._candidates = 0
        self._batches = 0

    # -- lifecycle ----------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._final_count = self.count
            self._L.rsv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def is_open(self) -> bool:
        return self._h is not None and bool(self._L.rsv_is_open(self._h))

    isOpen = is_open

    @property
    def count(self) -> int:
        if self._h is None:
            return self._final_count
        return int(self._L.rsv_count(self._h)) + len(self._elems)

    @property
    def max_sample_size(self) -> int:
        return self._k

    @property
    def is_distinct(self) -> bool:
        return True

    def _check_open(self) -> None:
        if not self.is_open:
            raise IllegalStateException("use of sampler after calling `result()`")

    # -- the candidate protocol ---------------------------------------------------------------
    def _batch(self, hashes_ptr, n: int, mem: int, elem_at: Callable[[int], Any]) -> None:
        """One engine batch: candidates by hash, their elements through ``elem_at(offset)`` (all of
        them before the replica changes), replay, commit.  A throwing ``elem_at`` aborts the batch."""
        nc = C.c_int64(0)
        N.check(self._L.rsv_distinct_candidates(self._h, hashes_ptr, n, mem, C.byref(nc)))
        try:
            c = nc.value
            offs = np.empty(max(c, 1), dtype=np.int64)
            hs = np.empty(max(c, 1), dtype=np.int64)
            N.check(self._L.rsv_candidates_read(self._h, offs.ctypes.data_as(C.c_void_p),
                                                hs.ctypes.data_as(C.c_void_p), c))
            elems = [elem_at(o) for o in offs[:c].tolist()]
        except BaseException:
            N.check(self._L.rsv_candidates_abort(self._h))
            raise
        v = self._values
        for e, h in zip(elems, hs[:c].tolist()):
            v.sample(e, h)
        N.check(self._L.rsv_candidates_commit(self._h, v.size, v.max_hash))
        self._candidates += c
        self._batches += 1

    def _flush(self) -> None:
        n = len(self._elems)
        if not n:
            return
        elems, self._elems = self._elems, []
        hs = np.array(self._hashes, dtype=np.int64)
        self._hashes = []
        self._batch(hs.ctypes.data_as(C.c_void_p), n, N.MEM_HOST, elems.__getitem__)

    # -- Sampler trait ------------------------------------------------------------------------
    def sample(self, element: Any) -> None:
        """Sampler.sample (Sampler.scala:37-38, :394-409)."""
        self._check_open()
        b = self._map(element)
        h = _as_long(self._hash(b))
        self._elems.append(b)
        self._hashes.append(h)
        if len(self._elems) == self._BATCH:
            self._flush()

    def sample_all(self, elements: Iterable, hashes=None) -> None:
        """Sampler.sampleAll (Sampler.scala:49-50).  Without ``hashes`` every element is mapped and
        hashed and the whole sequence goes as one engine batch.  With ``hashes`` -- one int64 per
        element of an indexable ``elements``, a numpy array or a CUDA tensor, equal to
        ``hash(map(x))`` -- only the candidates are mapped; a throwing ``map`` then drops the batch
        and leaves the sampler as it was."""
        self._check_open()
        self._flush()
        if hashes is None:
            elems = [self._map(x) for x in elements]
            if not elems:
                return
            hs = np.fromiter((_as_long(self._hash(b)) for b in elems), dtype=np.int64, count=len(elems))
            self._batch(hs.ctypes.data_as(C.c_void_p), len(elems), N.MEM_HOST, elems.__getitem__)
            return
        n = len(elements)

        def mapped(o: int):
            return self._map(elements[o])

        t = type(hashes)
        if t.__module__.startswith("torch") and t.__name__ == "Tensor":
            import torch

            if not hashes.is_cuda or hashes.dtype != torch.int64 or hashes.dim() != 1:
                raise IllegalArgumentException("hashes must be a 1-d int64 numpy array or CUDA tensor")
            if hashes.numel() != n:
                raise IllegalArgumentException("one hash per element")
            hv = hashes if hashes.is_contiguous() else hashes.contiguous()
            cur = torch.cuda.current_stream(hv.device)
            if cur.cuda_stream != self._stream:  # produced on torch's stream: order this handle's after it
                ev = torch.cuda.Event()
                ev.record(cur)
                torch.cuda.ExternalStream(self._stream, device=hv.device).wait_event(ev)
            # (the call returns with its device work done: hv needs no record_stream)
            self._batch(C.c_void_p(hv.data_ptr()), n, N.MEM_DEVICE, mapped)
            return
        hs = np.ascontiguousarray(np.asarray(hashes), dtype=np.int64)
        if hs.ndim != 1 or hs.size != n:
            raise IllegalArgumentException("one hash per element")
        self._batch(hs.ctypes.data_as(C.c_void_p), n, N.MEM_HOST, mapped)

    sampleAll = sample_all

    def result(self) -> list:
        """Sampler.result (Sampler.scala:59-60, :411): the distinct elements, ascending by scrambled
        hash.  A single-use sampler closes."""
        self._check_open()
        self._flush()
        out = self._values.result()
        if not self._reusable:
            self.close()
        return out

    def distinct_info(self) -> dict:
        """The replica's set size and maxHash, and what the engine returned so far."""
        return {"size": self._values.size, "max_hash": self._values.max_hash, "ordered": 1,
                "candidates": self._candidates, "batches": self._batches, "pending": len(self._elems)}
