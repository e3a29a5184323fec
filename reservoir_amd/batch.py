"""Stateless batch entry points of the HIP engine over device tensors.

torch is used only for device memory and streams (plumbing); the compute runs in
libreservoir_hip.so.  Every function raises if the engine is unavailable.

    sample_segmented  -- K2: S independent samplers in one launch (one wave per stream)
    distinct_segmented -- K5: S independent Sampler.distinct streams in one launch (bottom-k per stream)
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
    if not (keys.is_cuda and offsets.is_cuda):
        raise N.IllegalArgumentException("keys and offsets must be device tensors")
    if keys.dtype not in (torch.int64, torch.int32) or offsets.dtype != torch.int64:
        raise N.IllegalArgumentException("keys must be int64/int32 and offsets int64")
    if hashes is not None:
        if not hashes.is_cuda or hashes.dtype != torch.int64 or hashes.numel() != keys.numel():
            raise N.IllegalArgumentException("hashes must be an int64 device tensor, one per key")
        kind = N.HASH_PRECOMPUTED
        # an empty tensor has no address; the engine wants one for precomputed hashes
        hashes = hashes.contiguous() if hashes.numel() else torch.empty(1, dtype=torch.int64, device=keys.device)
    elif hash in _SEG_HASH:
        kind = _SEG_HASH[hash]
    else:
        raise N.IllegalArgumentException(f"unknown hash {hash!r}")
    keys = keys.contiguous()
    offsets = offsets.contiguous()
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
