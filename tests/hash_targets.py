"""Planting keys at chosen scrambled hashes, and the host mirror of the set merge's bucket map.

RandomValues scrambles an element's hash as h = byteswap64(r1 ^ byteswap64(r0 ^ hash)) with
byteswap64(v) = bswap64(v * G) * G (mod 2^64, G odd): a bijection on 64-bit words.  Its inverse gives
the hash value whose scrambled hash is exactly t:

    inv_byteswap64(y) = bswap64(y * INV) * INV,  INV = G^-1 mod 2^64
    unscramble(r0, r1, t) = r0 ^ inv_byteswap64(r1 ^ inv_byteswap64(t))

A Long key with the identity hash IS its hash value, so the preimage is the key; any other key type
carries the preimage as a precomputed hash (which also allows ties on purpose).
"""
import numpy as np

MIN, MAX = -(2**63), 2**63 - 1
M64 = 2**64 - 1
G = 0x9E3779B97F4A7C15
INV = pow(G, -1, 2**64)
EDGES = (MIN, MIN + 1, MIN + 2, MIN + 200, -1, 0, MAX - 1, MAX)


def _signed(v: int) -> int:
    v &= M64
    return v - 2**64 if v >= 2**63 else v


def _bswap64(v: int) -> int:
    return int.from_bytes((v & M64).to_bytes(8, "little"), "big")


def inv_byteswap64(y: int) -> int:
    return (_bswap64((y & M64) * INV) * INV) & M64


def unscramble(r0: int, r1: int, t: int) -> int:
    """The hash value that (r0, r1) scramble to exactly t, as a signed 64-bit int."""
    return _signed((r0 & M64) ^ inv_byteswap64((r1 & M64) ^ inv_byteswap64(t)))


def plant(r0: int, r1: int, targets) -> np.ndarray:
    """Preimages of the scrambled hashes `targets` (any iterable of ints) as an int64 array."""
    return np.array([unscramble(r0, r1, int(t)) for t in targets], dtype=np.int64)


def r01(oracle, seed: int):
    d = oracle.Distinct(1, seed, oracle.HASH_IDENTITY)
    return d.r0, d.r1


def bucket_log(total: int, log_bmax: int = 31) -> int:
    """rsv_distinct.hip bucket_log: the smallest lb with 2^(lb + 7) >= total (capped at log_bmax)."""
    lb = 0
    while lb < log_bmax and (1 << (lb + 7)) < total:
        lb += 1
    return lb


def bucket_nobound(h, lb: int) -> np.ndarray:
    """rsv_distinct.hip BucketMap for the merge without a bound (top = Long.MaxValue: span = 2^64 - 1,
    q = 1, mult = 1 << lb): bucket = umulhi(u, 2^lb) = u >> (64 - lb) with u = h - Long.MinValue.

    With a bound `top` the map is: span = top - Long.MinValue, q = floor((2^64 - 1) / (span + 1));
    when q >> (64 - lb) != 0 (that is span + 1 < 2^lb) the bucket is u itself (the direct branch,
    `direct_branch` below), else umulhi(u, q << lb); either way clamped to 2^lb - 1, and 0 for lb = 0.
    """
    u = np.atleast_1d(np.asarray(h, dtype=np.int64)).view(np.uint64) ^ np.uint64(1 << 63)
    if lb == 0:
        return np.zeros(u.size, dtype=np.int64)
    return (u >> np.uint64(64 - lb)).astype(np.int64)


def direct_branch(top: int, lb: int) -> bool:
    """Whether the bounded BucketMap takes `b = u` (mult = 0 with lb > 0) for entries <= top."""
    span = top - MIN
    q = 1 if span == M64 else M64 // (span + 1)
    return lb > 0 and (q >> (64 - lb)) != 0
