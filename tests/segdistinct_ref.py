"""The numpy reference of the segmented-distinct GPU tests (K5: stateless, update, merge).

Per stream: h = byteswap64(r1 ^ byteswap64(r0 ^ hash(u))) over its distinct keys u, lexsort((u, h))[:k],
with (r0, r1) the first two nextLong() of java.util.Random(seed + stream_base + s).
"""
import numpy as np

U64 = np.uint64
G = U64(0x9E3779B97F4A7C15)
WAVE_MAX_K = 256  # rsv_internal.h kSegDistinctWaveMaxK


def _bs(v):
    return (v * G).byteswap() * G  # uint64 arrays wrap


def _scramble(r0, r1, hashed):
    return _bs(r1.astype(U64) ^ _bs(r0.astype(U64) ^ hashed.astype(U64))).astype(np.int64)


def _wrap(v: int) -> int:
    v &= 2**64 - 1
    return v - 2**64 if v >= 2**63 else v


def _r01_np(seeds):
    """java.util.Random(seed): the first two nextLong(), vectorised (checked against the oracle below)."""
    mul, mask = U64(0x5DEECE66D), U64((1 << 48) - 1)
    st = (np.asarray(seeds).astype(U64) ^ mul) & mask
    w = []
    for _ in range(4):
        st = (st * mul + U64(0xB)) & mask
        w.append((st >> U64(16)).astype(np.uint32).astype(np.int32).astype(np.int64).astype(U64))
    return ((w[0] << U64(32)) + w[1]).astype(np.int64), ((w[2] << U64(32)) + w[3]).astype(np.int64)


def _r01(oracle, k, seed, stream_base, S):
    seeds = [_wrap(seed + stream_base + s) for s in range(S)]
    if S > 1000:  # the oracle pins the first streams, numpy restates the generator for the rest
        r0, r1 = _r01_np(np.array(seeds, dtype=np.int64))
        for s in range(64):
            d = oracle.Distinct(k, seeds[s], oracle.HASH_IDENTITY)
            assert (d.r0, d.r1) == (int(r0[s]), int(r1[s]))
        return r0, r1
    ds = [oracle.Distinct(k, sd, oracle.HASH_IDENTITY) for sd in seeds]
    return np.array([d.r0 for d in ds], dtype=np.int64), np.array([d.r1 for d in ds], dtype=np.int64)


def _expected(keys, hashed, offs, k, r0, r1):
    """Per stream lexsort((u, h))[:k] over its distinct keys u, for all streams at once."""
    S = offs.size - 1
    sid = np.repeat(np.arange(S), np.diff(offs))
    kk = keys[offs[0]:offs[-1]].astype(np.int64)
    h = _scramble(r0[sid], r1[sid], hashed[offs[0]:offs[-1]])
    order = np.lexsort((kk, h, sid))
    sid, h, kk = sid[order], h[order], kk[order]
    keep = np.ones(kk.size, dtype=bool)
    keep[1:] = (sid[1:] != sid[:-1]) | (kk[1:] != kk[:-1])  # equal keys of a stream are adjacent (equal h)
    sid, h, kk = sid[keep], h[keep], kk[keep]
    rank = np.arange(sid.size) - np.searchsorted(sid, np.arange(S))[sid]
    sel = rank < k
    out_k = np.zeros((S, k), dtype=np.int64)
    out_h = np.zeros((S, k), dtype=np.int64)
    out_k[sid[sel], rank[sel]] = kk[sel]
    out_h[sid[sel], rank[sel]] = h[sel]
    return out_k, out_h, np.bincount(sid[sel], minlength=S).astype(np.int64)


def _hash_np(keys, kind):
    v = keys.astype(np.int64)
    if kind == "java_long":
        u = v.view(U64)
        return ((u ^ (u >> U64(32))) & U64(0xFFFFFFFF)).astype(np.uint32).astype(np.int32).astype(np.int64)
    if kind == "java_int":
        return v.astype(np.int32).astype(np.int64)
    return v


def _with_repeats(rng, fresh, offs):
    """Each stream draws with replacement from a pool half its length."""
    keys = np.empty_like(fresh)
    for s in range(offs.size - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        if b > a:
            pool = fresh[a:a + max(1, (b - a) // 2)]
            keys[a:b] = pool[rng.integers(0, pool.size, size=b - a)]
    return keys
