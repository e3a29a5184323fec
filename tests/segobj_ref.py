"""The host reference of the segmented object-distinct tests (rsv_distinct_segmented_candidates).

Per stream, (r0, r1) and the scrambled hashes are segdistinct_ref's.  On top of them: the reference's own
admissions and replica (RandomValues over the whole stream), the replay of a candidate list, and the exact
running T -- the k-th smallest distinct scrambled hash among the elements before a position -- that the
tightness bound is stated against.
"""
import bisect

import numpy as np
from segdistinct_ref import _r01, _scramble

MAX = 2**63 - 1
# rsv_segdistinct.hip, with_form_of: (largest k, team size NT, candidate buffer W)
FORMS = ((64, 64, 256), (256, 64, 512), (1024, 256, 2048), (4096, 1024, 8192))


def form_of(k):
    return next((nt, w) for top, nt, w in FORMS if k <= top)


def scrambled(oracle, k, seed, stream_base, hashed, offs, rows=None):
    """h per element: segment b scrambled with the (r0, r1) of row rows[b] (None: row b)."""
    B = offs.size - 1
    rows = np.arange(B) if rows is None else np.asarray(rows)
    top = int(rows.max()) + 1 if B else 0
    r0, r1 = _r01(oracle, k, seed, stream_base, top)
    sid = np.repeat(rows, np.diff(offs))
    return _scramble(r0[sid], r1[sid], hashed[offs[0]:offs[-1]])


def admissions(k, ids, sh, v=None):
    """RandomValues over the stream (ids: the elements, sh: their scrambled hashes), from the replica v or an
    empty one: the positions it admits, and the replica."""
    from reservoir_amd.values import RandomValues

    v = RandomValues(k) if v is None else v
    adm = []
    for i, (e, h) in enumerate(zip(ids.tolist() if hasattr(ids, "tolist") else ids, sh.tolist())):
        if v.admits(e, h):
            adm.append(i)
            v.sample(e, h)
    return np.array(adm, dtype=np.int64), v


def replay(k, ids, sh, positions, v=None):
    """RandomValues over the elements at `positions` alone, in that order."""
    from reservoir_amd.values import RandomValues

    v = RandomValues(k) if v is None else v
    for p in np.asarray(positions).tolist():
        v.sample(ids[p].item() if hasattr(ids[p], "item") else ids[p], int(sh[p]))
    return v


def same_replica(a, b):
    """Heap array order (elements and hashes) and maxHash."""
    return a.heap() == b.heap() and a.max_hash == b.max_hash


def running_T(k, sh):
    """T[j] for j in 0..n: the k-th smallest distinct h among sh[:j], MAX + 1 (above every hash: the open prefix)
    while fewer than k distinct values have been seen."""
    out = np.empty(sh.size + 1, dtype=object)
    low, seen = [], set()  # the k smallest distinct values so far, ascending
    for j, h in enumerate(sh.tolist()):
        out[j] = low[-1] if len(low) == k else MAX + 1
        if h not in seen and (len(low) < k or h < low[-1]):
            seen.add(h)
            bisect.insort(low, h)
            if len(low) > k:
                seen.discard(low.pop())
    out[sh.size] = low[-1] if len(low) == k else MAX + 1
    return out


def running_T_brute(k, sh):
    out = np.empty(sh.size + 1, dtype=object)
    for j in range(sh.size + 1):
        d = sorted(set(sh[:j].tolist()))
        out[j] = d[k - 1] if len(d) >= k else MAX + 1
    return out


def rows16(ids):
    """The element ids as 16-byte rows [id | ~id]: what oracle.DistinctRows takes as keys."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack([ids, ~ids], axis=1).view(np.uint8)
