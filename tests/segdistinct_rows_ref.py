"""The numpy reference of the segmented-distinct GPU tests over byte keys (rsv_distinct_segmented_rows).

Per stream: the distinct rows u (W bytes = W / 8 little-endian 64-bit words), h = scramble(r0, r1, hash(u))
with segdistinct_ref's _scramble and (r0, r1) from its _r01, lexsort by (h, word 0, ..., word W/8 - 1 as
uint64), the first k.  The tests at the end (CPU only; tests/test_segdistinct_rows_ref.py collects them)
pin this restatement to oracle.DistinctRows -- rows, hashes and order -- and the numpy UUID.hashCode
to oracle.uuid_hashcode.
"""
import numpy as np
import pytest
from segdistinct_ref import _r01, _scramble

U64 = np.uint64
M64 = (1 << 64) - 1


def rows_of(ids, width, salt=0):
    """The width-byte key of element id: the splitmix stream of the id, one word per 8 bytes."""
    ids = np.asarray(ids, dtype=U64)
    out = np.empty((ids.size, width // 8), dtype=U64)
    for w in range(width // 8):
        z = ids * U64(0x9E3779B97F4A7C15) + U64(((w + salt) * 0x632BE59BD9B4E019 + 1) & M64)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        out[:, w] = z ^ (z >> U64(31))
    return out.view(np.uint8).reshape(ids.size, width)


def hashes_of(ids):
    """A 64-bit hash of the id: injective in practice."""
    return rows_of(ids, 8, salt=77).view(np.int64).reshape(-1)


def uuid_hashcode_np(rows):
    """java.util.UUID.hashCode of 16-byte rows [mostSigBits | leastSigBits], widened to int64."""
    w = np.ascontiguousarray(rows).view(U64).reshape(-1, 2)
    hilo = w[:, 0] ^ w[:, 1]
    return ((hilo >> U64(32)) ^ hilo).astype(np.uint32).astype(np.int32).astype(np.int64)


def expected_rows(rows, hashed, offs, k, r0, r1):
    """(out_rows uint8 [S, k, W], out_h int64 [S, k], counts int64 [S]) for all streams at once."""
    S = offs.size - 1
    W = rows.shape[1]
    lo, hi = int(offs[0]), int(offs[-1])
    sid = np.repeat(np.arange(S), np.diff(offs))
    words = np.ascontiguousarray(rows[lo:hi]).view(U64).reshape(hi - lo, W // 8)
    h = _scramble(r0[sid], r1[sid], hashed[lo:hi])
    order = np.lexsort(tuple(words[:, w] for w in range(W // 8 - 1, -1, -1)) + (h, sid))
    sid, h, words = sid[order], h[order], words[order]
    same = np.zeros(sid.size, dtype=bool)
    same[1:] = (sid[1:] == sid[:-1]) & (words[1:] == words[:-1]).all(axis=1)
    # equal rows carry equal hashes (the caller's contract), so the sort left them adjacent
    assert not (same[1:] & (h[1:] != h[:-1])).any()
    sid, h, words = sid[~same], h[~same], words[~same]
    rank = np.arange(sid.size) - np.searchsorted(sid, np.arange(S))[sid]
    sel = rank < k
    out_w = np.zeros((S, k, W // 8), dtype=U64)
    out_h = np.zeros((S, k), dtype=np.int64)
    out_w[sid[sel], rank[sel]] = words[sel]
    out_h[sid[sel], rank[sel]] = h[sel]
    return out_w.view(np.uint8).reshape(S, k, W), out_h, np.bincount(sid[sel], minlength=S).astype(np.int64)


def ragged_ids(rng, lens):
    """Per stream, ids drawn with replacement from a pool half its length (~50 % repeats); no id is
    shared between streams."""
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    ids = np.empty(int(offs[-1]), dtype=np.int64)
    for s, n in enumerate(lens):
        ids[offs[s]:offs[s + 1]] = offs[s] + rng.integers(0, max(1, n // 2), size=n)
    return ids, offs


@pytest.mark.parametrize("width,k,uuid", [(16, 64, False), (16, 5, True), (24, 300, False), (64, 1, False)])
def test_numpy_reference_equals_oracle_rows(oracle, width, k, uuid):
    """40 ragged streams of 0..900 rows: rows, hashes and order bit for bit against oracle.DistinctRows."""
    rng = np.random.default_rng(width + k)
    lens = rng.integers(0, 901, size=40)
    lens[:2] = [0, 1]
    ids, offs = ragged_ids(rng, lens)
    rows = rows_of(ids, width)
    hashed = uuid_hashcode_np(rows) if uuid else hashes_of(ids)
    seed, base = 31, 400
    r0, r1 = _r01(oracle, k, seed, base, lens.size)
    got_rows, got_h, got_n = expected_rows(rows, hashed, offs, k, r0, r1)
    for s in range(lens.size):
        ref = oracle.DistinctRows(k, seed + base + s, width, "uuid" if uuid else "precomputed")
        ref.sample_all(rows[offs[s]:offs[s + 1]], None if uuid else hashed[offs[s]:offs[s + 1]])
        want_rows, want_h = ref.result()
        m = int(got_n[s])
        assert m == want_rows.shape[0], s
        assert np.array_equal(got_rows[s, :m], want_rows) and np.array_equal(got_h[s, :m], want_h), s
        assert not got_rows[s, m:].any() and not got_h[s, m:].any(), s


def test_numpy_uuid_hashcode_equals_oracle(oracle):
    rows = rows_of(np.arange(200), 16)
    rows[:3].view(U64)[:] = [[0, 0], [M64, 5], [0x123456789ABCDEF0, 0x0FEDCBA987654321]]
    w = rows.view(np.int64).reshape(-1, 2)
    want = [oracle.uuid_hashcode(int(a), int(b)) for a, b in w]
    assert uuid_hashcode_np(rows).tolist() == want
