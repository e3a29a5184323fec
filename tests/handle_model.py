"""A plain model of one rsv_sampler handle (include/reservoir_hip.h), and the seeded operation programs
run against it (tests/test_gpu_handle_programs.py; the model itself is checked in
tests/test_handle_model.py).  Pure Python and numpy over the oracle: nothing of the engine is imported.

Keys are a function of the element's global index, so the content of any index range is known without
storing a stream:
    long     splitmix64(KEY_BASE + i)                      (oracle.splitmix_keys(KEY_BASE + lo, n))
    int      its low 32 bits
    bytesN   tests/wide_rows.py _rows(i, N)
Distinct streams repeat: element i carries the key of id i % period, so every batch longer than the
period holds duplicates; the "collide" family folds Long.hashCode to a few values, so the boundary hash
bucket ties and the reference's arrival order decides it (RSV_DISTINCT_ORDERED).

Elements model (both engines): per slot the global index of its writer (-1: none) and a count.
    philox_r  appending [lo, lo + n) sets each slot to the later of its writer and
              oracle.algo_r_last_writers(seed, stream_id, k, lo, n); seek(i) sets the count; a merge takes
              the larger index per slot and count = max(count, total_count)
    java_l    oracle.AlgoL fed the global indices as its values: its reservoir is the writer table
    result()  the keys of the first min(count, k) slots, zeros where a slot has no writer
An aborted index-only batch is never shown to the model (rsv_abort_indexed's contract).

Distinct model: oracle.Distinct fed the same key sequence; a set-mode merge under an injective hash is
the bottom-k of the union, which feeding the sibling's set to the same oracle object gives.

Lifecycle states (the rows of tests/test_gpu_handle_states.py): STATES below.
"""
import numpy as np

from wide_rows import _rows

STATES = ("fresh", "holding", "staged", "owed", "external", "cand_idle", "cand_pending", "closed", "taken")
KEY_BASE = 0x5EED

_M = np.uint64(2**64 - 1)


def splitmix_at(idx):
    """splitmix64(KEY_BASE + i) for an array of indices (oracle.splitmix_keys at scattered indices)."""
    with np.errstate(over="ignore"):
        z = np.asarray(idx, dtype=np.int64).astype(np.uint64) + np.uint64(KEY_BASE) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return (z ^ (z >> np.uint64(31))).view(np.int64)


def key_width(key_type):
    return {"long": 8, "int": 4}.get(key_type) or int(key_type[5:])


def keys_at(key_type, idx):
    """Element keys at the global indices idx: int64 / int32 arrays, or (n, N) uint8 rows."""
    idx = np.asarray(idx, dtype=np.int64)
    if key_type == "long":
        return splitmix_at(idx)
    if key_type == "int":
        return splitmix_at(idx).astype(np.int32)
    return _rows(idx, key_width(key_type))


def keys_range(key_type, lo, n):
    return keys_at(key_type, np.arange(lo, lo + n, dtype=np.int64))


def distinct_period(k):
    return 3 * k + 11


def distinct_keys(hash_name, k, lo, n):
    """Keys of a distinct stream's elements [lo, lo + n): ids repeat with distinct_period(k)."""
    ids = np.arange(lo, lo + n, dtype=np.int64) % distinct_period(k)
    x = splitmix_at(ids)
    if hash_name == "identity":
        return x
    if hash_name == "int":
        return x.astype(np.int32)
    # "collide": Long.hashCode = hi ^ lo folded to max(2, 3k/2) values
    u = x.view(np.uint64)
    hi = u >> np.uint64(32)
    c = u % np.uint64(max(2, 3 * k // 2))
    return ((hi << np.uint64(32)) | ((hi ^ c) & np.uint64(0xFFFFFFFF))).view(np.int64)


class ElementsModel:
    def __init__(self, O, engine, k, seed, stream_id, key_type):
        self.O, self.engine, self.k, self.seed, self.sid, self.key_type = O, engine, k, seed, stream_id, key_type
        self.count = 0
        self.writers = np.full(k, -1, dtype=np.int64)
        self._l = O.AlgoL(k, seed) if engine == "java_l" else None

    def append(self, n):
        """The n elements at global indices [count, count + n)."""
        if n <= 0:
            return
        lo = self.count
        if self._l is not None:
            self._l.sample_all(np.arange(lo, lo + n, dtype=np.int64))
            r = self._l.result()
            self.writers[: r.size] = r
        else:
            self.writers = np.maximum(self.writers, self.O.algo_r_last_writers(self.seed, self.sid, self.k, lo, n, 1))
        self.count = lo + n

    def seek(self, index):
        assert self._l is None and index >= self.count
        self.count = index

    def merge(self, other_writers, total_count):
        self.writers = np.maximum(self.writers, np.asarray(other_writers, dtype=np.int64))
        self.count = max(self.count, total_count)

    def offsets(self, n):
        """philox_r: what rsv_sample_indexed reports for the next n elements (before append(n))."""
        w = self.O.algo_r_last_writers(self.seed, self.sid, self.k, self.count, n, 1)
        return np.where(w > self.writers, w - self.count, -1)

    def keys(self):
        """All k slot keys, zeros where a slot has no writer."""
        w = self.writers
        out = keys_at(self.key_type, np.maximum(w, 0))
        out[w < 0] = 0
        return out

    def result(self):
        return self.keys()[: min(self.count, self.k)]


class DistinctModel:
    HASH = {"identity": "HASH_IDENTITY", "collide": "HASH_JAVA_LONG", "int": "HASH_JAVA_INT"}

    def __init__(self, O, hash_name, k, seed):
        self.O, self.hash_name, self.k, self.seed = O, hash_name, k, seed
        self.count = 0
        self._d = O.Distinct(k, seed, getattr(O, self.HASH[hash_name]))

    def append(self, n):
        if n <= 0:
            return
        self._d.sample_all(distinct_keys(self.hash_name, self.k, self.count, n).astype(np.int64))
        self.count += n

    def seek(self, index):  # a sibling's later range: the model only, a distinct handle has no seek
        self.count = index

    def merge(self, other_keys, total_count):
        self._d.sample_all(np.asarray(other_keys, dtype=np.int64))
        self.count = max(self.count, total_count)

    def result(self):
        return np.sort(self._d.result()[0])


# ---- the operation programs -----------------------------------------------------------------------
ELEMENT_FAMILIES = tuple(f"el-{kt}-{e}" for kt in ("long", "int", "bytes24") for e in ("philox_r", "java_l"))
DISTINCT_FAMILIES = ("di-identity", "di-collide", "di-int")
FAMILIES = ELEMENT_FAMILIES + DISTINCT_FAMILIES
KS = (1, 7, 64, 300, 2048, 2049, 8192, 8193)
BIG_K = 140_000  # k x 8 B above the runtime's kPublishMaxBytes: result() through the pinned copy

def seeds_of(family):
    """The committed seed list: as long as tests/test_handle_model.py's coverage conditions need (the
    philox_r alphabet is the widest, and its seeks and merges leave the fill phase early)."""
    if family.startswith("el-"):
        return tuple(range(1, 105 if family.endswith("philox_r") else 57))
    return tuple(range(1, 65))


BIG_SEEDS = (1001,)  # one k = BIG_K program per elements family

SAMPLING_OPS = ("sample", "stage", "host", "device", "device_torch", "indexed", "indexed_abort")
ELEMENT_OPS = SAMPLING_OPS + ("seek", "result", "result_device", "export_state", "export_packed", "merge_state",
                              "merge_packed", "merge_zero_state", "merge_zero_packed", "synchronize", "recreate")
DISTINCT_OPS = ("sample", "stage", "host", "device", "device_torch", "result", "distinct_info", "export_packed",
                "merge_packed", "export_state", "merge_state", "set_stream", "recreate")


def family_ops(family):
    """The family's alphabet: seek and merges are philox_r's; merges of distinct are set mode's."""
    if family.startswith("el-"):
        if family.endswith("java_l"):
            return tuple(o for o in ELEMENT_OPS if o != "seek" and not o.startswith("merge"))
        return ELEMENT_OPS
    if family == "di-collide":
        return tuple(o for o in DISTINCT_OPS if not o.startswith("merge"))
    return DISTINCT_OPS


def program_ids():
    out = [(f, s) for f in FAMILIES for s in seeds_of(f)]
    out += [(f, s) for f in ELEMENT_FAMILIES for s in BIG_SEEDS]
    return out


def _size(rng, k, count, cap=1 << 17):
    """A batch size: empty, one, below what is left of the fill, across k, up to cap."""
    c = int(rng.integers(0, 8))
    left = k - count
    if c == 0:
        return 0
    if c == 1:
        return 1
    if c in (2, 3, 7) and left > 4:
        return int(rng.integers(1, max(2, left // 4)))
    if c == 4 and 0 < left < cap:
        return min(cap, left + int(rng.integers(0, 2 * k + 2)))
    if c == 5:
        return int(rng.integers(1, min(cap, 4 * k + 64) + 1))
    if c == 6:
        return cap
    return int(rng.integers(1, cap + 1))


def gen_program(family, seed):
    """{"family", "seed", "k", "reusable", "ops"}: 12-20 operations, each a tuple (kind, args...) with
    every size and index written out, then ("final", how) -- how the program ends: "result" / "take"
    (single-use: rsv_result / rsv_result_take where the result is published), "external" (elements: an
    index-only batch accepted with rsv_commit_indexed) or "none" (reusable)."""
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    big = seed in BIG_SEEDS
    k = BIG_K if big else KS[(seed + FAMILIES.index(family)) % len(KS)]
    reusable = bool(seed % 2)
    elements = family.startswith("el-")
    alphabet = [o for o in family_ops(family) if reusable or o not in ("result", "result_device")]
    alphabet += [o for o in alphabet if o in ("result", "result_device")]  # (half the programs have none)
    ops = []
    count = 0
    n_ops = int(rng.integers(12, 21))
    while len(ops) < n_ops:
        op = alphabet[int(rng.integers(0, len(alphabet)))]
        if op == "sample":
            m = int(rng.integers(1, 301))
            ops.append((op, m))
            count += m
        elif op == "stage":
            m = int(rng.integers(0, 4)) and int(rng.integers(1, 5001))
            if count < k and rng.integers(0, 2):
                m = min(m, max(0, (k - count) // 3))
            ops.append((op, m))
            count += m
        elif op in ("host", "device", "device_torch", "indexed"):
            m = _size(rng, k, count)
            ops.append((op, m))
            count += m
        elif op == "indexed_abort":
            ops.append((op, max(1, _size(rng, k, count))))
        elif op == "seek":
            c = int(rng.integers(0, 6))
            if c in (0, 4, 5) and count < k - 1:
                t = int(rng.integers(count, k))  # within the fill phase
            elif c == 1:
                t = max(count, k) + int(rng.integers(0, k + 2))  # across k
            elif c == 2:
                t = count + (1 << 33) + int(rng.integers(0, 1000))  # far past it
            else:
                t = count + int(rng.integers(0, 500))
            ops.append((op, t - count))  # relative: a "throwing" batch that changes no slot counts
            count = t
        elif op in ("merge_state", "merge_packed"):
            gap, m = int(rng.integers(0, 2000)), _size(rng, k, count, 1 << 15)
            if count + 8 < k and rng.integers(0, 2):  # a sibling range that leaves the fill phase open
                gap = int(rng.integers(0, (k - count) // 4))
                m = min(m, (k - count) // 4)
            ops.append((op, gap, m))
            count += gap + m
        elif op in ("merge_zero_state", "merge_zero_packed"):
            t = count + (max(0, k - count) if rng.integers(0, 2) else 0) + int(rng.integers(0, 50))
            ops.append((op, t - count))
            count = t
        elif op == "recreate":
            ops.append((op,))
            count = 0
        else:
            ops.append((op,))
    if reusable:
        final = "none"
    else:
        final = ("result", "take", "external")[int(rng.integers(0, 3 if elements else 2))]
    ops.append(("final", final) if final != "external" else ("final", final, max(1, _size(rng, k, count))))
    return {"family": family, "seed": seed, "k": k, "reusable": reusable, "ops": ops,
            "checks": rng.integers(0, 2, size=len(ops)).astype(bool).tolist()}


def walk(prog):
    """The program's effect on the count and the lifecycle: yields (op, count_before, k, states), states
    being the lifecycle states the handle is in during and after the op (no engine, no oracle)."""
    k, count, staged = prog["k"], 0, 0
    for op in prog["ops"]:
        kind, before, states = op[0], count, []
        if kind == "sample":
            count, staged = count + op[1], staged + op[1]
        elif kind == "stage":
            count, staged = count + op[1], staged + op[1]
        elif kind in ("host", "device", "device_torch", "indexed"):
            if op[1]:
                staged = 0
                if kind == "indexed":
                    states.append("owed")
            count += op[1]
        elif kind == "indexed_abort":
            staged = 0
            states.append("owed")
        elif kind == "seek":
            staged, count = 0, count + op[1]
        elif kind in ("merge_state", "merge_packed"):
            staged, count = 0, count + op[1] + op[2]
        elif kind in ("merge_zero_state", "merge_zero_packed"):
            staged, count = 0, count + op[1]
        elif kind == "recreate":
            staged = count = 0
        elif kind == "final":
            if op[1] == "external":
                states += ["owed", "external"]
                count += op[2]
            elif op[1] != "none":
                states.append("taken" if op[1] == "take" and k * key_width_of(prog["family"]) <= (1 << 20) else "closed")
        elif kind not in ("synchronize", "set_stream"):
            staged = 0  # result, exports, distinct_info flush the staging buffer
        if not (kind == "final" and op[1] != "none"):
            states.append("staged" if staged else "holding" if count else "fresh")
        yield op, before, k, states


def key_width_of(family):
    if family.startswith("el-"):
        return key_width(family.split("-")[1])
    return 4 if family == "di-int" else 8


def show(prog):
    """The whole program, for an assertion message: a failing case is replayed by its id."""
    head = f"{prog['family']} seed={prog['seed']} k={prog['k']} reusable={prog['reusable']}"
    return head + "\n  " + "\n  ".join(f"{i:2d} {op}" for i, op in enumerate(prog["ops"]))
