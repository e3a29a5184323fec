"""The (lifecycle state x entry point) matrix of one rsv_sampler handle, laid beside include/reservoir_hip.h.

For each lifecycle state a family has (tests/handle_model.py STATES) a small handle (k = 16, n <= 100) is
put into it through the C ABI, and every entry point is issued once -- on a handle of its own -- with
otherwise valid arguments.  Pinned: the returned rsv_status; that a rejected call leaves rsv_count and
rsv_is_open as they were; and that the handle then completes its normal continuation (more keys and
result(), the owed keys, the next index-only or candidate batch) with the model's result -- for the
hash-only handles, which have no result, with what an undisturbed twin handle reports.  The plumbing
calls (streams, synchronize, profiling, count, is_open) are taken in every state but a pending candidate
batch, and are checked to change nothing either.

The table is the header's: a closed single-use handle, a handle that owes keys after
rsv_sample_indexed, one whose slots hold no keys (rsv_commit_indexed / rsv_distinct_candidates) and one
with a pending candidate batch reject every sampling, staging, result, seek, export, merge and log call
with RSV_E_ILLEGAL_STATE -- checkOpen before any other work, Sampler.scala:185-186 -- rsv_sample,
rsv_stage_acquire and rsv_stage_commit included while keys are owed (they used to stage the key).
    .  RSV_OK     S  RSV_E_ILLEGAL_STATE     U  RSV_E_UNSUPPORTED (the handle's kind has no such call)"""
import ctypes as C

import numpy as np
import pytest

import handle_model as HM

pytestmark = pytest.mark.gpu

K, SEED, SID = 16, 11, 5

CALLS = ("sample stage_acquire stage_commit batch_host batch_device "
         "sample_indexed fill_slots abort_indexed commit_indexed "
         "distinct_candidates candidates_read candidates_commit candidates_abort "
         "result result_device result_take "
         "seek export_state merge_state export_packed merge_packed "
         "get_distinct_info retain_log export_log merge_log "
         "set_stream set_resolve_stream synchronize profile_enable profile_read").split()
PLUMBING = CALLS[-5:]

#                            sample         indexed   candidates  result  seek/export    info/log  plumbing
#                            sa st st ho de in fi ab co ca re co ab rs dv tk sk ex mg ep mp in rt el ml ss sr sy pe pr
OPEN_EL = {"philox_r":      "..... .SSS USSS ... ..... UUUU .....",
           "java_l":        "..... .SSS USSS ... U.... UUUU ....."}
EXTERNAL_EL = {"philox_r":  "SSSSS .SSS USSS SSS .SSSS UUUU .....",
               "java_l":    "SSSSS .SSS USSS SSS USSSS UUUU ....."}
OWED_EL =                   "SSSSS S... SSSS SSS SSSSS SSSS ....."
CLOSED_EL =                 "SSSSS SSSS SSSS SSS SSSSS SSSS ....."
OPEN_DSET =                 "..... USSS USSS ... U.... ..UU .U..."
CLOSED_D =                  "SSSSS SSSS SSSS SSS SSSSS SSSS .U..."
TABLE = {}
for _e in ("philox_r", "java_l"):
    TABLE["el-" + _e] = {"fresh": OPEN_EL[_e], "holding": OPEN_EL[_e], "staged": OPEN_EL[_e], "owed": OWED_EL,
                         "external": EXTERNAL_EL[_e], "closed": CLOSED_EL, "taken": CLOSED_EL}
TABLE["di-set"] = {"fresh": OPEN_DSET, "holding": OPEN_DSET, "staged": OPEN_DSET, "closed": CLOSED_D,
                   "taken": CLOSED_D}
TABLE["di-hashonly"] = {"fresh":        "..... USSS .SSS ... U.... ..U. .U...",
                        "cand_idle":    "SSSSS USSS .SSS SSS USSSS SSSS .U...",
                        "cand_pending": "SSSSS SSSS S... SSS SSSSS SSSS SSSSS",
                        "closed": CLOSED_D}
CASES = [(f, st) for f, rows in TABLE.items() for st in rows]


def test_table_is_whole():
    assert set(TABLE["el-philox_r"]) == set(TABLE["el-java_l"]) == {"fresh", "holding", "staged", "owed", "external",
                                                                    "closed", "taken"}
    assert all(st in HM.STATES for rows in TABLE.values() for st in rows)
    for rows in TABLE.values():
        for row in rows.values():
            assert len(row.replace(" ", "")) == len(CALLS) and set(row) <= set(".SU ")


class Ctx:
    """One handle in one state, the buffers every call needs, and the state's continuation."""

    def __init__(self, family, state, cuda, oracle):
        import torch

        from reservoir_amd import _native as N

        self.N, self.L, self.torch, self.cuda, self.O = N, N.load(), torch, cuda, oracle
        self.family, self.state = family, state
        self.elements = family.startswith("el-")
        cfg = N.RsvConfig()
        N.check(self.L.rsv_config_init(C.byref(cfg)))
        cfg.max_sample_size, cfg.key_width, cfg.reusable, cfg.seed, cfg.stream_id = K, 8, 0, SEED, SID
        if self.elements:
            self.engine = family[3:]
            cfg.kind, cfg.engine = N.KIND_ELEMENTS, N.ENGINE_JAVA_L if self.engine == "java_l" else N.ENGINE_PHILOX_R
            self.m = HM.ElementsModel(oracle, self.engine, K, SEED, SID, "long")
        else:
            cfg.kind = N.KIND_DISTINCT
            cfg.hash_kind = N.HASH_IDENTITY if family == "di-set" else N.HASH_PRECOMPUTED
            self.m = HM.DistinctModel(oracle, "identity", K, SEED)  # (a precomputed hash(x) = x is the identity's)
        h = C.c_void_p()
        N.check(self.L.rsv_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.offs = np.full(K, -1, dtype=np.int64)
        self.out = np.zeros(K, dtype=np.int64)
        self.cnt = C.c_int64()
        self.dev = torch.zeros(3 * K + 8, dtype=torch.int64, device=cuda)  # device scratch: k keys, idx, hashes, a row
        self.dev_keys = torch.from_numpy(self.keys(1000, 5)).to(cuda)
        torch.cuda.synchronize()
        self.enter(state)

    def close(self):
        self.L.rsv_destroy(self.h)

    def keys(self, lo, n):
        if self.elements:
            return np.ascontiguousarray(HM.keys_range("long", lo, n))
        return np.ascontiguousarray(HM.distinct_keys("identity", K, lo, n))

    @staticmethod
    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    def batch(self, n):
        ks = self.keys(self.m.count, n)
        self.N.check(self.L.rsv_sample_batch(self.h, self.p(ks), n, self.N.MEM_HOST, self.p(ks)))
        self.m.append(n)

    def candidates(self, lo, n):
        hs = self.keys(lo, n)
        nc = C.c_int64()
        self.N.check(self.L.rsv_distinct_candidates(self.h, self.p(hs), n, self.N.MEM_HOST, C.byref(nc)))
        return nc.value

    def read_commit(self):
        nc = 100
        o, hh = np.full(nc, -7, dtype=np.int64), np.zeros(nc, dtype=np.int64)
        self.N.check(self.L.rsv_candidates_read(self.h, self.p(o), self.p(hh), nc))
        self.N.check(self.L.rsv_candidates_commit(self.h, 0, 0))
        return o.tolist() + hh.tolist()

    def enter(self, state):
        N, L, h = self.N, self.L, self.h
        if state in ("holding", "staged", "owed", "closed", "taken"):
            self.batch(40)
        if state == "staged":
            ks = self.keys(self.m.count, 5)
            for i in range(5):
                N.check(L.rsv_sample(h, self.p(ks[i:]), self.p(ks[i:])))
            self.m.append(5)
        if state == "owed":
            N.check(L.rsv_sample_indexed(h, 30, self.p(self.offs)))
        if state == "external":
            N.check(L.rsv_sample_indexed(h, 40, self.p(self.offs)))
            N.check(L.rsv_commit_indexed(h))
            self.m.append(40)
        if state == "closed":
            N.check(L.rsv_result(h, self.p(self.out), K, C.byref(self.cnt)))
        if state == "taken":
            buf = C.c_void_p()
            N.check(L.rsv_result_take(h, C.byref(buf), C.byref(self.cnt)))
            L.rsv_host_release(buf)
        if state in ("cand_idle", "cand_pending"):
            self.candidates(0, 20)
            self.read_commit()
        if state == "cand_pending":
            self.candidates(20, 20)

    def count(self):
        return int(self.L.rsv_count(self.h))

    def is_open(self):
        return int(self.L.rsv_is_open(self.h))

    # -- every entry point once, with otherwise valid arguments ----------------------------------------
    def call(self, name):
        N, L, h, p, d = self.N, self.L, self.h, self.p, self.dev
        ks = self.keys(500, 8)
        dp = lambda off: C.c_void_p(d.data_ptr() + 8 * off)  # noqa: E731
        vp, cap, n = C.c_void_p(), C.c_int64(), C.c_int64()
        if name == "result_take":
            st = L.rsv_result_take(h, C.byref(vp), C.byref(n))
            if st == N.OK:
                L.rsv_host_release(vp)
            return st
        info = N.RsvDistinctInfo()
        info.struct_size = C.sizeof(N.RsvDistinctInfo)
        dbl = C.c_double()
        f = {
            "sample": lambda: L.rsv_sample(h, p(ks), p(ks)),
            "stage_acquire": lambda: L.rsv_stage_acquire(h, C.byref(vp), C.byref(C.c_void_p()), C.byref(cap)),
            "stage_commit": lambda: L.rsv_stage_commit(h, 0),
            "batch_host": lambda: L.rsv_sample_batch(h, p(ks), 8, N.MEM_HOST, p(ks)),
            "batch_device": lambda: L.rsv_sample_batch(h, C.c_void_p(self.dev_keys.data_ptr()), 5, N.MEM_DEVICE,
                                                       C.c_void_p(self.dev_keys.data_ptr())),
            "sample_indexed": lambda: L.rsv_sample_indexed(h, 9, p(np.empty(K, dtype=np.int64))),
            "fill_slots": lambda: L.rsv_fill_slots(h, p(self.keys(self.m.count, K))),
            "abort_indexed": lambda: L.rsv_abort_indexed(h),
            "commit_indexed": lambda: L.rsv_commit_indexed(h),
            "distinct_candidates": lambda: L.rsv_distinct_candidates(h, p(ks), 8, N.MEM_HOST, C.byref(n)),
            "candidates_read": lambda: L.rsv_candidates_read(h, p(np.empty(100, dtype=np.int64)),
                                                             p(np.empty(100, dtype=np.int64)), 100),
            "candidates_commit": lambda: L.rsv_candidates_commit(h, 0, 0),
            "candidates_abort": lambda: L.rsv_candidates_abort(h),
            "result": lambda: L.rsv_result(h, p(np.empty(K, dtype=np.int64)), K, C.byref(n)),
            "result_device": lambda: L.rsv_result_device(h, dp(0), K, C.byref(n)),
            "seek": lambda: L.rsv_seek(h, self.count() + 3),
            "export_state": lambda: L.rsv_export_state(h, dp(0), dp(K), dp(2 * K), C.byref(n)),
            "merge_state": lambda: L.rsv_merge_state(h, dp(0), dp(K), dp(2 * K), p(np.zeros(1, dtype=np.int64)), 0, K,
                                                     self.count()),
            "export_packed": lambda: L.rsv_export_packed(h, dp(0)),
            "merge_packed": lambda: L.rsv_merge_packed(h, dp(0), 0, 2 * K + 6, self.count()),
            "get_distinct_info": lambda: L.rsv_get_distinct_info(h, C.byref(info)),
            "retain_log": lambda: L.rsv_retain_log(h, 1),
            "export_log": lambda: L.rsv_export_log(h, 2**63 - 1, None, None, 0, C.byref(n)),
            "merge_log": lambda: L.rsv_merge_log(h, None, None, 0, self.count()),
            "set_stream": lambda: L.rsv_set_stream(h, C.c_void_p(self.torch.cuda.current_stream(self.cuda).cuda_stream)),
            "set_resolve_stream": lambda: L.rsv_set_resolve_stream(h, None),
            "synchronize": lambda: L.rsv_synchronize(h),
            "profile_enable": lambda: L.rsv_profile_enable(h, 0),
            "profile_read": lambda: L.rsv_profile_read(h, C.byref(dbl), C.byref(n)),
        }[name]
        return f()

    # -- what the handle does next, as something to compare ------------------------------------------
    def finish(self):
        """Complete the state's normal continuation; returns (got, want) -- want from the model, or None
        where only a twin handle can say (the hash-only states)."""
        N, L, h = self.N, self.L, self.h
        st = self.state
        if st in ("closed", "taken"):
            got = (L.rsv_result(h, self.p(self.out), K, C.byref(self.cnt)), self.is_open(), self.count())
            return got, (N.E_ILLEGAL_STATE, 0, self.m.count)
        if st == "external":
            c0 = self.count()
            N.check(L.rsv_sample_indexed(h, 7, self.p(self.offs)))
            want_offs = self.m.offsets(7).tolist() if self.engine == "philox_r" else self.offs.tolist()
            N.check(L.rsv_commit_indexed(h))
            return (self.count(), self.is_open(), self.offs.tolist()), (c0 + 7, 1, want_offs)
        if st in ("cand_idle", "cand_pending"):
            if st == "cand_idle":
                self.candidates(20, 20)
            got = self.read_commit()
            return (self.count(), got), None
        if st == "owed":
            owed = HM.keys_at("long", self.m.count + np.maximum(self.offs, 0))
            assert self.engine != "philox_r" or np.array_equal(self.offs, self.m.offsets(30))
            N.check(L.rsv_fill_slots(h, self.p(np.ascontiguousarray(owed))))
            self.m.append(30)
        else:
            self.batch(30)
        N.check(L.rsv_result(h, self.p(self.out), K, C.byref(self.cnt)))
        got = self.out[: self.cnt.value].copy()
        if not self.elements:
            got = np.sort(got)
        return (self.count(), self.is_open(), got.tolist()), (self.m.count, 0, self.m.result().tolist())


@pytest.mark.parametrize("family,state", CASES, ids=lambda v: str(v))
def test_state_row(cuda, oracle, family, state):
    from reservoir_amd import _native as N

    code = {".": N.OK, "S": N.E_ILLEGAL_STATE, "U": N.E_UNSUPPORTED}
    row = TABLE[family][state].replace(" ", "")
    twin = Ctx(family, state, cuda, oracle)
    want_twin, want_model = twin.finish()
    twin.close()
    if want_model is not None:
        assert want_twin == want_model, "the undisturbed handle"
    bad = []
    for name, letter in zip(CALLS, row):
        c = Ctx(family, state, cuda, oracle)
        count, is_open = c.count(), c.is_open()
        st = c.call(name)
        if st != code[letter]:
            bad.append((name, "want " + letter, "got status %d" % st))
        elif st != N.OK or name in PLUMBING:
            # rejected (or plumbing): nothing moved, and the handle goes on as if never asked
            if (c.count(), c.is_open()) != (count, is_open):
                bad.append((name, "count/is_open moved", (count, is_open), (c.count(), c.is_open())))
            elif c.finish()[0] != want_twin:
                bad.append((name, "the continuation differs"))
        c.close()
    assert not bad, bad


@pytest.mark.parametrize("family,state", CASES, ids=lambda v: str(v))
def test_count_and_is_open_answer_in_every_state(cuda, oracle, family, state):
    """rsv_count, rsv_is_open and rsv_get_stream are taken everywhere; a closed handle keeps its count."""
    c = Ctx(family, state, cuda, oracle)
    want = {"owed": 70, "cand_idle": 20, "cand_pending": 20}.get(state, c.m.count)
    assert c.count() == want and c.is_open() == (0 if state in ("closed", "taken") else 1)
    assert c.L.rsv_get_stream(c.h)
    c.close()


@pytest.mark.parametrize("then", ["nothing", "export_state", "merge_state"])
def test_distinct_serves_a_publication_only_as_the_last_group(cuda, oracle, monkeypatch, then):
    """A distinct batch may publish its merged set speculatively (forced for every batch here through
    RSV_SPEC_MIN_BATCH, read at creation), and result() then only waits for that publication -- but only
    while no group of work came after it.  rsv_export_state opens a group that reads the set, and
    rsv_merge_state of a distinct sampler changes the set without a word about the publication: after
    either, result() publishes again, and gives the oracle's set of everything sampled and merged."""
    import torch

    from reservoir_amd import Sampler

    monkeypatch.setenv("RSV_SPEC_MIN_BATCH", "1")
    keys = oracle.splitmix_keys(77, 6000)
    kd = torch.from_numpy(keys).to(cuda)
    d = Sampler.distinct(K, seed=SEED, reusable=True)(hash="identity")
    ref = oracle.Distinct(K, SEED, oracle.HASH_IDENTITY)
    d.sample_all(kd[:4000])
    ref.sample_all(keys[:4000])
    if then == "export_state":
        _, got_keys, _, n = d.export_state(cuda)
        assert n == K and np.array_equal(np.sort(got_keys.cpu().numpy()), np.sort(ref.result()[0]))
    elif then == "merge_state":
        e = Sampler.distinct(K, seed=SEED)(hash="identity")
        e.sample_all(kd[4000:])
        _, pk, ph, pn = e.export_state(cuda)
        d.merge_state(torch.zeros((1, K), dtype=torch.int64, device=cuda), pk[None], ph[None], [pn], keys.size)
        ref.sample_all(keys[4000:])
        e.close()
    want = ref.result()[0]
    assert np.array_equal(d.result(), want)
    assert np.array_equal(d.result(), want)  # a reusable sampler: asked twice
    d.close()
