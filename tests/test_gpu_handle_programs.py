"""Seeded operation programs on one rsv_sampler handle against the model of tests/handle_model.py.

Every other test of the handle is a sequence its author scripted; the bugs this layer has had were
interactions nobody had scripted (a zero-part merge or a seek crossing k that kept a stale
publication, a throwing `map` that left keys owed).  Here numpy.random.default_rng(seed) draws 12-20
operations from the family's alphabet (handle_model.gen_program: per-element, staged, host, device and
index-only batches, aborted batches, seeks, results, exports, merges of a sibling's later range,
zero-part merges, stream hand-overs, close + a new handle on the recycled slot block), at the k where
the runtime changes path (2048/2049: the fused K1 + resolve; 8192/8193: the fused publication and the
coherent offsets block; 140 000: result() through the pinned copy).  After every operation count and
is_open are the model's; on a reusable handle result() is compared after half of them; a single-use
handle ends in its result, after which every sampling, result, export and merge call must raise
IllegalStateException.  A failing case prints its whole program and is replayed by its id."""
import collections.abc
import ctypes as C

import numpy as np
import pytest

import handle_model as HM

pytestmark = pytest.mark.gpu

SID = 7


class Boom(Exception):
    pass


class Throwing(collections.abc.Sequence):
    """An IndexedSeq whose every element throws: the `map` that fails on the first winner."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        raise Boom(i)


class Run:
    def __init__(self, prog, cuda, oracle):
        import torch

        from reservoir_amd import _native as N

        self.torch, self.N, self.L = torch, N, N.load()
        self.prog, self.cuda, self.O = prog, cuda, oracle
        fam = prog["family"].split("-")
        self.elements = fam[0] == "el"
        self.k, self.seed = prog["k"], 100 + prog["seed"]
        if self.elements:
            self.kt, self.engine = fam[1], fam[2]
        else:
            self.hash_name = fam[1]
            self.kt = "int" if fam[1] == "int" else "long"
        self.side = torch.cuda.Stream(device=cuda)
        self.s = self.m = None
        self.siblings = []
        self.new_handle(prog["reusable"])

    # -- handles ---------------------------------------------------------------------------------
    def make(self, reusable):
        from reservoir_amd import Sampler

        if self.elements:
            return Sampler(self.k, reusable=reusable, key_type=self.kt, engine=self.engine, seed=self.seed,
                           stream_id=SID)()
        if self.hash_name == "identity":
            return Sampler.distinct(self.k, reusable=reusable, seed=self.seed)(hash="identity")
        if self.hash_name == "collide":
            return Sampler.distinct(self.k, reusable=reusable, seed=self.seed, retain_log=True)()
        return Sampler.distinct(self.k, reusable=reusable, seed=self.seed, key_type="int")()

    def model(self):
        if self.elements:
            return HM.ElementsModel(self.O, self.engine, self.k, self.seed, SID, self.kt)
        return HM.DistinctModel(self.O, self.hash_name, self.k, self.seed)

    def new_handle(self, reusable):
        if self.s is not None:
            self.s.close()
        self.s, self.m = self.make(reusable), self.model()

    def keys(self, lo, n):
        if self.elements:
            return np.ascontiguousarray(HM.keys_range(self.kt, lo, n))
        return np.ascontiguousarray(HM.distinct_keys(self.hash_name, self.k, lo, n))

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.cuda)

    def ptr(self, a):
        return a.ctypes.data_as(C.c_void_p)

    # -- comparisons -------------------------------------------------------------------------------
    def same(self, got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        if not self.elements:
            got = np.sort(got)
        assert got.shape == want.shape and np.array_equal(got, want), what

    def check_result(self):
        self.same(self.s.result(), self.m.result(), "result()")

    # -- the operations ----------------------------------------------------------------------------
    def op_sample(self, m):
        ks = self.keys(self.m.count, m)
        for x in (ks.tolist() if ks.ndim == 1 else [r.tobytes() for r in ks]):
            self.s.sample(x)
        self.m.append(m)

    def op_stage(self, n):
        ks = self.keys(self.m.count, n)
        p, cap = C.c_void_p(), C.c_int64()
        self.N.check(self.L.rsv_stage_acquire(self.s.handle, C.byref(p), None, C.byref(cap)))
        assert cap.value >= n
        if n:
            C.memmove(p.value, ks.ctypes.data, ks.nbytes)
        self.N.check(self.L.rsv_stage_commit(self.s.handle, n))
        self.m.append(n)

    def op_host(self, n):
        ks = self.keys(self.m.count, n)
        self.N.check(self.L.rsv_sample_batch(self.s.handle, self.ptr(ks), n, self.N.MEM_HOST, None))
        self.m.append(n)

    def op_device(self, n):
        self.s.sample_all(self.dev(self.keys(self.m.count, n)))
        self.m.append(n)

    def op_device_torch(self, n):
        torch = self.torch
        self.s.set_stream(self.side.cuda_stream)
        with torch.cuda.stream(self.side):
            self.s.sample_all(self.dev(self.keys(self.m.count, n)))
        self.s.set_stream(torch.cuda.current_stream(self.cuda).cuda_stream)  # and back: a hand-over
        self.m.append(n)

    def op_set_stream(self):
        self.s.set_stream(self.torch.cuda.current_stream(self.cuda).cuda_stream)

    def abi_indexed(self, n):
        offs = np.empty(self.k, dtype=np.int64)
        self.N.check(self.L.rsv_sample_indexed(self.s.handle, n, self.ptr(offs)))
        if self.elements and self.engine == "philox_r":
            assert np.array_equal(offs, self.m.offsets(n) if n else np.full(self.k, -1)), "rsv_sample_indexed offsets"
        return offs

    def op_indexed(self, n):
        if self.kt in ("long", "int"):
            ks = self.keys(self.m.count, n)
            self.s.sample_all(ks if n % 2 else ks.tolist())  # a host array, a list: both IndexedSeq
        else:
            offs = self.abi_indexed(n)
            if n:
                assert self.s.count == self.m.count + n and self.s.is_open
                owed = HM.keys_at(self.kt, self.m.count + np.maximum(offs, 0))
                owed[offs < 0] = 0xEE  # not read
                self.N.check(self.L.rsv_fill_slots(self.s.handle, self.ptr(np.ascontiguousarray(owed))))
        self.m.append(n)

    def op_indexed_abort(self, n):
        if self.kt in ("long", "int"):
            winners = (self.m.offsets(n) >= 0).any() if self.engine == "philox_r" else None
            try:
                self.s.sample_all(Throwing(n))
            except Boom:
                threw = True
            else:
                threw = False  # no slot changed: `map` was not called, the batch counts
                self.m.append(n)
            assert winners is None or threw == winners, "map runs iff a slot changed"
        else:
            self.abi_indexed(n)
            self.N.check(self.L.rsv_abort_indexed(self.s.handle))

    def op_seek(self, delta):
        t = self.m.count + delta
        self.s.seek(t)
        self.m.seek(t)

    def op_result(self):
        self.check_result()

    def op_result_device(self):
        torch = self.torch
        shape = (self.k, HM.key_width(self.kt)) if self.kt.startswith("bytes") else (self.k,)
        dt = torch.uint8 if len(shape) == 2 else torch.int64 if self.kt == "long" else torch.int32
        out = torch.zeros(shape, dtype=dt, device=self.cuda)
        n = self.s.result_device(out)
        self.same(out[:n].cpu().numpy(), self.m.result(), "result_device")

    def op_export_state(self):
        idx, keys, hashes, n = self.s.export_state(self.cuda)
        if self.elements:
            held = self.m.writers >= 0
            assert n == self.k and np.array_equal(idx.cpu().numpy(), self.m.writers), "export_state idx"
            assert np.array_equal(keys.cpu().numpy()[held], self.m.keys()[held]), "export_state keys"
        else:
            self.same(keys.cpu().numpy()[:n], self.m.result(), "export_state keys")
        return idx, keys, hashes, n

    def op_export_packed(self, s=None, m=None, count=None):
        s, m = s or self.s, m or self.m
        row = self.torch.zeros(s.packed_width, dtype=self.torch.int64, device=self.cuda)
        s.export_packed(row)
        r, k = row.cpu().numpy(), self.k
        if self.elements:
            held = m.writers >= 0
            assert np.array_equal(r[:k], m.writers), "export_packed idx"
            if self.kt.startswith("bytes"):
                got = r[k:].view(np.uint8).reshape(k, -1)
            else:
                got = r[k:2 * k]
            assert np.array_equal(got[held], m.keys()[held].astype(np.int64) if got.ndim == 1 else m.keys()[held]), \
                "export_packed keys"
        else:
            n = int(r[2 * k])
            assert int(r[2 * k + 1]) == (m.count if count is None else count), "export_packed count"
            self.same(r[:n].astype(np.int32 if self.kt == "int" else np.int64), m.result(), "export_packed keys")
        return row

    def sibling(self, gap, n):
        """A second handle of the same stream over the later range [count + gap, count + gap + n)."""
        lo = self.m.count + gap
        sib, sm = self.make(False), self.model()
        self.siblings.append(sib)
        if self.elements:
            sib.seek(lo)
        sm.seek(lo)
        sib.sample_all(self.dev(self.keys(lo, n)))
        sm.append(n)
        return sib, sm, lo + n

    def merge_model(self, sm, total):
        self.m.merge(sm.writers if self.elements else sm.result(), total)

    def op_merge_state(self, gap, n):
        sib, sm, total = self.sibling(gap, n)
        idx, keys, hashes, cnt = sib.export_state(self.cuda)
        self.s.merge_state(idx[None], keys[None], hashes[None], [cnt], total)
        self.merge_model(sm, total)

    def op_merge_packed(self, gap, n):
        sib, sm, total = self.sibling(gap, n)
        row = self.op_export_packed(sib, sm, n)  # (a distinct handle has no seek: its count is its own n)
        self.s.merge_packed(row[None].contiguous(), total)
        self.merge_model(sm, total)

    def op_merge_zero_state(self, delta):
        torch, k, total = self.torch, self.k, self.m.count + delta
        kshape = (0, k, HM.key_width(self.kt)) if self.kt.startswith("bytes") else (0, k)
        z = torch.zeros((0, k), dtype=torch.int64, device=self.cuda)
        self.s.merge_state(z, torch.zeros(kshape, dtype=torch.uint8, device=self.cuda), z, [], total)
        self.m.merge(np.full(k, -1), total)

    def op_merge_zero_packed(self, delta):
        total = self.m.count + delta
        rows = self.torch.zeros((0, self.s.packed_width), dtype=self.torch.int64, device=self.cuda)
        self.s.merge_packed(rows, total)
        self.m.merge(np.full(self.k, -1), total)

    def op_synchronize(self):
        self.s.synchronize()

    def op_distinct_info(self):
        assert self.s.distinct_info()["size"] == self.m.result().size, "distinct_info size"

    def op_recreate(self):
        self.new_handle(self.prog["reusable"])

    # -- how a program ends --------------------------------------------------------------------------
    def rejected(self):
        """Every sampling, result, export and merge call: all must raise IllegalStateException."""
        from reservoir_amd import IllegalStateException as ISE

        N, L, h = self.N, self.L, self.s.handle
        one = self.keys(0, 1)
        dev1 = self.dev(one)
        count = self.s.count
        calls = [lambda: self.s.sample(one.tolist()[0] if one.ndim == 1 else one[0].tobytes()),
                 lambda: self.s.sample_all(dev1), lambda: self.s.result(), lambda: self.op_result_device(),
                 lambda: self.s.export_state(self.cuda), lambda: self.op_export_packed(),
                 lambda: self.op_merge_zero_packed(count), lambda: self.op_merge_zero_state(count),
                 lambda: N.check(L.rsv_sample_batch(h, self.ptr(one), 1, N.MEM_HOST, None)),
                 lambda: self.op_stage(0), lambda: N.check(L.rsv_stage_commit(h, 0))]
        if self.elements:
            calls += [lambda: self.abi_indexed(1), lambda: self.s.seek(count + 1)]
            if self.kt != "bytes24":
                calls.append(lambda: self.s.sample_all([1, 2, 3]))
        else:
            calls.append(lambda: self.s.distinct_info())
        for i, call in enumerate(calls):
            with pytest.raises(ISE):
                call()
            assert self.s.count == count, i

    def op_final(self, how, n=0):
        N, L = self.N, self.L
        if how == "none":
            self.check_result()
            return
        if how == "external":
            self.abi_indexed(n)
            N.check(L.rsv_commit_indexed(self.s.handle))
            self.m.append(n)
            assert self.s.count == self.m.count and self.s.is_open
            self.rejected_external()
            return
        want = self.m.result()
        if how == "take":
            got = self.s.result()  # rsv_result_take where the result is published, else rsv_result
        else:
            out = np.empty(self.k, dtype=self.s.key_dtype)
            cnt = C.c_int64()
            N.check(L.rsv_result(self.s.handle, self.ptr(out), self.k, C.byref(cnt)))
            got = out[: cnt.value]
            if self.kt.startswith("bytes"):
                got = got.view(np.uint8).reshape(cnt.value, HM.key_width(self.kt))
        self.same(got, want, "the final result()")
        assert not self.s.is_open and self.s.count == self.m.count
        self.rejected()
        self.s.synchronize()  # plumbing stays valid on a closed handle
        assert not self.s.is_open and self.s.count == self.m.count

    def rejected_external(self):
        """After rsv_commit_indexed the slots hold no keys: keyed calls are rejected, index-only
        batches go on."""
        from reservoir_amd import IllegalStateException as ISE

        N, L, h = self.N, self.L, self.s.handle
        one = self.keys(0, 1)
        count = self.s.count
        for call in (lambda: self.s.result(), lambda: self.s.export_state(self.cuda), lambda: self.op_export_packed(),
                     lambda: N.check(L.rsv_sample_batch(h, self.ptr(one), 1, N.MEM_HOST, None)),
                     lambda: self.op_stage(0), lambda: self.op_merge_zero_packed(count)):
            with pytest.raises(ISE):
                call()
            assert self.s.count == count and self.s.is_open
        self.abi_indexed(5)
        assert self.s.count == count + 5
        N.check(L.rsv_abort_indexed(h))
        assert self.s.count == count and self.s.is_open

    def run(self):
        prog = self.prog
        for i, (op, chk) in enumerate(zip(prog["ops"], prog["checks"])):
            try:
                getattr(self, "op_" + op[0])(*op[1:])
                if op[0] != "final":
                    assert self.s.count == self.m.count, "count"
                    assert self.s.is_open, "is_open"
                    if prog["reusable"] and chk:
                        self.check_result()
            except Exception as e:
                raise AssertionError(f"op {i} {op}: {type(e).__name__}: {e}\n{HM.show(prog)}") from e
        self.s.close()
        for sib in self.siblings:
            sib.close()


@pytest.mark.parametrize("family,seed", HM.program_ids(), ids=lambda v: str(v))
def test_program(cuda, oracle, family, seed):
    Run(HM.gen_program(family, seed), cuda, oracle).run()


def test_seek_alone_then_result_is_empty_slots(cuda):
    """What the programs found: a count that came from rsv_seek alone, on a handle that took over the
    slot block of a closed sampler, used to publish that sampler's keys; the result is zeros."""
    import torch

    from reservoir_amd import Sampler

    for k in (7, 2049, 8193):
        old = Sampler(k, seed=1)()
        old.sample_all(torch.arange(1, 3 * k, dtype=torch.int64, device=cuda))
        assert old.result().all()
        old.close()  # its block goes back clean
        s = Sampler(k, seed=1, reusable=True)()
        s.seek(k // 2 + 1)
        assert not s.result().any() and s.result().size == k // 2 + 1
        s.seek(10 * k)
        out = torch.ones(k, dtype=torch.int64, device=cuda)
        assert s.result_device(out) == k and not out.cpu().numpy().any()
        s.close()
