"""What a handle remembers, on the GPU: the walks of tests/handle_walk.py executed step by step on ONE PieContext each.

After every run step every word of the result is compared with the exact definition for the handle's current database, masks, keys,
queries and settings (handle_walk.Reference: schedule_layer_exact and level_oracles of tests/test_chain_schedule.py, mod_reduce_exact of
tests/test_result_limbs.py, o.pie_run for the default configuration) -- whatever came before must not matter.  After every refused
step the return code and the word piehip_last_error() must carry are checked, and the next run gives the bits it would have given
without the attempt.  Nothing is compared against another GPU run, except the fresh-handle run of `fused`, which is redundant with
the reference on purpose: if the walk fails it tells whether history or the configuration is at fault.  The three pieces of `small`
start from fresh handles in the states the long walk is in at their first steps: read which piece fails to bisect it.

A call that returns PIEHIP_EHIP ends the test at that step, and every later test of this file then fails without touching the device.

Measured on an MI355X, references included: this file 3.5 s of wall time (`fused` 2.2 s, `small` 0.6 s, `own_key` and the three pieces
0.15 s together), tests/test_gpu_chain_schedule.py 6.0 s in the same session.  DESIGN.md section 4f has the table of derived copies, the
steps that hold each and what three scratch builds with one refresh removed did to this file.
"""
import numpy as np
import pytest

from tests import handle_walk as hw

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A      # above every modulus: a word of a caller's buffer that run_into leaves unwritten shows
_hip_failed = []
_env = {}


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


@pytest.fixture
def codes(pie, monkeypatch):
    """every return code that reaches the Python mirror's check, in order (the mirror turns codes into exceptions and hands out no
    code: PIEHIP_ESTATE and PIEHIP_EHIP both arrive as RuntimeError, and this file must tell them apart)"""
    seen, orig = [], pie._check

    def check(rc):
        seen.append(rc)
        return orig(rc)
    monkeypatch.setattr(pie, "_check", check)
    return seen


def env(ob, pie, walk):
    """the oracle, the arrays and the expected results of a walk, computed once and shared by every test on it"""
    if walk.name not in _env:
        o = ob.Oracle(walk.N, walk.L, walk.t)

        def expand(seeds):
            cc = pie.PieContext(walk.N, walk.L, walk.t)
            try:
                return cc.expand_uniform(np.ascontiguousarray(seeds))
            finally:
                cc.close()
        data = hw.Data(o, expand=expand)
        ref = hw.Reference(ob, data)
        ref.prepare([c for _, c in hw.run_configs(walk)])
        _env[walk.name] = (o, data, ref)
    return _env[walk.name]


def by_query(nq, rows):
    """the library's [b][nq] rows (a handle without a batch: [b]) as [nq][b]"""
    return rows[None] if nq == 1 else rows.transpose(1, 0, 2, 3, 4)


class Runner:
    def __init__(self, pie, walk, data, codes):
        import torch
        self.torch, self.pie, self.walk, self.data, self.codes = torch, pie, walk, data, codes
        self.cc = pie.PieContext(walk.N, walk.L, walk.t)
        assert (self.cc.moduli == data.o.moduli).all()
        self.op, self.model = None, hw.Model(walk.L)
        self.alive, self.bufs = [], {}

    def close(self):
        if not _hip_failed:
            self.cc.close()

    def _device(self, a):
        t = self.torch.from_numpy(np.array(a).view(np.int64)).cuda()
        self.torch.cuda.synchronize()
        self.alive.append(t)        # kept: the next array of the same size lands at another address
        return t.data_ptr()

    def _results(self, rows):
        """rows as the library lays them out, in a caller's buffer or array"""
        return by_query(self.model.nq, rows).copy()

    def execute(self, step):
        """one step on the handle; a run step returns its results [nq][b][components][limbs][N]"""
        k, a, m, cc, op, data = step.kind, step.args, self.model, self.cc, self.op, self.data
        if k == "db":
            db, masks = data.db(a[0])
            self.op = self.pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
        elif k == "key":
            cc.load_relin_key(data.key(a[0]))
        elif k == "key_seeded":
            cc.load_relin_key_seeded(*data.seeded_key(a[0]))
        elif k == "key_q":
            cc.load_relin_key(data.key(a[0]), query=a[1])
        elif k == "batch":
            op.setQueryBatch(a[0])
        elif k in ("query", "query_dev"):
            q = a[1] if len(a) > 1 else 0
            idx, minus = data.query(m.db, a[0])
            if k == "query":
                op.setIndex(idx, query=q)
                op.setMinusCompareElement(minus, query=q)
            else:
                op.setIndexDevice(self._device(idx), query=q)
                op.setMinusCompareElementDevice(self._device(minus), query=q)
        elif k == "sched":
            who = op if op is not None else cc
            if len(a[0]) == 1:
                who.setChainLimbs(a[0][0])
            else:
                who.setChainSchedule(a[0])
        elif k == "keep":
            op.setResultLimbs(a[0])
        elif k == "relin":
            op.setResultRelin(a[0])
        elif k == "queues":
            cc.set_run_streams(a[0])
        elif k == "slots":
            cc.set_transform_slots(a[0])
        elif k == "graph":
            cc.set_graph(a[0])
        elif k == "profiling":
            cc.set_profiling(a[0])
        elif k == "run":
            if a == ("back_to_back",):
                op.run(sync=False)
            op.run()
            got = op.getResultList()            # [nq][b] for a batch already
            return (got[None] if m.nq == 1 else got).copy()
        elif k == "run_into":
            cfg = m.expected()          # rows [b][nq][components][limbs][N] ([b][..] without a batch), by the model
            shape = (m.b,) + ((m.nq,) if m.nq > 1 else ()) + (2 if cfg.relin else 3, cfg.limbs, self.walk.N)
            buf = self.bufs.get(a[0])
            if buf is None or tuple(buf.shape) != shape:
                buf = self.bufs[a[0]] = self.torch.empty(shape, dtype=self.torch.int64, device="cuda")
            buf.fill_(PATTERN)
            self.torch.cuda.synchronize()
            op.run(into=buf.data_ptr())
            return self._results(buf.cpu().numpy().view(np.uint64))
        elif k == "run_host":
            qs = [data.query(m.db, n) for n in a[0]]
            idx, minus = (qs[0] if m.nq == 1 else tuple(np.stack(v) for v in zip(*qs)))
            res = op.hostBuffers()[2]          # the page-locked array, asked for again: it follows the settings
            return self._results(op.runHost(idx, minus, results=res))
        elif k == "run_host_seeded":
            qs = [data.seeded_query(m.db, n) for n in a[0]]
            args = qs[0] if m.nq == 1 else tuple(np.stack(v) for v in zip(*qs))
            res = op.hostBuffers()[2]
            return self._results(op.runHostSeeded(*args, results=res))
        else:
            raise AssertionError(k)

    def guarded(self, step):
        try:
            return self.execute(step)
        finally:
            if hw.EHIP in self.codes:
                _hip_failed.append(step)

    def refused(self, step, where):
        from nested_hashing_psi_amd._lib import lib
        inner, code, word = step.args
        assert self.model.refusal(inner) == (code, word)
        n = len(self.codes)
        with pytest.raises((ValueError, RuntimeError, MemoryError)):
            self.guarded(inner)
        assert not _hip_failed, "%s: PIEHIP_EHIP: %s" % (where, lib().piehip_last_error())
        got = [c for c in self.codes[n:] if c]
        assert got == [code], "%s: return codes %s, expected %d" % (where, got, code)
        assert word.encode() in lib().piehip_last_error(), "%s: piehip_last_error() is %r, expected to name %r" % (where, lib().piehip_last_error(), word)


def mismatch(where, changes, got, want):
    if got.shape != want.shape:
        return "%s (last changes: %s): result shape %s, expected %s" % (where, changes, got.shape, want.shape)
    if (got == want).all():
        return None
    bad = np.argwhere((got != want).any(axis=(-1, -2)))
    return "%s (last changes: %s): %d of %d words differ; [query, bin layer, component] of the rows that differ: %s" % (
        where, changes, int((got != want).sum()), got.size, [tuple(int(v) for v in r) for r in bad[:24]])


def walk_steps(ob, pie, walk, codes, steps, label):
    """the steps on one fresh PieContext; returns the last run's results"""
    if _hip_failed:
        pytest.fail("an earlier test of this file met PIEHIP_EHIP at %r: nothing more is started on the device" % (_hip_failed[0],))
    _, data, ref = env(ob, pie, walk)
    r = Runner(pie, walk, data, codes)
    last, changes = None, []
    try:
        for i, step in enumerate(steps):
            where = "%s step %d %s%r%s" % (label, i, step.kind, step.args if step.kind != "refused" else step.args[0][:2],
                                           " '%s'" % step.name if step.name else "")
            if step.kind == "refused":
                r.refused(step, where)
            elif step.kind in hw.RUN_KINDS:
                r.model.apply(step)
                want = ref(r.model.expected())
                last = r.guarded(step)
                msg = mismatch(where, changes[-4:], last, want)
                assert msg is None, msg
            else:
                r.guarded(step)
                r.model.apply(step)
            if step.kind not in hw.RUN_KINDS:
                changes.append("%d %s%s" % (i, step.kind, " '%s'" % step.name if step.name else ""))
            assert not _hip_failed
    finally:
        r.close()
    return last


@pytest.mark.parametrize("name", sorted(hw.WALKS))
def test_walk(ob, pie, codes, name):
    """every run of the walk against the definition, every refusal by its code and its message"""
    walk = hw.WALKS[name]
    last = walk_steps(ob, pie, walk, codes, walk.steps, name)
    if name != "fused":
        return
    # the final configuration on a fresh handle: the same bits
    final = hw.states(walk)[-1]
    fresh = walk_steps(ob, pie, walk, codes, final.setup() + [hw.R], "fused, fresh handle")
    assert (fresh == last).all()


@pytest.mark.parametrize("label,first,end", hw.pieces(hw.SMALL), ids=[p[0] for p in hw.pieces(hw.SMALL)])
def test_piece_of_small_alone(ob, pie, codes, label, first, end):
    """steps [first, end) of `small` on a fresh handle, behind the shortest set-up of the state they start in"""
    walk_steps(ob, pie, hw.SMALL, codes, hw.piece_steps(hw.SMALL, first, end), "small[%d:%d]" % (first, end))
