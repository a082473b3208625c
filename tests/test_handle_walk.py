"""The walks of tests/handle_walk.py on the CPU: every walk against what it declares, and the model against the exact definitions.

The GPU test (tests/test_gpu_handle_walk.py) compares results; whether a walk still holds the orders it was written for is decided
here.  A pair "derived copy <- later change of its source" whose change step, the run in front of it or the run behind it has been
edited away fails in this file instead of passing vacuously on the device.
"""
import pytest

from tests import handle_walk as hw
from tests.param_chains import T16
from tests.test_chain_schedule import level_oracles, run_chain_schedule_exact
from tests.test_result_limbs import mod_reduce_exact

WALKS = sorted(hw.WALKS)


def check_pair(walk, pair, steps=None):
    """the pair's step is there, a run used the derived copy in front of it, the step is a real change, a run follows it"""
    steps = walk.steps if steps is None else steps
    hits = [i for i, s in enumerate(steps) if s.name == pair.name]
    assert len(hits) == 1, "pair %s: its step occurs %d times" % (pair.name, len(hits))
    i = hits[0]
    st = hw.states(walk, steps)
    step = steps[i]
    assert step.kind == pair.kind, "pair %s: the step is a %s" % (pair.name, step.kind)
    if pair.before is not None:
        runs = [j for j in range(i) if steps[j].kind in hw.RUN_KINDS]
        assert runs, "pair %s: no run in front of the change" % pair.name
        j = runs[-1]
        used_at = st[j + 1] if steps[j].kind in ("run_host", "run_host_seeded") else st[j]
        assert pair.before(used_at), "pair %s: the run in front of the change (step %d) does not use the derived copy" % (pair.name, j)
        for k in range(j + 1, i + 1):
            assert pair.before(st[k]), "pair %s: the derived copy is gone at step %d, in front of the change" % (pair.name, k)
    if pair.change is not None:
        assert pair.change(st[i], step), "pair %s: the step changes nothing of the source" % pair.name
    if pair.replays:
        # the run that captured the graph and `replays` replays of it, directly in front of the step
        front = steps[max(i - pair.replays - 1, 0):i]
        assert len(front) == pair.replays + 1 and all(s.kind in ("run", "run_into") and s[:2] == front[0][:2] for s in front), \
            "pair %s: fewer than %d replays of one graph in front of the change" % (pair.name, pair.replays)
        assert all(hw.on_graph(st[k]) for k in range(i - pair.replays - 1, i + 1))
    after = [k for k in range(i if step.kind in hw.RUN_KINDS else i + 1, len(steps)) if steps[k].kind in hw.RUN_KINDS]
    assert after, "pair %s: no run behind the change" % pair.name
    k = after[0]
    # nothing but the queries and per-query keys that run needs, a refused call, or a change the pair is written to be chained with
    for s in steps[i + 1:k]:
        assert s.kind in ("query", "query_dev", "key_q", "refused") or s.name in hw.CHAINED, \
            "pair %s: a %s step lies between the change and the run behind it" % (pair.name, s.kind)
    if pair.after is not None:
        at = st[k + 1] if steps[k].kind in ("run_host", "run_host_seeded") else st[k]
        assert pair.after(at), "pair %s: the run behind the change (step %d) is not in the state the pair is about" % (pair.name, k)


def check_walk(walk, steps=None):
    """everything a walk declares; steps: an edited copy of the walk's steps"""
    steps = walk.steps if steps is None else steps
    st = hw.states(walk, steps)          # (the model accepts every step outside `refused`)
    for i, s in enumerate(steps):
        if s.kind == "refused":
            inner, code, word = s.args
            assert st[i].refusal(inner) == (code, word), "step %d: the model answers %r" % (i, st[i].refusal(inner))
            # directly in front of a run: at most the queries and per-query keys that run needs lie between
            rest = [t for t in steps[i + 1:] if t.kind not in ("query", "query_dev", "key_q")]
            assert rest and rest[0].kind in hw.RUN_KINDS, "step %d: no run directly behind the refused call" % i
        elif s.kind in ("run", "run_into"):
            assert st[i].refusal(s) is None, "step %d: the model refuses this run: %r" % (i, st[i].refusal(s))
    for name in walk.refusals:
        hits = [s for s in steps if s.name == name]
        assert len(hits) == 1 and hits[0].kind == "refused", "refused step %s occurs %d times" % (name, len(hits))
    assert set(s.name for s in steps if s.kind == "refused") == set(walk.refusals), "a refused step the walk does not declare"
    for pair in walk.pairs:
        check_pair(walk, pair, steps)
    runs = hw.run_configs(walk, steps)
    distinct = len(set(c for _, c in runs))
    assert distinct >= walk.distinct, "%d distinct expected results, the walk states %d" % (distinct, walk.distinct)
    for (i, a), (j, b) in zip(runs, runs[1:]):
        between = [s.kind for s in steps[i + 1:j] if s.kind not in hw.NEUTRAL]
        assert not between or a != b, "runs %d and %d expect the same result across %s" % (i, j, between)


@pytest.mark.parametrize("name", WALKS)
def test_walk_holds_what_it_declares(name):
    check_walk(hw.WALKS[name])


def test_every_kind_of_step_occurs():
    small = hw.SMALL.steps
    assert set(s.kind for s in small) == set(hw.KINDS)
    refused = set(s.args[0].kind for s in small if s.kind == "refused")
    assert refused >= {"run", "graph", "sched", "keep", "relin", "key_q"}
    assert {len(s.args[0]) for s in small if s.kind == "sched"} == {1, 2}      # setChainLimbs and setChainSchedule
    assert all(s.kind in hw.KINDS for w in hw.WALKS.values() for s in w.steps)


def test_queue_counts_alternate_at_both_layer_counts():
    """queues 1 -> 2 -> 1 -> 2 with b = 3 and with b = 5, each followed by two runs back to back"""
    steps, st = hw.SMALL.steps, hw.states(hw.SMALL)
    seen = {}
    for i, s in enumerate(steps):
        if s.kind == "queues" and i + 1 < len(steps) and steps[i + 1] == hw.B2B and st[i].nq == 1:
            seen.setdefault(st[i].b, []).append(s.args[0])
    for b in (3, 5):
        assert any(seen.get(b, [])[k:k + 4] == [1, 2, 1, 2] for k in range(len(seen.get(b, [])))), (b, seen)


def test_pieces_cover_the_walk_and_start_in_its_states():
    walk = hw.SMALL
    ps = hw.pieces(walk)
    assert ps[0][1:] == (0, 12) and [p[2] for p in ps[:-1]] == [p[1] for p in ps[1:]] and ps[-1][2] == len(walk.steps)
    st = hw.states(walk)
    for _, first, end in ps:
        steps = hw.piece_steps(walk, first, end)
        n = len(steps) - (end - first)
        got = hw.states(walk, steps)
        for k in ("db", "key", "nq", "keyq", "slot", "sched", "keep", "relin", "queues", "slots", "graph", "profiling"):
            assert getattr(got[n], k) == getattr(st[first], k), (first, k)
        # the same expected results, run for run
        assert [c for _, c in hw.run_configs(walk, steps)] == [c for i, c in hw.run_configs(walk) if first <= i < end]


@pytest.mark.parametrize("name,step,caught", [
    ("small", "level_key", "its step occurs 0 times"),                          # the change itself
    ("small", "run_after_batch_grew", "refused step run_after_batch_grew occurs 0 times"),
    ("small", "graph_key_q", "pair graph_key_q: its step occurs 0 times"),
    ("small", -1, "pair sched_first: a db step lies between"),                  # the only run at K = 2, in front of masks_K2_to_K3
    ("fused", +1, "lies between the change and the run behind it"),             # the run behind evk_sigma_key
])
def test_a_deleted_step_is_noticed(name, step, caught):
    """one step deleted each: the change of a pair, a declared refused step, the graph's key_q change, the run in front of a change,
    the run behind one; `caught` is the assertion that notices"""
    walk = hw.WALKS[name]
    steps = list(walk.steps)
    if isinstance(step, str):
        del steps[walk.index(step)]
    elif step < 0:
        i = walk.index("masks_K2_to_K3")
        del steps[max(j for j in range(i) if steps[j].kind in hw.RUN_KINDS)]
    else:
        i = walk.index("evk_sigma_key")
        del steps[min(j for j in range(i, len(steps)) if steps[j].kind in hw.RUN_KINDS)]
    with pytest.raises(AssertionError, match=caught):
        check_walk(walk, steps)


# ---- the model against the exact definitions, N = 64 -----------------------------------------------------------------------------------
N64, L64 = 64, 3
DBS64 = {"one": (1, 2, 2), "three": (3, 2, 2)}


@pytest.fixture(scope="module")
def small_ring(ob):
    o = ob.Oracle(N64, L64, T16)
    data = hw.Data(o, DBS64)
    return o, data, hw.Reference(ob, data)


def _model(db, sched, relin, keep):
    m = hw.Model(L64, DBS64)
    for s in (hw.S("key", "k0"), hw.S("db", db), hw.S("query", "q0"), hw.S("sched", sched), hw.S("relin", relin), hw.S("keep", keep)):
        m.apply(s)
    return m


def test_one_hash_function_ignores_schedule_and_relin(ob, small_ring):
    """include/piehip.h: K = 1 has no product; both settings are accepted and change nothing, and rows have `keep` limbs"""
    o, data, ref = small_ring
    db, masks = data.db("one")
    idx, minus = data.query("one", "q0")
    plain = run_chain_schedule_exact(ob, o, idx, minus, db, masks, None, [L64])       # stage A and the mask multiply
    assert plain.shape == (2, 2, L64, N64)
    for sched in ((3,), (2,), (3, 1)):
        for relin in (True, False):
            for keep in (3, 2, 1):
                cfg = _model("one", sched, relin, keep).expected()
                assert cfg == hw.Config("one", ("q0",), (None,), (), True, keep)
                want = plain if keep == L64 else mod_reduce_exact(o, plain, keep)
                assert (ref(cfg)[0] == want).all(), (sched, relin, keep)


def test_rows_have_the_smaller_of_keep_and_the_last_level(ob, small_ring):
    """against the composition tests/test_chain_schedule.py and tests/test_result_relin.py pin: the schedule's rows, then the result
    reduction inside the last level where keep is below it"""
    o, data, ref = small_ring
    db, masks = data.db("three")
    idx, minus = data.query("three", "q0")
    evk = data.key("k0")
    for sched in ((3,), (3, 2), (2, 2), (3, 1)):
        levels = level_oracles(ob, o, sched)
        last = sched[-1]
        for relin in (True, False):
            rows = run_chain_schedule_exact(ob, o, idx, minus, db, masks, evk, list(sched), relin_last=relin)
            assert rows.shape == (2, 2 if relin else 3, last, N64)
            for keep in (3, 2, 1):
                cfg = _model("three", sched, relin, keep).expected()
                assert cfg.limbs == min(keep, last) and cfg.levels == (sched[0], last) and cfg.keys == ("k0",)
                want = rows if keep >= last else mod_reduce_exact(levels[last], rows, keep)
                got = ref(cfg)
                assert got.shape == (1, 2, 2 if relin else 3, min(keep, last), N64)
                assert (got[0] == want).all(), (sched, relin, keep)


def test_the_documented_forgetting(ob):
    """a batch change forgets per-query keys and the queries it drops; a database load forgets every index matrix; unloaded key
    slots take the handle's key; K = 2 without the last relinearisation reads no key"""
    m = hw.Model(3)
    for s in (hw.S("key", "k0"), hw.S("db", "A"), hw.S("batch", 3), hw.S("query", "q0"), hw.S("query", "q1", 1), hw.S("query", "q2", 2),
              hw.S("key_q", "k1", 1)):
        m.apply(s)
    assert m.expected().keys == ("k0", "k1", "k0")
    m.apply(hw.S("key", "k2"))
    assert m.expected().keys == ("k2", "k1", "k2")
    m.apply(hw.S("batch", 2))
    assert m.expected() == hw.Config("A", ("q0", "q1"), ("k2", "k2"), (3, 3), True, 3)
    m.apply(hw.S("batch", 3))
    assert m.refusal(hw.S("run")) == (hw.ESTATE, "query of the batch")
    assert m.refusal(hw.S("key_q", "k1", 3)) == (hw.EINVAL, "batch")
    m.apply(hw.S("db", "B"))
    assert m.refusal(hw.S("run")) == (hw.ESTATE, "setIndex")
    for q in range(3):
        m.apply(hw.S("query", "q0", q))
    m.apply(hw.S("relin", False))
    assert m.expected().keys == (None, None, None) and not m.expected().relin
    assert m.refusal(hw.S("graph", True)) == (hw.ESTATE, "result_relin")
