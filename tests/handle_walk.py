"""What a handle remembers, as data: three written-out walks over the public surface of one handle, the pairs "derived copy <- later
change of its source" each walk holds, and a small model of the state a handle must be in after any sequence of steps.

A step is a named tuple (kind, args, name).  The model restates the documented rules of include/piehip.h, not the library's code:
  - a batch change forgets per-query keys and the queries it drops;
  - a database load forgets every index matrix;
  - key slots no query loaded take the handle's key, and query q's own key (piehip_load_relin_key_q) is the one it relinearises with,
    in a batch of one as in any other;
  - with K = 1, chain limbs and the result relinearisation change nothing; with K = 2 and no last relinearisation no key is read;
  - result rows have min(keep, last level) limbs.
Given the steps so far it says which (database, queries, keys, product levels, relin, row limbs) the next run must compute with
(Model.expected) and which calls must be refused, with which code and which word in piehip_last_error() (Model.refusal).

tests/test_handle_walk.py holds the walks to what they declare here; tests/test_gpu_handle_walk.py executes them on one PieContext and
compares every run, word for word, with reference() below: the exact definitions of tests/test_chain_schedule.py and
tests/test_result_limbs.py, and o.pie_run for the default configuration.
"""
import collections
import zlib

import numpy as np

from tests.param_chains import T16, T32

EINVAL, ESTATE, EHIP = -1, -2, -3

Step = collections.namedtuple("Step", "kind args name")


def S(kind, *args, name=""):
    return Step(kind, args, name)


KINDS = ("db", "key", "key_seeded", "key_q", "batch", "query", "query_dev", "sched", "keep", "relin", "queues", "slots", "graph",
         "profiling", "run", "run_into", "run_host", "run_host_seeded", "refused")
RUN_KINDS = ("run", "run_into", "run_host", "run_host_seeded")
# steps that must change no bit of a result
NEUTRAL = ("queues", "slots", "graph", "profiling", "refused")

# database name -> (K, b, E).  A2 is A' of the same shape with other contents and masks; D has more bin layers than any other
DBS = {"A": (3, 3, 2), "A2": (3, 3, 2), "B": (2, 2, 3), "C": (1, 3, 2), "D": (3, 5, 2)}

# what a run computes with: per query of the batch its name and its key's (None where no key is read), the limb count of every
# product of the chain (empty at K = 1), whether the last product is relinearised, and the limbs of a result row
Config = collections.namedtuple("Config", "db queries keys levels relin limbs")


class Model:
    def __init__(self, L, dbs=DBS):
        self.L, self.dbs = L, dbs
        self.db = self.key = None
        self.nq = 1
        self.keyq = {}
        self.slot = [None] * 8
        self.sched, self.keep, self.relin = (L,), L, True
        self.queues = self.slots = 0
        self.graph = self.profiling = False

    def copy(self):
        m = Model(self.L, self.dbs)
        m.__dict__.update(self.__dict__)
        m.keyq, m.slot = dict(self.keyq), list(self.slot)
        return m

    @property
    def K(self):
        return self.dbs[self.db][0] if self.db else 0

    @property
    def b(self):
        return self.dbs[self.db][1] if self.db else 0

    def levels(self):
        """limbs of product hf = 1 .. K - 1"""
        return tuple(self.sched[min(hf, len(self.sched)) - 1] for hf in range(1, self.K))

    @property
    def last(self):
        """limbs of the last product that runs: the mask multiply's and the result rows' (L where there is no product)"""
        lv = self.levels()
        return lv[-1] if lv else self.L

    def below(self):
        """some product of the chain runs on a level context"""
        return self.K >= 2 and min(self.levels()) < self.L

    def key_read(self):
        return self.K >= 3 or (self.K == 2 and self.relin)

    def key_of(self, q):
        return self.keyq.get(q, self.key)

    def _run_refusal(self, with_queries):
        if not self.db:
            return ESTATE, "database"
        if self.key_read() and not (self.key or all(q in self.keyq for q in range(self.nq))):
            return ESTATE, "key"
        for q in range(self.nq if with_queries else 0):
            if self.slot[q] is None:
                return ESTATE, ("query of the batch" if q else "setIndex")
        return None

    def refusal(self, step):
        """(code, a word of the message) where the documented rules refuse the call, else None"""
        k, a, L = step.kind, step.args, self.L
        if k == "key_q":
            return (EINVAL, "batch") if a[1] >= self.nq else None
        if k == "batch":
            return None if 1 <= a[0] <= 8 else (EINVAL, "between 1 and 8")
        if k in ("query", "query_dev"):
            q = a[1] if len(a) > 1 else 0
            if k == "query" and not self.db:
                return ESTATE, "database"
            return (EINVAL, "batch") if q >= self.nq else None
        if k == "sched":
            s = a[0]
            if not 1 <= len(s) <= 7:
                return EINVAL, "entries"
            if any(not 1 <= v <= L for v in s):
                return EINVAL, "between 1 and L"
            if any(x < y for x, y in zip(s, s[1:])):
                return EINVAL, "increase"
            return (ESTATE, "graph") if min(s) < L and self.graph else None
        if k == "keep":
            if not 1 <= a[0] <= L:
                return EINVAL, "keep"
            return (ESTATE, "graph") if a[0] < L and self.graph else None
        if k == "relin":
            return (ESTATE, "graph") if not a[0] and self.graph else None
        if k == "graph" and a[0]:
            if self.keep < L:
                return ESTATE, "result_limbs"
            if not self.relin:
                return ESTATE, "result_relin"
            if min(self.sched) < L:
                return ESTATE, "chain_limbs"
            return None
        if k in ("run", "run_into"):
            return self._run_refusal(True)
        if k in ("run_host", "run_host_seeded"):
            return self._run_refusal(False)
        return None

    def apply(self, step):
        """the state after an accepted step (a refused one changes nothing)"""
        k, a = step.kind, step.args
        assert k in KINDS, k
        if k == "refused" or k in ("run", "run_into"):
            return
        assert self.refusal(step) is None, "the model refuses %r: %r" % (step, self.refusal(step))
        if k == "db":
            self.db = a[0]
            self.slot = [None] * 8          # every index matrix is gone
        elif k in ("key", "key_seeded"):
            self.key = a[0]
        elif k == "key_q":
            self.keyq[a[1]] = a[0]
        elif k == "batch":
            if a[0] != self.nq:
                self.keyq = {}
                self.slot[a[0]:] = [None] * (8 - a[0])
                self.nq = a[0]
        elif k in ("query", "query_dev"):
            self.slot[a[1] if len(a) > 1 else 0] = a[0]
        elif k in ("run_host", "run_host_seeded"):
            assert len(a[0]) == self.nq
            self.slot[:self.nq] = list(a[0])
        elif k == "sched":
            self.sched = tuple(a[0])
        elif k in ("keep", "relin", "queues", "slots", "graph", "profiling"):
            setattr(self, k, a[0])

    def expected(self):
        """the configuration the next run must compute with"""
        assert self._run_refusal(True) is None, self._run_refusal(True)
        K = self.K
        keys = tuple(self.key_of(q) if self.key_read() else None for q in range(self.nq))
        return Config(self.db, tuple(self.slot[:self.nq]), keys, self.levels(), self.relin or K < 2,
                      min(self.keep, self.last) if K >= 2 else self.keep)

    def setup(self):
        """the shortest steps that bring a fresh handle into this state (host-memory queries)"""
        out = []
        if self.sched != (self.L,):
            out.append(S("sched", self.sched))
        for kind in ("queues", "slots"):
            if getattr(self, kind):
                out.append(S(kind, getattr(self, kind)))
        if self.key:
            out.append(S("key_seeded" if self.key.startswith("s") else "key", self.key))
        if self.db:
            out.append(S("db", self.db))
            if self.nq != 1:
                out.append(S("batch", self.nq))
            out += [S("query", self.slot[q], q) for q in range(self.nq) if self.slot[q] is not None]
            out += [S("key_q", k, q) for q, k in sorted(self.keyq.items())]
            if self.keep != self.L:
                out.append(S("keep", self.keep))
            if not self.relin:
                out.append(S("relin", False))
        else:
            assert self.nq == 1 and not self.keyq and self.keep == self.L and self.relin
        if self.graph:
            out.append(S("graph", True))
        if self.profiling:
            out.append(S("profiling", True))
        return out


def states(walk, steps=None):
    """the model in front of every step, and behind the last one"""
    m, out = Model(walk.L), []
    for st in (walk.steps if steps is None else steps):
        out.append(m.copy())
        m.apply(st)
    out.append(m)
    return out


def run_configs(walk, steps=None):
    """[(index, Config)] of the run steps"""
    steps = walk.steps if steps is None else steps
    st = states(walk, steps)
    return [(i, (st[i + 1] if s.kind in ("run_host", "run_host_seeded") else st[i]).expected()) for i, s in enumerate(steps) if s.kind in RUN_KINDS]


# ---- the pairs ---------------------------------------------------------------------------------------------------------------------
# Pair: the step `name` of kind `kind` changes the source of a derived copy.  before(model) must hold from a run in front of the
# step up to it (the copy exists and a run used it); change(model in front, step) says the step is a real change; after(model) must
# hold at the first run behind it.  replays: that many replays of one captured graph directly in front of the step (behind the run
# that captured it).
Pair = collections.namedtuple("Pair", "name kind before change after replays")


# changes that follow another pair's change with no run between, on purpose (sched, then key, then db; graph off, then a schedule)
CHAINED = ("key_after_sched", "db_after_sched", "sched_after_graph")


def P(name, kind, before=None, change=None, after=None, replays=0):
    return Pair(name, kind, before, change, after if after is not None else before, replays)


def _level3(m):        # a chain with a product on a level context: the level has its copies of the keys and, the last one, of the masks
    return m.K >= 3 and m.last < m.L and m.key is not None


def on_graph(m):
    return m.graph and m.nq == 1 and not m.profiling


def _own_key(m):       # a handle without a batch whose query 0 has a key of its own
    return m.nq == 1 and 0 in m.keyq and m.key_read()


_other_key = lambda m, s: s.args[0] != m.key
_other_db = lambda m, s: s.args[0] != m.db
_partly = lambda m: m.nq > 1 and 0 < len(m.keyq) < m.nq and m.key is not None      # key slots of some queries only

B2B = S("run", "back_to_back")
R = S("run")


class Walk:
    def __init__(self, name, N, L, t, steps, pairs, distinct, refusals):
        """refusals: the names of the `refused` steps the walk must hold, each once"""
        self.name, self.N, self.L, self.t, self.steps, self.pairs, self.distinct = name, N, L, t, steps, pairs, distinct
        self.refusals = refusals

    def index(self, name):
        hits = [i for i, s in enumerate(self.steps) if s.name == name]
        assert len(hits) == 1, "step %r occurs %d times in walk %s" % (name, len(hits), self.name)
        return hits[0]


def _queue_block(name=""):
    """queues 1 -> 2 -> 1 -> 2, two runs back to back behind each"""
    return [S("queues", 1, name=name), B2B, S("queues", 2), B2B, S("queues", 1), B2B, S("queues", 2), B2B]


# small: N = 4096, L = 3, t = T16, default chain: the 32-coefficient route, drops on chain_drop_kernel, no x_direct, no fused tensor
# load.  The plan of this ring HAS a lane order (ntt_plan_decide: every ring from 2^12 under the default chain), so the lane-ordered
# twins evk_sigma, evkq_sigma and masks_sigma exist here too and this walk's key and database steps hold them as well as `fused`'s do:
# a same-shape database load that skips make_masks_sigma fails this walk at full level (graph_db_same_shape), not only under a schedule.
# The long walk: every kind of step.
_SMALL = [
    # 0. the reverse of the suite's order: a schedule on a fresh handle, then the key, then a database.  K = 2 first, so that the only
    # product runs on level 3 and level 2 has no masks until K = 3 arrives
    S("sched", (3, 2), name="sched_first"),
    S("key", "k0", name="key_after_sched"),
    S("db", "B", name="db_after_sched"),
    S("query", "q0"), R,
    S("db", "A", name="masks_K2_to_K3"),
    S("refused", S("run"), ESTATE, "setIndex", name="run_after_db"),
    S("query", "q0"), R,
    # 1. the level's copies of the handle's key
    S("key", "k1", name="level_key"), R,
    S("key_seeded", "s0", name="level_key_seeded"), R,
    # 2. the level's masks: same shape (buffers kept), then more bin layers than the level's copy has room for
    S("db", "A2", name="level_masks_same_shape"), S("query", "q0"), R,
    S("db", "D", name="level_masks_more_layers"), S("query", "q1"), R,
    # 3. one and two queues, b = 5 and b = 3, under the schedule
    *_queue_block("queues_b5"),
    S("db", "A"), S("query", "q1"),
    *_queue_block("queues_b3"),
    S("queues", 1),
    # 4. a batch under the schedule: per-query keys, the slots nobody loaded, and the level's copies of both
    S("batch", 3), S("query", "q2", 1), S("query", "q3", 2), R,
    S("key_q", "k2", 0), S("key_q", "k3", 2), R,
    S("key", "k0", name="unloaded_slots_level"), R,
    S("batch", 2, name="level_evkq_shrink"), R,                  # the handle's key on every row
    S("key_q", "k2", 0), R,
    S("batch", 3, name="level_evkq_grow"),
    S("refused", S("run"), ESTATE, "query of the batch", name="run_after_batch_grew"),
    S("query", "q3", 2), R,                                      # the handle's key on every row
    S("key_q", "k3", 1),
    S("refused", S("key_q", "k2", 3), EINVAL, "batch", name="key_q_outside"), R,
    # 5. the same slots on every limb
    S("sched", (3,)), R,
    S("key", "k1", name="unloaded_slots_full"), R,
    # 6. the workspace: rows 9 -> 3 -> 6 within its capacity; databases A -> B -> A; 10 rows, beyond it; K 3 -> 1 -> 2
    S("batch", 1, name="ws_batch_3_1"), R,
    S("key_q", "k2", 0, name="key_q_single"), R,
    S("key", "k3", name="key_after_key_q_single"), S("query", "q2"), R,       # query 0 keeps its own key
    S("sched", (3, 2), name="level_key_q_single"), R,                         # ... and the level reads its copy of it
    S("sched", (3,)),
    S("batch", 2, name="ws_batch_1_2"), S("query", "q3", 1), R,
    S("db", "B", name="ws_db_A_B"), S("query", "q0"), S("query", "q1", 1), R,
    S("db", "A", name="ws_db_B_A"), S("query", "q0"), S("query", "q1", 1), R,
    S("db", "D", name="ws_rows_beyond"), S("query", "q0"), S("query", "q1", 1), R,
    S("db", "C", name="ws_K_3_1"), S("query", "q0"), S("query", "q1", 1), R,
    S("sched", (2,)), S("relin", False), S("query", "q2"), R,     # K = 1: neither setting is read
    S("db", "B", name="ws_K_1_2"), S("query", "q0"), S("query", "q1", 1), R,   # both are now: level 2, three components, no key
    S("sched", (3,)), S("relin", True), R,
    # 7. result rows.  (a) three components at nq = 1, then a larger batch
    S("batch", 1), S("db", "A"), S("query", "q0"), R,
    S("relin", False, name="res_relin_off_nq1"), R,
    S("batch", 3, name="res_batch_after_relin_off"), S("query", "q1", 1), S("query", "q2", 2), R,
    S("relin", True), R,
    # (b) keep = 1, then a last level of 1 (no reduction left), then back
    S("keep", 1, name="res_keep_1"), R,
    S("sched", (3, 1), name="res_sched_to_keep"), R,
    S("sched", (3,), name="res_sched_back"), R,
    S("keep", 3), S("batch", 1), R,
    # (c) three components, then K = 1 (two again), then K = 2
    S("relin", False, name="res_relin_off_K3"), R,
    S("db", "C", name="res_db_K1"), S("query", "q0"), R,
    S("db", "B", name="res_db_K2"), S("query", "q0"), R,
    S("relin", True), R,
    # 8. the host path: the page-locked result array follows keep and the schedule; a finished expansion does not come back
    S("db", "A"), S("run_host", ("q1",), name="host_plain"),
    S("keep", 2, name="host_keep"), S("run_host", ("q2",)),
    S("sched", (3, 1), name="host_sched"), S("run_host", ("q1",)),
    S("sched", (3,)), S("keep", 3),
    S("run_host_seeded", ("s1",), name="host_seeded"),
    S("query", "q0", name="query_after_seeded"), R,
    S("batch", 2), S("run_host", ("q1", "q2")),
    S("batch", 1),
    # 9. the captured graph: every change follows two replays
    S("keep", 2),
    S("refused", S("graph", True), ESTATE, "result_limbs", name="graph_below_keep"), R,
    S("keep", 3),
    S("graph", True), R, R, R,
    S("query", "q2", name="graph_query"), R, R, R,                          # same address, new contents
    S("query_dev", "q3", name="graph_query_dev"), R, R, R,                  # another address
    S("run_into", "u", name="graph_run_into"), S("run_into", "u"), S("run_into", "u"),
    S("key", "k0", name="graph_key"), R, R, R,
    S("db", "A2", name="graph_db_same_shape"), S("query", "q0"), R, R, R,
    S("db", "B", name="graph_db_other_shape"), S("query", "q0"), R, R, R,
    S("db", "A"), S("query", "q1"), R, R, R,
    S("queues", 2, name="graph_queues"), R, R, R,
    S("slots", 7, name="graph_slots"), R, R, R,
    S("profiling", True, name="graph_profiling"), R, S("profiling", False), R, R, R,
    S("key_q", "k2", 0, name="graph_key_q"), R, R, R,                       # the graph was captured with the handle's key
    S("refused", S("sched", (3, 2)), ESTATE, "graph", name="sched_under_graph"), R,
    S("refused", S("keep", 2), ESTATE, "graph", name="keep_under_graph"), R,
    S("refused", S("relin", False), ESTATE, "graph", name="relin_under_graph"), R,
    S("slots", 0), S("queues", 1),
    S("graph", False, name="graph_off"),
    S("sched", (3, 2), name="sched_after_graph"), R,
    S("refused", S("graph", True), ESTATE, "chain_limbs", name="graph_below_L"), R,
    S("sched", (3,)),
    S("graph", True, name="graph_on_again"), R, R,
    S("graph", False), R,
]

_SMALL_PAIRS = [
    # level copies <- sched on a fresh handle before any key or database, then key, then db
    P("sched_first", "sched", change=lambda m, s: m.db is None and m.key is None, after=lambda m: m.key and m.db and min(m.sched) < m.L),
    P("key_after_sched", "key", change=lambda m, s: m.db is None and min(m.sched) < m.L, after=lambda m: m.db is not None),
    P("db_after_sched", "db", change=lambda m, s: m.key is not None and min(m.sched) < m.L),
    # level masks <- db B -> A under (L, L - 1): the last product's level moves from L to L - 1
    P("masks_K2_to_K3", "db", before=lambda m: m.K == 2 and m.sched == (m.L, m.L - 1), change=_other_db, after=_level3),
    P("level_key", "key", before=_level3, change=_other_key),
    P("level_key_seeded", "key_seeded", before=_level3, change=_other_key),
    P("level_masks_same_shape", "db", before=_level3, change=lambda m, s: s.args[0] != m.db and m.dbs[s.args[0]] == m.dbs[m.db]),
    P("level_masks_more_layers", "db", before=_level3, change=lambda m, s: m.dbs[s.args[0]][1] > max(v[1] for v in m.dbs.values() if v != m.dbs[s.args[0]])),
    # unloaded key slots <- key after key_q for some queries only: under a schedule below L, and at full level
    P("unloaded_slots_level", "key", before=lambda m: _partly(m) and _level3(m), change=_other_key),
    P("unloaded_slots_full", "key", before=lambda m: _partly(m) and not m.below(), change=_other_key),
    # level evkq <- batch 3 -> 2 -> 3
    P("level_evkq_shrink", "batch", before=lambda m: m.nq == 3 and m.keyq and _level3(m), change=lambda m, s: s.args[0] == 2,
      after=lambda m: not m.keyq and _level3(m)),
    P("level_evkq_grow", "batch", before=lambda m: m.nq == 2 and m.keyq and _level3(m), change=lambda m, s: s.args[0] == 3,
      after=lambda m: not m.keyq and _level3(m)),
    # workspace capacity
    P("ws_batch_3_1", "batch", before=lambda m: m.nq == 3, change=lambda m, s: s.args[0] == 1, after=lambda m: m.nq == 1),
    P("ws_batch_1_2", "batch", before=lambda m: m.nq == 1, change=lambda m, s: s.args[0] == 2, after=lambda m: m.nq == 2),
    P("ws_db_A_B", "db", before=lambda m: m.db == "A", change=lambda m, s: s.args[0] == "B", after=lambda m: m.db == "B"),
    P("ws_db_B_A", "db", before=lambda m: m.db == "B", change=lambda m, s: s.args[0] == "A", after=lambda m: m.db == "A"),
    P("ws_rows_beyond", "db", before=lambda m: m.nq == 2, change=lambda m, s: m.dbs[s.args[0]][1] * m.nq > 9, after=lambda m: m.nq == 2),
    P("ws_K_3_1", "db", before=lambda m: m.K == 3, change=lambda m, s: m.dbs[s.args[0]][0] == 1, after=lambda m: m.K == 1),
    P("ws_K_1_2", "db", before=lambda m: m.K == 1, change=lambda m, s: m.dbs[s.args[0]][0] == 2, after=lambda m: m.K == 2),
    # a batch of one: query 0's own key
    P("key_q_single", "key_q", before=lambda m: m.nq == 1 and m.key_read(), change=lambda m, s: s.args[0] != m.key),
    P("key_after_key_q_single", "key", before=lambda m: _own_key(m) and not m.below(), change=_other_key),
    P("level_key_q_single", "sched", before=lambda m: _own_key(m) and not m.below(), change=lambda m, s: min(s.args[0]) < m.L,
      after=lambda m: _own_key(m) and m.K >= 3 and m.last < m.L),
    # result rows
    P("res_relin_off_nq1", "relin", before=lambda m: m.nq == 1 and m.K >= 2 and m.relin, change=lambda m, s: not s.args[0],
      after=lambda m: m.nq == 1 and not m.relin),
    P("res_batch_after_relin_off", "batch", before=lambda m: m.nq == 1 and m.K >= 2 and not m.relin, change=lambda m, s: s.args[0] == 3,
      after=lambda m: m.nq == 3 and not m.relin),
    P("res_keep_1", "keep", before=lambda m: m.keep == m.L and not m.below(), change=lambda m, s: s.args[0] == 1, after=lambda m: m.keep == 1),
    P("res_sched_to_keep", "sched", before=lambda m: m.keep == 1 and not m.below(), change=lambda m, s: s.args[0][-1] == 1,
      after=lambda m: m.keep >= m.last),
    P("res_sched_back", "sched", before=lambda m: m.keep >= m.last and m.below(), change=lambda m, s: min(s.args[0]) == m.L,
      after=lambda m: m.keep == 1 and not m.below()),
    P("res_relin_off_K3", "relin", before=lambda m: m.K == 3 and m.relin, change=lambda m, s: not s.args[0], after=lambda m: not m.relin),
    P("res_db_K1", "db", before=lambda m: m.K >= 2 and not m.relin, change=lambda m, s: m.dbs[s.args[0]][0] == 1,
      after=lambda m: m.K == 1 and not m.relin),
    P("res_db_K2", "db", before=lambda m: m.K == 1 and not m.relin, change=lambda m, s: m.dbs[s.args[0]][0] == 2,
      after=lambda m: m.K == 2 and not m.relin),
    # the host path
    P("host_keep", "keep", before=lambda m: m.keep == m.L, change=lambda m, s: s.args[0] < m.L, after=lambda m: m.keep < m.L),
    P("host_sched", "sched", before=lambda m: not m.below(), change=lambda m, s: min(s.args[0]) < m.L, after=lambda m: m.below()),
    P("query_after_seeded", "query", before=lambda m: m.slot[0].startswith("s"), change=lambda m, s: not s.args[0].startswith("s"),
      after=lambda m: True),
    # the captured graph
    P("graph_query", "query", before=on_graph, change=lambda m, s: s.args[0] != m.slot[0], replays=2),
    P("graph_query_dev", "query_dev", before=on_graph, change=lambda m, s: s.args[0] != m.slot[0], replays=2),
    P("graph_run_into", "run_into", before=on_graph, replays=2),
    P("graph_key", "key", before=on_graph, change=_other_key, replays=2),
    P("graph_db_same_shape", "db", before=on_graph, change=lambda m, s: s.args[0] != m.db and m.dbs[s.args[0]] == m.dbs[m.db], replays=2),
    P("graph_db_other_shape", "db", before=on_graph, change=lambda m, s: m.dbs[s.args[0]] != m.dbs[m.db], replays=2),
    P("graph_queues", "queues", before=on_graph, change=lambda m, s: s.args[0] != m.queues and m.b >= 2, replays=2),
    P("graph_slots", "slots", before=on_graph, change=lambda m, s: s.args[0] != m.slots, replays=2),
    P("graph_profiling", "profiling", before=on_graph, change=lambda m, s: s.args[0], after=lambda m: m.graph and m.profiling, replays=2),
    P("graph_key_q", "key_q", before=lambda m: on_graph(m) and not m.keyq, change=lambda m, s: s.args[1] == 0 and s.args[0] != m.key,
      after=lambda m: on_graph(m) and _own_key(m), replays=2),
    P("graph_off", "graph", before=on_graph, change=lambda m, s: not s.args[0], after=lambda m: not m.graph and m.below()),
    P("sched_after_graph", "sched", change=lambda m, s: not m.graph and min(s.args[0]) < m.L, after=lambda m: m.below()),
    P("graph_on_again", "graph", before=lambda m: not m.graph, change=lambda m, s: s.args[0] and not m.below(), after=on_graph),
]

# fused: N = 16384, L = 4, t = T32, default chain: lane-ordered twins, x_direct (nq > 1), the fused tensor load, d01_eval_q, fused drops,
# folded conversions.  The pairs on the lane-ordered twins again, read by the routes only this ring takes, two queues and the graph.
_FUSED = [
    S("queues", 1), S("key", "k0"), S("db", "A"), S("batch", 2), S("query", "q0"), S("query", "q1", 1), R,
    S("key", "k1", name="evk_sigma_key"), R,
    S("key_seeded", "s0", name="evk_sigma_key_seeded"), R,
    S("key_q", "k2", 0), R,
    S("key", "k0", name="evkq_sigma_unloaded_full"), R,
    S("db", "A2", name="masks_sigma_same_shape"),
    S("refused", S("run"), ESTATE, "setIndex", name="run_after_db"),
    S("query", "q0"), S("query", "q1", 1), R,
    S("sched", (4, 3)), R,
    S("key", "k1", name="evkq_sigma_unloaded_level"), R,
    S("sched", (4,)),
    S("queues", 2, name="two_queues"), B2B,
    S("batch", 1),
    S("graph", True), R, R, R,
    S("query", "q1", name="graph_query"), R, R, R,
    S("key", "k0", name="graph_key"), R, R,
    S("graph", False), R,
]

_FUSED_PAIRS = [
    P("evk_sigma_key", "key", before=lambda m: m.key_read() and not m.keyq, change=_other_key),
    P("evk_sigma_key_seeded", "key_seeded", before=lambda m: m.key_read() and not m.keyq, change=_other_key),
    P("evkq_sigma_unloaded_full", "key", before=lambda m: _partly(m) and not m.below(), change=_other_key),
    P("masks_sigma_same_shape", "db", before=lambda m: m.key_read(), change=lambda m, s: s.args[0] != m.db and m.dbs[s.args[0]] == m.dbs[m.db]),
    P("evkq_sigma_unloaded_level", "key", before=lambda m: _partly(m) and _level3(m), change=_other_key),
    P("two_queues", "queues", before=lambda m: m.queues == 1 and m.nq > 1, change=lambda m, s: s.args[0] == 2 and m.b >= 2,
      after=lambda m: m.queues == 2 and m.nq > 1),
    P("graph_query", "query", before=on_graph, change=lambda m, s: s.args[0] != m.slot[0], replays=2),
    P("graph_key", "key", before=on_graph, change=_other_key, replays=2),
]

# own_key: small's ring, a handle that never had a key of its own when query 0's arrives: the only key is in the per-query array, at
# full level and on a level context; the handle's key, loaded later, changes nothing until a batch change forgets query 0's
_OWN_KEY = [
    S("db", "A"), S("query", "q0"),
    S("refused", S("run"), ESTATE, "key", name="run_without_key"),
    S("key_q", "k2", 0, name="only_key_q"), R,
    S("sched", (3, 2), name="only_key_q_level"), R,
    S("key", "k0", name="key_after_only_key_q"), S("query", "q1"), R,
    S("sched", (3,)),
    S("batch", 2, name="batch_forgets_only_key_q"), S("query", "q2", 1), R,
]

_no_key = lambda m: m.key is None and _own_key(m)
_OWN_KEY_PAIRS = [
    P("only_key_q", "key_q", change=lambda m, s: m.key is None and not m.keyq and m.nq == 1 and m.key_read(), after=lambda m: _no_key(m) and not m.below()),
    P("only_key_q_level", "sched", before=lambda m: _no_key(m) and not m.below(), change=lambda m, s: min(s.args[0]) < m.L,
      after=lambda m: _no_key(m) and m.last < m.L),
    P("key_after_only_key_q", "key", before=lambda m: _no_key(m) and m.last < m.L, change=lambda m, s: s.args[0] != m.keyq[0],
      after=lambda m: _own_key(m) and m.key is not None),
    P("batch_forgets_only_key_q", "batch", before=lambda m: _own_key(m) and m.key is not None, change=lambda m, s: s.args[0] == 2,
      after=lambda m: not m.keyq and m.nq == 2),
]

# distinct: the least number of different expected results among the runs of a walk
SMALL = Walk("small", 4096, 3, T16, _SMALL, _SMALL_PAIRS, distinct=48,
             refusals=("run_after_db", "run_after_batch_grew", "key_q_outside", "graph_below_keep", "sched_under_graph", "keep_under_graph",
                       "relin_under_graph", "graph_below_L"))
FUSED = Walk("fused", 16384, 4, T32, _FUSED, _FUSED_PAIRS, distinct=12, refusals=("run_after_db",))
OWN_KEY = Walk("own_key", 4096, 3, T16, _OWN_KEY, _OWN_KEY_PAIRS, distinct=4, refusals=("run_without_key",))
WALKS = {"small": SMALL, "fused": FUSED, "own_key": OWN_KEY}


def pieces(walk):
    """[(label, first, end)]: the first twelve steps, and the rest in two halves"""
    n = len(walk.steps)
    mid = 12 + (n - 12) // 2
    return [("first", 0, 12), ("middle", 12, mid), ("last", mid, n)]


def piece_steps(walk, first, end):
    """the steps [first, end) of a walk behind the shortest set-up of the state they start in"""
    return states(walk)[first].setup() + list(walk.steps[first:end])


# ---- data and the reference ------------------------------------------------------------------------------------------------------
def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def rand_limbs(rng, moduli, shape_prefix, N):
    out = np.zeros(tuple(shape_prefix) + (len(moduli), N), dtype=np.uint64)
    for i, m in enumerate(moduli):
        out[..., i, :] = rng.integers(0, int(m), tuple(shape_prefix) + (N,), dtype=np.uint64)
    return out


class Data:
    """the arrays behind the names of a walk, drawn once per name from a generator seeded by it.  Names that begin with "s" are
    seeded: their second components are expand(seeds) -- the device's expansion (PieContext.expand_uniform), handed in by the caller"""

    def __init__(self, o, dbs=DBS, expand=None):
        self.o, self.dbs, self.expand, self._memo = o, dbs, expand, {}

    def _once(self, key, make):
        if key not in self._memo:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    def db(self, name):
        """(db[K][b][E][L][N], masks[b][L][N])"""
        K, b, E = self.dbs[name]
        o = self.o

        def make():
            rng = _rng("db", name, o.N, o.L)
            return rand_limbs(rng, o.q, (K, b, E), o.N), rand_limbs(rng, o.q, (b,), o.N)
        return self._once(("db", name), make)

    def seeded_key(self, name):
        """(evk0[L][L][N], seeds[L][32])"""
        o = self.o

        def make():
            rng = _rng("key", name, o.N, o.L)
            return rand_limbs(rng, o.q, (o.L,), o.N), rng.integers(0, 256, (o.L, 32), dtype=np.uint8)
        return self._once(("key0", name), make)

    def key(self, name):
        """evk[L][2][L][N]"""
        o = self.o

        def make():
            if name.startswith("s"):
                evk0, seeds = self.seeded_key(name)
                return np.ascontiguousarray(np.stack([evk0, self.expand(seeds)], axis=1))
            return rand_limbs(_rng("key", name, o.N, o.L), o.q, (o.L, 2), o.N)
        return self._once(("key", name), make)

    def seeded_query(self, db, name):
        """(c0 of the index matrix [K][E][L][N], its seeds [K][E][32], c0 of the minus element [L][N], its seed [32])"""
        K, _, E = self.dbs[db]
        o = self.o

        def make():
            rng = _rng("query", name, K, E, o.N, o.L)
            return (rand_limbs(rng, o.q, (K, E), o.N), rng.integers(0, 256, (K, E, 32), dtype=np.uint8),
                    rand_limbs(rng, o.q, (), o.N), rng.integers(0, 256, (32,), dtype=np.uint8))
        return self._once(("query0", name, K, E), make)

    def query(self, db, name):
        """(idx[K][E][2][L][N], minus[2][L][N]) of query `name` for a database of db's K and E"""
        K, _, E = self.dbs[db]
        o = self.o

        def make():
            if name.startswith("s"):
                c0i, si, c0m, sm = self.seeded_query(db, name)
                a = self.expand(np.concatenate([si.reshape(K * E, 32), sm[None]]))
                return (np.ascontiguousarray(np.stack([c0i, a[:K * E].reshape(K, E, o.L, o.N)], axis=2)),
                        np.ascontiguousarray(np.stack([c0m, a[K * E]])))
            rng = _rng("query", name, K, E, o.N, o.L)
            return rand_limbs(rng, o.q, (K, E, 2), o.N), rand_limbs(rng, o.q, (2,), o.N)
        return self._once(("query", name, K, E), make)


class Reference:
    """expected result arrays [nq][b][2 or 3][limbs][N] of a Config by the exact definitions, memoised per (database, query, key, levels,
    relin) and bin layer, and per row limbs on top"""

    def __init__(self, ob, data):
        from tests.test_chain_schedule import level_oracles
        self.ob, self.data, self.o = ob, data, data.o
        self.levels = level_oracles(ob, self.o, range(1, self.o.L + 1))
        self._layers, self._blocks = {}, {}

    def _jobs(self, cfg):
        b = self.data.dbs[cfg.db][1]
        return [(cfg.db, q, k, cfg.levels, cfg.relin, bn) for q, k in zip(cfg.queries, cfg.keys) for bn in range(b)]

    def _layer(self, job):
        from tests.test_chain_schedule import schedule_layer_exact
        db_name, q, k, levels, relin, bn = job
        o = self.o
        db, masks = self.data.db(db_name)
        idx, minus = self.data.query(db_name, q)
        evk = self.data.key(k) if k is not None else None
        if relin and all(l == o.L for l in levels) and evk is not None:
            return o.pie_run(idx, minus, db, masks, evk, bn, bn + 1)[bn]         # the default configuration
        return schedule_layer_exact(o, self.levels, idx, minus, db, masks, evk, list(levels) or [o.L], bn, relin)

    def prepare(self, configs, workers=12):
        """every layer the configurations need that is not there yet, through a thread pool"""
        import concurrent.futures
        jobs = []
        for cfg in configs:
            for qn in cfg.queries:       # (the arrays are drawn here, on one thread)
                self.data.query(cfg.db, qn)
            jobs += [j for j in self._jobs(cfg) if j not in self._layers and j not in jobs]
        for j in jobs:
            if j[2] is not None:
                self.data.key(j[2])
            self.data.db(j[0])
        with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
            for j, row in zip(jobs, pool.map(self._layer, jobs)):
                self._layers[j] = row

    def __call__(self, cfg):
        from tests.test_result_limbs import mod_reduce_exact
        if cfg not in self._blocks:
            self.prepare([cfg])
            b = self.data.dbs[cfg.db][1]
            rows = np.stack([self._layers[j] for j in self._jobs(cfg)])
            rows = rows.reshape((len(cfg.queries), b) + rows.shape[1:])
            at = rows.shape[-2]
            assert at == (cfg.levels[-1] if cfg.levels else self.o.L) and cfg.limbs <= at
            if cfg.limbs < at:
                rows = mod_reduce_exact(self.levels[at], rows, cfg.limbs)
            rows.setflags(write=False)
            self._blocks[cfg] = rows
        return self._blocks[cfg]
