"""Chain schedule on the GPU (include/piehip.h "Chain limbs", piehip_set_chain_schedule): run() with a limb count per product on the
fused conversions and on the drop kernel's fallback, the settings a schedule composes with, the refusals, and a real client.

Every comparison is bit for bit, on every word, against run_chain_schedule_exact's layers (tests/test_chain_schedule.py) on random
limbs.  Each point's route is written beside it and asserted from the profile: the class limb_drop is there exactly on the fallback
points (a library built with -DPIEHIP_CHAIN_DROP_FUSED=0, run with PIEHIP_TEST_CHAIN_DROP_FUSED=0, shows it on every point).
E = 2 and b <= 3 throughout.
"""
import concurrent.futures
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T16, T32
from tests.test_chain_schedule import last_level, level_oracles, schedule_layer_exact
from tests.test_gpu_chain_drop_columns import _drop_launched, _profiled
from tests.test_gpu_chain_limbs import _by_query, _contexts, _database, _keys, _load_keys, _queries, _set_queries
from tests.test_gpu_parity import rand_limbs
from tests.test_result_limbs import mod_reduce_exact

pytestmark = pytest.mark.gpu

E = 2


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _exact(ob, o, queries, db, masks, evks, sched, relin_last=True):
    """[nq][b][2 or 3][l_last][N] by the definition, one task per (query, bin layer)"""
    levels = level_oracles(ob, o, sched)
    b = db.shape[1]
    jobs = [(i, bn) for i in range(len(queries)) for bn in range(b)]

    def one(job):
        i, bn = job
        return schedule_layer_exact(o, levels, queries[i][0], queries[i][1], db, masks, evks[i], list(sched), bn, relin_last)
    with concurrent.futures.ThreadPoolExecutor(max_workers=12) as pool:
        rows = list(pool.map(one, jobs))
    return np.stack(rows).reshape((len(queries), b) + rows[0].shape)


def _run(op):
    op.run()
    return _by_query(op, op.getResultList()).copy()


def _check_route(prof, route):
    assert ("limb_drop" in prof) == _drop_launched(route), "route %s: classes %s" % (route, sorted(prof))
    assert "expand" in prof


# ---- 1. run() on both routes ---------------------------------------------------------------------------------------------------------
# (N, L, chain, K, schedule, b, nq, route).  fused: every drop of the chain rides in a conversion's load phase (folded rings, moduli in
# (2^59, 2^60), source and target levels the conversion is built for); fallback: chain_drop_kernel and plain conversions.
POINTS = [
    (16384, 4, None, 3, (4, 3), 1, 1, "fused"),       # C3's ring: X of the second product comes from the product array
    (16384, 4, None, 3, (4, 3), 3, 3, "fused"),       # a batch on two queues: the workspace rows of groups in different products
    (16384, 4, None, 3, (3, 2), 1, 1, "fused"),       # X from level 3, Y from 4, both to 2
    (16384, 4, None, 4, (4, 4, 3), 1, 1, "fused"),
    (16384, 4, None, 4, (4, 3, 2), 1, 1, "fused"),
    (16384, 6, None, 3, (5, 4), 1, 1, "fused"),       # the drop body (6,4) for Y
    (16384, 6, None, 3, (4, 3), 1, 1, "fused"),       # (6,4) for both operands, then (6,3) for Y and (4,3) for X
    (32768, 6, None, 3, (4, 3), 1, 1, "fused"),       # the ring of 2^15, transformed in slices of 2^14
    (16384, 2, None, 3, (2, 1), 1, 1, "fused"),
    (16384, 7, None, 3, (7, 6), 1, 1, "fused"),
    (4096, 4, None, 3, (4, 3), 2, 1, "fallback"),     # an unfolded ring
    (4096, 4, None, 3, (4, 2), 2, 1, "fallback"),
    (4096, 4, None, 3, (3, 2), 2, 1, "fallback"),
    (4096, 4, None, 4, (3, 2, 1), 2, 2, "fallback"),  # a drop between every pair of products
    (16384, 5, None, 3, (5, 3), 1, 1, "fallback"),    # a folded ring, a pair the conversion is not built for
    (16384, 4, 1 << 50, 3, (4, 3), 1, 1, "fallback"),  # a chain outside (2^59, 2^60)
    (16384, 4, "one_p_61", 3, (4, 3), 1, 1, "fallback"),  # the parent does not fold, the level does
    # the triple (6,5,4) of expand_both_drop_xy_kernel (Y from 6 limbs, X from 5, both to 4) under the Barrett kind of the column-sum
    # reduction, and on a chain whose level 5 is of the Barrett kind and whose level 4 folds (param_chains.over_at)
    (16384, 6, "barrett_60", 3, (5, 4), 1, 1, "fused"),
    (16384, 6, "q4_over", 3, (5, 4), 1, 1, "fused"),
]
# PieContext.reduction() of the handle and of every level of the schedule, for the points that name a chain by its kind; every
# default-chain point is "fold" throughout
REDUCTION = {"barrett_60": {6: "barrett", 5: "barrett", 4: "barrett"}, "q4_over": {6: "barrett", 5: "barrett", 4: "fold"}}


@pytest.mark.parametrize("N,L,chain,K,sched,b,nq,route", POINTS,
                         ids=["%d-L%d-%s-K%d-%s-b%d-nq%d-%s" % (p[0], p[1], p[2], p[3], "".join(map(str, p[4])), p[5], p[6], p[7]) for p in POINTS])
def test_run_with_a_schedule(ob, pie, N, L, chain, K, sched, b, nq, route):
    """every word against the definition, on one queue and (b >= 2) on two; the profiled run gives the same bits and names the route;
    back at the default the handle gives the bits of a handle that never had a schedule"""
    o, cc = _contexts(ob, pie, N, L, T32, chain)
    rng = np.random.default_rng(N + 100 * K + 10 * b + nq + L + sum(sched))
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    evks = _keys(o, rng, nq)
    queries = _queries(o, rng, K, E, nq)
    _set_queries(op, queries)
    _load_keys(cc, op, evks)
    never = _run(op)
    want = _exact(ob, o, queries, db, masks, evks, sched)
    op.setChainSchedule(sched)
    assert op.chainSchedule() == list(sched) and op.chainLimbs() == last_level(sched, K)
    if chain is None or chain in REDUCTION:
        for lv in (L,) + tuple(sched):
            assert cc.reduction(level=lv) == ("fold" if chain is None else REDUCTION[chain][lv]), "the kind of level %d" % lv
    for streams in ((1, 2) if b >= 2 else (1,)):
        cc.set_run_streams(streams)
        got = _run(op)
        assert got.shape == (nq, b, 2, last_level(sched, K), N)
        assert (got == want).all(), "queues %d" % streams
    cc.set_run_streams(1)
    got, prof = _profiled(cc, lambda: _run(op))
    assert (got == want).all()
    _check_route(prof, route)
    op.setChainLimbs(L)
    assert op.chainSchedule() == [L]
    assert (_run(op) == never).all()
    cc.close()


# ---- 2. the settings around a schedule: (4,3) at C3's ring, K = 3 -------------------------------------------------------------------
N3, L3, K3, B3, NQ3, SCHED3 = 16384, 4, 3, 2, 3, (4, 3)


@pytest.fixture(scope="module")
def c3(ob, pie):
    """one database, three queries with a key each, and their rows by the definition; query 0 has seeded c1 halves"""
    o, cc = _contexts(ob, pie, N3, L3, T32)
    rng = np.random.default_rng(4343)
    db, masks = rand_limbs(rng, o.q, (K3, B3, E), N3), rand_limbs(rng, o.q, (B3,), N3)
    evks = _keys(o, rng, NQ3)
    queries = _queries(o, rng, K3, E, NQ3)
    seeds = rng.integers(0, 256, (K3 * E + 1, 32), dtype=np.uint8)
    a = cc.expand_uniform(seeds)
    cc.close()
    queries[0][0][:, :, 1] = a[:K3 * E].reshape(K3, E, L3, N3)
    queries[0][1][1] = a[K3 * E]
    want = _exact(ob, o, queries, db, masks, evks, SCHED3)
    for v in (db, masks, want) + tuple(evks) + tuple(x for q in queries for x in q):
        v.setflags(write=False)
    return dict(o=o, db=db, masks=masks, evks=evks, queries=queries, seeds=seeds, want=want)


def _c3_operator(pie, c3, nq):
    cc = pie.PieContext(N3, L3, T32)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=c3["db"], preCalcRandomMask=c3["masks"])
    if nq > 1:
        op.setQueryBatch(nq)
    _set_queries(op, c3["queries"][:nq])
    return cc, op


def test_degree_two_results_need_the_first_products_key_alone(ob, pie, c3):
    """piehip_set_result_relin(0): the first product relinearises on all limbs with the handle's key; the last one, on three limbs,
    goes out as a tensor product, and both keep forms follow"""
    o = c3["o"]
    cc, op = _c3_operator(pie, c3, 1)
    cc.load_relin_key(c3["evks"][0])
    op.setChainSchedule(SCHED3)
    op.setResultRelin(False)
    want3 = _exact(ob, o, c3["queries"][:1], c3["db"], c3["masks"], c3["evks"][:1], SCHED3, relin_last=False)
    got, prof = _profiled(cc, lambda: _run(op))
    assert got.shape == (1, B3, 3, 3, N3) and (got == want3).all()
    _check_route(prof, "fused")
    op.setResultLimbs(2)
    got = _run(op)
    assert got.shape == (1, B3, 3, 2, N3) and (got == mod_reduce_exact(level_oracles(ob, o, SCHED3)[3], want3, 2)).all()
    cc.close()


@pytest.mark.parametrize("keep", [2, 1])
def test_result_limbs_below_the_last_level(ob, pie, c3, keep):
    o = c3["o"]
    cc, op = _c3_operator(pie, c3, 1)
    cc.load_relin_key(c3["evks"][0])
    op.setChainSchedule(SCHED3)
    op.setResultLimbs(keep)
    got = _run(op)
    assert got.shape == (1, B3, 2, keep, N3)
    assert (got == mod_reduce_exact(level_oracles(ob, o, SCHED3)[3], c3["want"][:1], keep)).all()
    cc.close()


def test_a_key_per_query(pie, c3):
    cc, op = _c3_operator(pie, c3, NQ3)
    _load_keys(cc, op, c3["evks"])
    op.setChainSchedule(SCHED3)
    for streams in (1, 2):
        cc.set_run_streams(streams)
        got = _run(op)
        assert got.shape == (NQ3, B3, 2, 3, N3)
        for i in range(NQ3):
            assert (got[i] == c3["want"][i]).all(), "query %d, %d queue(s)" % (i, streams)
    cc.close()


def test_host_path_and_a_seeded_query(pie, c3):
    """piehip_run_host with the page-locked result array sized by the last level; the same query with its c1 halves from seeds"""
    cc, op = _c3_operator(pie, c3, 1)
    cc.load_relin_key(c3["evks"][0])
    op.setChainSchedule(SCHED3)
    idx, minus = (np.array(v) for v in c3["queries"][0])
    assert op.hostBuffers()[2].shape == (B3, 2, 3, N3)
    got = op.runHost(idx, minus)
    assert (got == c3["want"][0]).all()
    seeds = c3["seeds"]
    got = op.runHostSeeded(np.ascontiguousarray(idx[:, :, 0]), seeds[:K3 * E].reshape(K3, E, 32), np.ascontiguousarray(minus[0]), seeds[K3 * E])
    assert (got == c3["want"][0]).all()
    cc.close()


def test_a_query_slot_has_its_own_schedule(ob, pie, c3):
    """the owner on every limb, its slot on (4,3) with its own copies of the owner's key and masks; then the other way round"""
    o = c3["o"]
    cc, op = _c3_operator(pie, c3, 1)
    cc.load_relin_key(c3["evks"][0])
    cc2 = pie.PieContext(N3, L3, T32)
    slot = pie.BatchedFHEHIPPIE(cc2, attachTo=op)
    _set_queries(slot, c3["queries"][:1])
    q = c3["queries"][0]
    full = o.pie_run(np.array(q[0]), np.array(q[1]), np.array(c3["db"]), np.array(c3["masks"]), np.array(c3["evks"][0]))
    low = c3["want"][0]
    slot.setChainSchedule(SCHED3)
    assert (op.chainSchedule(), slot.chainSchedule()) == ([L3], list(SCHED3))
    op.run()
    slot.run()
    assert (op.getResultList() == full).all() and (slot.getResultList() == low).all()
    slot.setChainLimbs(L3)
    op.setChainSchedule(SCHED3)
    op.run()
    slot.run()
    assert (op.getResultList() == low).all() and (slot.getResultList() == full).all()
    del slot
    cc2.close()
    cc.close()


def test_schedule_off_and_on_again(pie, c3):
    cc, op = _c3_operator(pie, c3, 1)
    cc.load_relin_key(c3["evks"][0])
    op.setChainSchedule(SCHED3)
    first = _run(op)
    assert (first == c3["want"][:1]).all()
    op.setChainLimbs(L3)
    assert _run(op).shape == (1, B3, 2, L3, N3)
    op.setChainSchedule(SCHED3)
    assert (_run(op) == first).all()
    cc.close()


def test_two_hash_functions_take_the_first_entry_and_one_takes_none(ob, pie):
    """K = 2 with (4,3): the only product runs on four limbs, which is the default run; K = 1: unchanged"""
    for K in (2, 1):
        o, cc = _contexts(ob, pie, N3, L3, T32)
        rng = np.random.default_rng(70 + K)
        op, db, masks = _database(pie, o, cc, rng, K, E, 2, 1)
        evks = _keys(o, rng, 1)
        queries = _queries(o, rng, K, E, 1)
        _set_queries(op, queries)
        _load_keys(cc, op, evks)
        never = _run(op)
        op.setChainSchedule(SCHED3)
        assert op.chainSchedule() == list(SCHED3) and op.chainLimbs() == L3
        got = _run(op)
        assert got.shape == (1, 2, 2, L3, N3) and (got == never).all()
        cc.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(ob, pie):
    from nested_hashing_psi_amd._lib import lib, u64p
    N, L, K, b = 4096, 4, 3, 2
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(66)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, 1)
    evks = _keys(o, rng, 1)
    queries = _queries(o, rng, K, E, 1)
    _set_queries(op, queries)
    cc.load_relin_key(evks[0])
    full = _run(op)
    arr = lambda *v: (C.c_uint32 * max(len(v), 1))(*v)
    set_ = lambda *v: lib().piehip_set_chain_schedule(cc._h, arr(*v), len(v))
    n, buf = C.c_uint32(), arr(*[0] * 7)
    assert set_(3, 4) == pie.EINVAL            # increasing
    assert set_(4, 0) == pie.EINVAL            # entry 0
    assert set_(L + 1, 3) == pie.EINVAL        # entry above L
    assert set_() == pie.EINVAL                # n = 0
    assert set_(*[4] * 8) == pie.EINVAL        # n = 8
    assert lib().piehip_set_chain_schedule(cc._h, None, 2) == pie.EINVAL
    assert lib().piehip_get_chain_schedule(cc._h, buf, 7, C.byref(n)) == 0 and (n.value, buf[0]) == (1, L)
    kind = C.c_uint32()
    assert lib().piehip_get_level_reduction(cc._h, 3, C.byref(kind)) == pie.ESTATE     # a level no schedule has named
    assert set_(4, 3) == 0
    # a level's kind: the levels the schedule has built and the handle itself; not one it has not built, nor a count outside 1 .. L
    assert [lib().piehip_get_level_reduction(cc._h, lv, C.byref(kind)) for lv in (0, 2, L + 1)] == [pie.EINVAL, pie.ESTATE, pie.EINVAL]
    assert lib().piehip_get_level_reduction(cc._h, 3, None) == pie.EINVAL
    assert (cc.reduction(level=3), cc.reduction(level=L), cc.reduction()) == ("fold",) * 3
    assert lib().piehip_get_chain_schedule(cc._h, buf, 1, C.byref(n)) == pie.EINVAL    # no room
    assert lib().piehip_get_chain_schedule(cc._h, buf, 2, C.byref(n)) == 0 and (n.value, buf[0], buf[1]) == (2, 4, 3)
    assert set_(L) == 0
    # the captured graph and a schedule below L exclude each other, whichever comes second
    cc.set_graph(True)
    assert set_(4, 3) == pie.ESTATE and b"graph" in lib().piehip_last_error()
    assert set_(4, 4) == 0                     # what the graph runs: accepted
    assert (_run(op) == full).all()
    cc.set_graph(False)
    assert set_(4, 3) == 0
    assert lib().piehip_set_graph(cc._h, 1) == pie.ESTATE
    want = _exact(ob, o, queries, db, masks, evks, (4, 3))
    assert (_run(op) == want).all()
    # (4,4,3) with K = 3: no product runs below L, but an entry is below L -- the gather refuses all the same
    assert set_(4, 4, 3) == 0
    assert (_run(op) == full).all()
    p = u64p()
    assert lib().piehip_gather_results_host(cc._h, b, 0, C.byref(p)) == pie.ESTATE
    assert lib().piehip_gather_results(cc._h, b, 0, C.c_void_p(op.resultsDevicePtr())) == pie.ESTATE
    assert set_(L) == 0
    assert (_run(op) == full).all()
    cc.close()
    # a query-sliced handle refuses a schedule below L, and a handle with one refuses a sliced load
    cc = pie.PieContext(N, L, T16)
    sl = pie.QuerySlicedBatchedFHEHIPPIE([cc], vectorizedHCT=db, preCalcRandomMask=masks)
    assert set_(4, 3) == pie.ESTATE and b"sliced" in lib().piehip_last_error()
    assert set_(L, L) == 0
    del sl
    cc.close()
    cc = pie.PieContext(N, L, T16)
    assert set_(4, 3) == 0
    with pytest.raises(RuntimeError, match="piehip_set_chain_limbs"):
        pie.QuerySlicedBatchedFHEHIPPIE([cc], vectorizedHCT=db, preCalcRandomMask=masks)
    cc.close()


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def test_client_reads_rows_of_a_schedule(ob, pie):
    """a real client at C3's ring and t with K = 3, E = 14, b = 1: (4,3) gives exactly the full run's matches with budget left"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    N, L, t, sched = 16384, 4, T32, (4, 3)
    k, e, K, E_, b = 2, 16, 3, 14, 1
    o, cc = _contexts(ob, pie, N, L, t)
    rng = np.random.default_rng(N + 1)
    items = np.unique(rng.integers(1, 1 << 31, 400, dtype=np.uint64))[:150]
    rng.shuffle(items)
    server, clientSet = items[:140].copy(), np.concatenate([items[:5], items[140:150]])
    op = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=dict(k=k, e=e, K=K, E=E_, b=b, hash_seed=4242, evict_seed=3,
                                                                    shuffle_seed=6, mask_seed=7))
    cl = BatchedFHEPSIClient(cc, k, e, K, E_, b, hashSeed=4242)
    cc.load_relin_key(cl.runSetUpPhase())
    minus, idx = cl.runOfflinePhase(clientSet)
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    full = sorted(int(v) for v in cl.extractIntersection(op.getResultList().copy()))
    assert full == sorted(int(v) for v in items[:5])
    op.setChainSchedule(sched)
    op.run()
    rows = op.getResultList().copy()
    assert rows.shape == (b, 2, 3, N)
    got = cl.extractIntersection(rows, limbs=3)
    assert sorted(int(v) for v in got) == full
    ok = level_oracles(ob, o, sched)[3]
    dec = [ok.decrypt_slots(np.ascontiguousarray(cl.sk[:3]), rows[bn], cl.B) for bn in range(b)]
    print("N=%d t=%d K=%d schedule %s: noise budget min %d bits" % (N, t, K, sched, min(d[1] for d in dec)))
    assert min(d[1] for d in dec) >= 1
    cc.close()
