"""Chain limbs on the GPU (include/piehip.h "Chain limbs"): run() with piehip_set_chain_limbs below L on every route of the transform
plan, the fused conversion and its fallback, the shapes the setting composes with, the setting switched off again, the refusals,
and a real client.

Every comparison is bit for bit, on every word, against the exact definition in tests/test_chain_limbs.py (chain_layer_exact; then
mod_reduce_exact on the level oracle where keep < Lc): integer arithmetic only, so every schedule and route gives the same bits.
"""
import concurrent.futures
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T16, T32, chain_by_name, uniform_chain
from tests.test_chain_limbs import chain_layer_exact, level_key, level_oracle
from tests.test_gpu_parity import rand_limbs
from tests.test_result_limbs import mod_reduce_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _contexts(ob, pie, N, L, t, chain=None):
    if chain is None:
        q, p = None, None
    elif isinstance(chain, str):
        q, p = chain_by_name(N, L, chain)
    else:
        q, p = uniform_chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    cc = pie.PieContext(N, L, t, q, p)
    assert (cc.moduli == o.moduli).all()
    return o, cc


def _database(pie, o, cc, rng, K, E, b, nq):
    db, masks = rand_limbs(rng, o.q, (K, b, E), o.N), rand_limbs(rng, o.q, (b,), o.N)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    if nq > 1:
        op.setQueryBatch(nq)
    return op, db, masks


def _keys(o, rng, nq):
    return [rand_limbs(rng, o.q, (o.L, 2), o.N) for _ in range(nq)]


def _load_keys(cc, op, evks):
    if op.nq == 1:
        cc.load_relin_key(evks[0])
    else:
        for i, k in enumerate(evks):
            cc.load_relin_key(k, query=i)


def _queries(o, rng, K, E, nq):
    return [(rand_limbs(rng, o.q, (K, E, 2), o.N), rand_limbs(rng, o.q, (2,), o.N)) for _ in range(nq)]


def _set_queries(op, queries):
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus, query=i)
        op.setIndex(idx, query=i)


def _exact(ob, o, queries, db, masks, evks, Lc, relin_last=True):
    """[nq][b][2 or 3][Lc][N] by the definition, one task per (query, bin layer)"""
    ol = o if Lc == o.L else level_oracle(ob, o, Lc)
    b = db.shape[1]
    jobs = [(i, bn) for i in range(len(queries)) for bn in range(b)]

    def one(job):
        i, bn = job
        return chain_layer_exact(o, ol, queries[i][0], queries[i][1], db, masks, level_key(evks[i], Lc), Lc, bn, relin_last)
    with concurrent.futures.ThreadPoolExecutor(max_workers=12) as pool:
        rows = list(pool.map(one, jobs))
    return np.stack(rows).reshape((len(queries), b) + rows[0].shape)


def _by_query(op, got):
    return got[None] if op.nq == 1 else got


# ---- 1. run() on every route, limb pair and shape ------------------------------------------------------------------------------------
# (N, L, chain, t, b, nq, K, Lcs): one ring per route of ntt_plan_decide, as tests/test_gpu_result_relin.py chooses them.  chain: None
# = the default 60-bit chain, a number = the uniform chain below it, a name = tests/param_chains.py.  Rings of 2^14 and above use
# b <= 2 and nq <= 2 (the Python-integer drop of the definition is the slow part).
RUNS = [
    (2048, 4, None, T16, 3, 1, 2, (3, 2)),              # radix-2 ring: drop kernel, plain conversions
    (2048, 3, 1 << 50, T32, 3, 3, 3, (2,)),             # a chain outside (2^59, 2^60): generic arithmetic, key per query
    (4096, 4, None, T16, 3, 3, 2, (3, 2)),              # ring 2^12, 32-coefficient kernel; key per query
    (4096, 2, None, T16, 3, 1, 3, (1,)),                # L = 2 with Lc = 1, K = 3
    (8192, 4, None, T32, 9, 1, 3, (3,)),                # ring 2^13, 16-coefficient kernel unfolded; one and two queues (b = 9)
    (16384, 4, None, T32, 2, 2, 2, (3, 2)),             # the folded ring 2^14 (C3's): the fused conversion, both pairs built for L = 4
    (16384, 4, None, T32, 2, 1, 3, (3,)),               # ... K = 3: the second product drops Y alone
    (16384, 5, None, T32, 1, 1, 3, (2,)),               # a pair the fused kernel is not built for, on a folded ring: the fallback
    (16384, 3, "one_p_61", T32, 1, 1, 2, (2,)),         # the parent does not fold (a 61-bit P prime), the level does
    (32768, 7, None, T32, 1, 1, 2, (6,)),               # the folded ring 2^15, L = 7 with Lc = 6
    (32768, 3, None, T32, 1, 2, 3, (2,)),               # ... K = 3, a batch
]


@pytest.mark.parametrize("N,L,chain,t,b,nq,K,Lcs", RUNS)
def test_run_with_the_chain_on_fewer_limbs(ob, pie, N, L, chain, t, b, nq, K, Lcs):
    """every word against the definition; one queue and two (piehip_set_run_streams) where b >= 2; a different key per query of a
    batch; then the setting put back to L gives the results of a handle that never had it"""
    E = 2 + (N // 64 + K) % 2
    o, cc = _contexts(ob, pie, N, L, t, chain)
    rng = np.random.default_rng(N + 100 * K + 10 * b + nq + L)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    evks = _keys(o, rng, nq)
    queries = _queries(o, rng, K, E, nq)
    _set_queries(op, queries)
    _load_keys(cc, op, evks)
    assert op.chainLimbs() == L
    op.run()
    never = _by_query(op, op.getResultList()).copy()
    assert never.shape == (nq, b, 2, L, N)
    for Lc in Lcs:
        want = _exact(ob, o, queries, db, masks, evks, Lc)
        op.setChainLimbs(Lc)
        assert op.chainLimbs() == Lc
        for streams in ((1, 2) if b >= 2 else (0,)):
            cc.set_run_streams(streams)
            op.run()
            got = _by_query(op, op.getResultList())
            assert got.shape == (nq, b, 2, Lc, N)
            assert (got == want).all(), "Lc %d queues %d" % (Lc, streams)
    op.setChainLimbs(L)
    op.run()
    assert (_by_query(op, op.getResultList()) == never).all()
    cc.close()


@pytest.mark.parametrize("N,L,Lc,K", [(4096, 3, 2, 2), (16384, 4, 3, 2), (16384, 4, 3, 3)])
def test_degree_two_results_and_result_limbs_at_a_lower_level(ob, pie, N, L, Lc, K):
    """piehip_set_result_relin(0) at a lower level -- K = 2 with NO key loaded -- and keep < Lc in both forms: the result reduction runs
    inside the level context"""
    E, b, nq = 2, 2, 1
    o, cc = _contexts(ob, pie, N, L, T32)
    ol = level_oracle(ob, o, Lc)
    rng = np.random.default_rng(N + K)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    evks = _keys(o, rng, nq)
    queries = _queries(o, rng, K, E, nq)
    _set_queries(op, queries)
    op.setChainLimbs(Lc)
    op.setResultRelin(False)
    if K > 2:
        _load_keys(cc, op, evks)
    want3 = _exact(ob, o, queries, db, masks, evks if K > 2 else [None], Lc, relin_last=False)
    for keep in (L, Lc - 1):
        op.setResultLimbs(keep)
        op.run()
        got = _by_query(op, op.getResultList())
        assert got.shape == (nq, b, 3, min(keep, Lc), N)
        assert (got == (want3 if keep >= Lc else mod_reduce_exact(ol, want3, keep))).all(), "degree 2, keep %d" % keep
    _load_keys(cc, op, evks)
    op.setResultRelin(True)
    want2 = _exact(ob, o, queries, db, masks, evks, Lc)
    for keep in (Lc - 1, Lc):
        op.setResultLimbs(keep)
        op.run()
        got = _by_query(op, op.getResultList())
        assert got.shape == (nq, b, 2, keep, N)
        assert (got == (want2 if keep == Lc else mod_reduce_exact(ol, want2, keep))).all(), "keep %d" % keep
    cc.close()


def test_one_inner_hash_function_is_unchanged(ob, pie):
    N, L, E, b = 4096, 3, 3, 3
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(11)
    op, db, masks = _database(pie, o, cc, rng, 1, E, b, 1)
    queries = _queries(o, rng, 1, E, 1)
    _set_queries(op, queries)
    op.run()
    before = op.getResultList().copy()
    op.setChainLimbs(2)
    assert op.chainLimbs() == 2
    op.run()
    got = op.getResultList()
    assert got.shape == (b, 2, L, N) and (got == before).all()
    cc.close()


@pytest.mark.parametrize("nq", [1, 2])
def test_host_path_and_seeded_queries(ob, pie, nq):
    """piehip_run_host at C3's ring with b = 9 -- two queue groups, the second behind the first group's hand-over -- at Lc = 3 and
    then keep = 1; the page-locked result array follows the settings; one query: the same query seeded (stage A is untouched)"""
    N, L, K, E, b, Lc = 16384, 4, 2, 2, 9, 3
    o, cc = _contexts(ob, pie, N, L, T32)
    ol = level_oracle(ob, o, Lc)
    rng = np.random.default_rng(4200 + nq)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    evks = _keys(o, rng, nq)
    _load_keys(cc, op, evks)
    pre = () if nq == 1 else (nq,)
    by_query = lambda a: a[None] if nq == 1 else a.transpose(1, 0, 2, 3, 4)
    queries = _queries(o, rng, K, E, nq)
    seeds = None
    if nq == 1:     # the c1 halves come from seeds: expand them with the library, as the server would
        seeds = rng.integers(0, 256, (K * E + 1, 32), dtype=np.uint8)
        idx, minus = queries[0]
        a = cc.expand_uniform(seeds)
        idx[:, :, 1] = a[:K * E].reshape(K, E, L, N)
        minus[1] = a[K * E]
    op.setChainLimbs(Lc)
    want = _exact(ob, o, queries, db, masks, evks, Lc)
    idx, minus = np.stack([q[0] for q in queries]), np.stack([q[1] for q in queries])
    if nq == 1:
        idx, minus = idx[0], minus[0]
    for keep in (L, 1):
        op.setResultLimbs(keep)
        w = want if keep >= Lc else mod_reduce_exact(ol, want, keep)
        pr = op.hostBuffers()[2]
        assert pr.shape == (b,) + pre + (2, min(keep, Lc), N)
        got = op.runHost(idx, minus)
        assert got.shape == pr.shape and (by_query(got) == w).all(), "runHost keep %d" % keep
        if seeds is not None:
            got = op.runHostSeeded(np.ascontiguousarray(idx[:, :, 0]), seeds[:K * E].reshape(K, E, 32), np.ascontiguousarray(minus[0]), seeds[K * E])
            assert (by_query(got) == w).all(), "runHostSeeded keep %d" % keep
    cc.close()


def test_query_slot_has_its_own_setting(ob, pie):
    """the owner runs on all limbs, its slot on Lc = 2 with its own copies of the owner's key and masks; then the other way round"""
    N, L, K, E, b, Lc = 4096, 3, 2, 3, 4, 2
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(79)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, 1)
    evks = _keys(o, rng, 1)
    cc.load_relin_key(evks[0])
    cc2 = pie.PieContext(N, L, T16)
    slot = pie.BatchedFHEHIPPIE(cc2, attachTo=op)
    queries = _queries(o, rng, K, E, 1)
    full = _exact(ob, o, queries, db, masks, evks, L)[0]
    low = _exact(ob, o, queries, db, masks, evks, Lc)[0]
    _set_queries(op, queries)
    _set_queries(slot, queries)
    slot.setChainLimbs(Lc)
    assert (op.chainLimbs(), slot.chainLimbs()) == (L, Lc)
    op.run()
    slot.run()
    assert (op.getResultList() == full).all() and (slot.getResultList() == low).all()
    slot.setChainLimbs(L)
    op.setChainLimbs(Lc)
    op.run()
    slot.run()
    assert (op.getResultList() == low).all() and (slot.getResultList() == full).all()
    del slot
    cc2.close()
    cc.close()


def test_the_setting_at_L_changes_nothing(ob, pie):
    """Lc = L on a fresh handle, and a handle whose setting went below L and back, both give the bits of a handle that never set it"""
    N, L, K, E, b, nq = 16384, 4, 2, 2, 2, 2
    o, cc = _contexts(ob, pie, N, L, T32)
    rng = np.random.default_rng(5)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    evks = _keys(o, rng, nq)
    queries = _queries(o, rng, K, E, nq)
    _set_queries(op, queries)
    _load_keys(cc, op, evks)
    op.run()
    never = op.getResultList().copy()
    assert (never == np.stack([o.pie_run(q[0], q[1], db, masks, k) for q, k in zip(queries, evks)])).all()
    op.setChainLimbs(L)
    op.run()
    assert (op.getResultList() == never).all()
    op.setChainLimbs(L - 1)
    op.run()
    assert op.getResultList().shape == (nq, b, 2, L - 1, N)
    op.setChainLimbs(L)
    op.run()
    assert (op.getResultList() == never).all()
    cc.close()


def test_refusals_leave_the_handle_usable(ob, pie):
    from nested_hashing_psi_amd._lib import lib, u64p
    N, L, K, E, b = 4096, 3, 2, 3, 3
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(6)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, 1)
    evks = _keys(o, rng, 1)
    queries = _queries(o, rng, K, E, 1)
    full = _exact(ob, o, queries, db, masks, evks, L)[0]
    low = _exact(ob, o, queries, db, masks, evks, 2)[0]
    _set_queries(op, queries)
    cc.load_relin_key(evks[0])
    n = C.c_uint32()
    assert lib().piehip_set_chain_limbs(None, 2) == pie.EINVAL
    assert lib().piehip_get_chain_limbs(cc._h, None) == pie.EINVAL
    assert lib().piehip_set_chain_limbs(cc._h, 0) == pie.EINVAL
    assert lib().piehip_set_chain_limbs(cc._h, L + 1) == pie.EINVAL
    assert lib().piehip_get_chain_limbs(cc._h, C.byref(n)) == 0 and n.value == L
    # the captured graph and a chain on fewer limbs exclude each other, whichever comes second
    cc.set_graph(True)
    assert lib().piehip_set_chain_limbs(cc._h, 2) == pie.ESTATE
    assert b"graph" in lib().piehip_last_error()
    op.setChainLimbs(L)                         # what the graph runs: accepted
    op.run()
    assert (op.getResultList() == full).all()
    cc.set_graph(False)
    op.setChainLimbs(2)
    assert lib().piehip_set_graph(cc._h, 1) == pie.ESTATE
    assert b"set_chain_limbs" in lib().piehip_last_error()
    op.run()
    assert (op.getResultList() == low).all()
    # the gather of a sharded server refuses the shorter rows, before it looks at its communicator
    p = u64p()
    assert lib().piehip_gather_results_host(cc._h, b, 0, C.byref(p)) == pie.ESTATE
    assert b"piehip_set_chain_limbs" in lib().piehip_last_error()
    assert lib().piehip_gather_results(cc._h, b, 0, C.c_void_p(op.resultsDevicePtr())) == pie.ESTATE
    assert b"piehip_set_chain_limbs" in lib().piehip_last_error()
    op.setChainLimbs(L)
    op.run()
    assert (op.getResultList() == full).all()   # a correct default run() on the same handle afterwards
    cc.close()
    # a query-sliced handle: the setting is refused there, and a handle with the setting refuses a sliced load
    cc = pie.PieContext(N, L, T16)
    sl = pie.QuerySlicedBatchedFHEHIPPIE([cc], vectorizedHCT=db, preCalcRandomMask=masks)
    assert lib().piehip_set_chain_limbs(cc._h, 2) == pie.ESTATE
    assert b"sliced" in lib().piehip_last_error()
    assert lib().piehip_set_chain_limbs(cc._h, L) == 0
    del sl
    cc.close()
    cc = pie.PieContext(N, L, T16)
    assert lib().piehip_set_chain_limbs(cc._h, 2) == 0
    with pytest.raises(RuntimeError, match="piehip_set_chain_limbs"):
        pie.QuerySlicedBatchedFHEHIPPIE([cc], vectorizedHCT=db, preCalcRandomMask=masks)
    cc.close()


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------------
def test_client_reads_rows_of_the_lower_level(ob, pie):
    """a real client at C3's parameters, b = 2: the chain on three limbs, then one result limb, gives exactly the full run's matches"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    N, L, t, Lc = 16384, 4, T32, 3
    k, e, K, E, b = 2, 16, 2, 14, 2
    o, cc = _contexts(ob, pie, N, L, t)
    rng = np.random.default_rng(N + 1)
    items = np.unique(rng.integers(1, 1 << 31, 400, dtype=np.uint64))[:150]
    rng.shuffle(items)
    server, clientSet = items[:140].copy(), np.concatenate([items[:5], items[140:150]])
    op = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=dict(k=k, e=e, K=K, E=E, b=b, hash_seed=4242, evict_seed=3,
                                                                    shuffle_seed=6, mask_seed=7))
    cl = BatchedFHEPSIClient(cc, k, e, K, E, b, hashSeed=4242)
    cc.load_relin_key(cl.runSetUpPhase())
    minus, idx = cl.runOfflinePhase(clientSet)
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    full = sorted(int(v) for v in cl.extractIntersection(op.getResultList().copy()))
    assert full == sorted(int(v) for v in items[:5])
    op.setChainLimbs(Lc)
    for keep in (L, 1):
        op.setResultLimbs(keep)
        op.run()
        rows = op.getResultList().copy()
        limbs = min(keep, Lc)
        assert rows.shape == (b, 2, limbs, N)
        got = cl.extractIntersection(rows, limbs=limbs)
        assert sorted(int(v) for v in got) == full, "Lc = %d, keep = %d" % (Lc, keep)
        ok = level_oracle(ob, o, limbs)
        dec = [ok.decrypt_slots(np.ascontiguousarray(cl.sk[:limbs]), rows[bn], cl.B) for bn in range(b)]
        print("N=%d t=%d chain limbs %d keep %d: noise budget min %d bits" % (N, t, Lc, keep, min(d[1] for d in dec)))
        assert min(d[1] for d in dec) >= 1
    cc.close()
