"""Result relinearisation on the GPU (include/piehip.h "Result relinearisation"): run() with piehip_set_result_relin(0) on every
route of the transform plan, the host-memory path, K = 1, the refusals, and a real client decrypting three-component rows.

Every comparison is bit for bit, on every word, against the exact definition in tests/test_result_relin.py (layer_rows /
run_deg2_exact; then mod_reduce_exact where keep < L): integer arithmetic only, so every schedule and route gives the same bits.
"""
import concurrent.futures
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T16, T32, uniform_chain
from tests.test_gpu_parity import rand_limbs
from tests.test_result_limbs import mod_reduce_exact, reduced_oracle
from tests.test_result_relin import layer_rows, mask_mul_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _contexts(ob, pie, N, L, t, below=None):
    q, p = (None, None) if below is None else uniform_chain(N, L, below)
    o = ob.Oracle(N, L, t, q, p)
    cc = pie.PieContext(N, L, t, q, p)
    assert (cc.moduli == o.moduli).all()
    return o, cc


def _database(pie, o, cc, rng, K, E, b, nq):
    """random limbs everywhere; NO key loaded; a batch of nq"""
    db, masks = rand_limbs(rng, o.q, (K, b, E), o.N), rand_limbs(rng, o.q, (b,), o.N)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    if nq > 1:
        op.setQueryBatch(nq)
    return op, db, masks


def _keys(o, rng, nq):
    return [rand_limbs(rng, o.q, (o.L, 2), o.N) for _ in range(nq)]


def _load_keys(cc, op, evks):
    """a different key per query of a batch (piehip_load_relin_key_q); one query: the handle's key"""
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


def _exact(o, queries, db, masks, evks, reference=True):
    """([nq][b][3][L][N], [nq][b][2][L][N] or None): the three-component rows by the definition and the reference's rows, one task
    per (bin layer, query)"""
    b = db.shape[1]
    jobs = [(i, bn) for i in range(len(queries)) for bn in range(b)]

    def one(job):
        i, bn = job
        return layer_rows(o, queries[i][0], queries[i][1], db, masks, evks[i], bn, reference=reference, mask=mask_mul_oracle)
    with concurrent.futures.ThreadPoolExecutor(max_workers=12) as pool:
        rows = list(pool.map(one, jobs))
    shape = (len(queries), b)
    deg2 = np.stack([r[0] for r in rows]).reshape(shape + (3, o.L, o.N))
    ref = np.stack([r[1] for r in rows]).reshape(shape + (2, o.L, o.N)) if reference else None
    return deg2, ref


def _by_query(op, got):
    return got[None] if op.nq == 1 else got


def _reduced(o, rows, keep):
    return rows if keep == o.L else mod_reduce_exact(o, rows, keep)


# ---- 1. run() on every route ---------------------------------------------------------------------------------------------------------
# (N, L, chain bound, t, b, nq, K, keeps): one ring per route of ntt_plan_decide; E in {2, 3} (stage A is unchanged)
RUNS = [
    (64, 2, None, T16, 3, 1, 2, "L"),                 # radix-2, fallback
    (2048, 3, 1 << 50, T32, 3, 2, 2, "L"),            # fallback, generic arithmetic
    (2048, 3, 1 << 50, T32, 3, 2, 3, "L"),
    (4096, 4, None, T16, 3, 3, 2, "L"),               # 32-coefficient kernel, fallback
    (8192, 3, None, T32, 1, 1, 2, "all"),             # 16-coefficient kernel unfolded, fused
    (8192, 3, None, T32, 1, 1, 3, "all"),
    (8192, 3, None, T32, 9, 3, 2, "all"),
    (8192, 3, None, T32, 9, 3, 3, "all"),
    (16384, 4, None, T32, 3, 1, 2, "all"),            # folded 2^13 slices, fused (C3's ring)
    (16384, 4, None, T32, 3, 1, 3, "all"),
    (16384, 4, None, T32, 9, 3, 2, "all"),            # two queues, shares 5 + 4, 27 rows
    (16384, 4, None, T32, 9, 3, 3, "all"),
    (16384, 4, 1 << 61, T32, 3, 3, 2, "L"),           # C3's ring on a 61-bit chain: fallback
    (32768, 6, None, T32, 3, 3, 3, "all"),            # folded 2^14 slices, fused (C5's ring)
    (65536, 2, None, T32, 2, 1, 2, "L"),              # ring 2^16, fallback
]


@pytest.mark.parametrize("N,L,below,t,b,nq,K,keeps", RUNS)
def test_run_without_the_last_relinearisation(ob, pie, N, L, below, t, b, nq, K, keeps):
    """K = 2 runs with NO key loaded; K = 3 with a different key per query; one queue and two where b >= 8; keep in {1, L - 1, L}
    on the fused rings; off -> on -> off on one handle; two run()s back to back without a sync"""
    import torch
    E = 2 + (N // 64 + K) % 2
    o, cc = _contexts(ob, pie, N, L, t, below)
    rng = np.random.default_rng(N + 100 * K + 10 * b + nq)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    evks = _keys(o, rng, nq)
    queries = _queries(o, rng, K, E, nq)
    deg2, ref = _exact(o, queries, db, masks, evks)
    _set_queries(op, queries)
    assert op.resultRelin and op.resultComponents() == 2
    op.setResultRelin(False)
    assert not op.resultRelin and op.resultComponents() == 3
    if K > 2:
        with pytest.raises(RuntimeError, match="relinearisation key"):
            op.run()
        _load_keys(cc, op, evks)
    first = None
    want = {keep: _reduced(o, deg2, keep) for keep in (sorted({1, L - 1, L}) if keeps == "all" else (L,))}
    for streams in ((1, 2) if b >= 8 else (0,)):
        cc.set_run_streams(streams)
        for keep in want:
            op.setResultLimbs(keep)
            op.run()          # K = 2: no EvalMult key on the handle
            got = _by_query(op, op.getResultList())
            assert got.shape == (nq, b, 3, keep, N)
            assert (got == want[keep]).all(), "queues %d keep %d" % (streams, keep)
        first = got.copy()
    # switching on one handle, with a key loaded: on is the reference's run(), the second off equals the first
    _load_keys(cc, op, evks)
    op.setResultRelin(True)
    assert op.resultComponents() == 2
    op.run()
    assert (_by_query(op, op.getResultList()) == ref).all()
    op.setResultRelin(False)
    op.run()
    assert (_by_query(op, op.getResultList()) == first).all()
    # two run()s back to back, no sync in between, into two buffers of the caller's
    words = b * nq * 3 * L * N
    bufs = [torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(2)]
    for d in bufs:
        op.run(sync=False, into=d.data_ptr())
    op.sync()
    for d in bufs:
        got = d.cpu().numpy().view(np.uint64).reshape((b, 3, L, N) if nq == 1 else (b, nq, 3, L, N))
        got = got[None] if nq == 1 else got.transpose(1, 0, 2, 3, 4)
        assert (got == first).all()
    cc.close()


# ---- 2. the host-memory path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 3])
def test_host_path_with_three_component_rows(ob, pie, nq):
    """runHost and the staged path (stageIndexCiphertext .. runStaged) at C3's ring with b = 9 -- two queue groups, the second behind
    the first group's hand-over, each group's download behind its result-writing kernel -- at keep = L and keep = 1, no key loaded"""
    N, L, K, E, b = 16384, 4, 2, 2, 9
    o, cc = _contexts(ob, pie, N, L, T32)
    rng = np.random.default_rng(4100 + nq)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, nq)
    op.setResultRelin(False)
    pre = () if nq == 1 else (nq,)
    by_query = lambda a: a[None] if nq == 1 else a.transpose(1, 0, 2, 3, 4)     # [b][nq] rows -> [nq][b]
    queries = _queries(o, rng, K, E, nq)
    deg2, _ = _exact(o, queries, db, masks, [None] * nq, reference=False)
    idx, minus = np.stack([q[0] for q in queries]), np.stack([q[1] for q in queries])
    if nq == 1:
        idx, minus = idx[0], minus[0]
    for keep in (L, 1):
        op.setResultLimbs(keep)
        want = _reduced(o, deg2, keep)
        pr = op.hostBuffers()[2]
        assert pr.shape == (b,) + pre + (3, keep, N)
        got = op.runHost(idx, minus)
        assert got.shape == pr.shape and (by_query(got) == want).all(), "runHost keep %d" % keep
        for i, (qi, qm) in enumerate(queries):
            op.stageMinus(qm, query=i)
            for h in range(K):
                for j in range(E):
                    op.stageIndexCiphertext(h, j, np.ascontiguousarray(qi[h, j]), query=i)
        pr[...] = 0
        op.runStaged(pr)
        op.waitHost()
        assert (by_query(pr) == want).all(), "runStaged keep %d" % keep
        assert (_by_query(op, op.getResultList()) == want).all()
    cc.close()


# ---- 3. K = 1, the query slot's own setting, refusals --------------------------------------------------------------------------------
def test_one_inner_hash_function_keeps_two_components(ob, pie):
    N, L, E, b = 4096, 3, 3, 3
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(11)
    op, db, masks = _database(pie, o, cc, rng, 1, E, b, 1)
    queries = _queries(o, rng, 1, E, 1)
    _set_queries(op, queries)
    op.run()
    before = op.getResultList().copy()
    assert (before == o.pie_run(queries[0][0], queries[0][1], db, masks, rand_limbs(rng, o.q, (L, 2), N))).all()
    op.setResultRelin(False)
    assert not op.resultRelin and op.resultComponents() == 2
    op.run()
    got = op.getResultList()
    assert got.shape == (b, 2, L, N) and (got == before).all()
    cc.close()


def test_query_slot_has_its_own_setting(ob, pie):
    """a keyless owner (K = 2, relinearisation off) lends its database; the slot starts with the default and is refused for want of a
    key until it is switched off too; the owner, switched back on, is refused in turn and relinearises once it has a key"""
    N, L, K, E, b = 4096, 3, 2, 3, 4
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(78)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, 1)
    cc2 = pie.PieContext(N, L, T16)
    with pytest.raises(RuntimeError, match="no key"):
        pie.BatchedFHEHIPPIE(cc2, attachTo=op)
    op.setResultRelin(False)
    slot = pie.BatchedFHEHIPPIE(cc2, attachTo=op)
    assert (op.resultComponents(), slot.resultComponents()) == (3, 2)
    evks = _keys(o, rng, 1)
    queries = _queries(o, rng, K, E, 1)
    deg2, ref = _exact(o, queries, db, masks, evks)
    _set_queries(op, queries)
    _set_queries(slot, queries)
    with pytest.raises(RuntimeError, match="relinearisation key"):
        slot.run()
    slot.setResultRelin(False)
    op.setResultRelin(True)
    assert (op.resultComponents(), slot.resultComponents()) == (2, 3)
    with pytest.raises(RuntimeError, match="relinearisation key"):
        op.run()
    slot.run()
    assert (slot.getResultList() == deg2[0]).all()
    del slot
    cc2.close()
    cc.load_relin_key(evks[0])
    op.run()
    assert (op.getResultList() == ref[0]).all()
    cc.close()


def test_refusals_leave_the_handle_usable(ob, pie):
    from nested_hashing_psi_amd._lib import lib, u64p
    N, L, K, E, b = 4096, 3, 2, 3, 3
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(6)
    op, db, masks = _database(pie, o, cc, rng, K, E, b, 1)
    evks = _keys(o, rng, 1)
    queries = _queries(o, rng, K, E, 1)
    deg2, ref = _exact(o, queries, db, masks, evks)
    _set_queries(op, queries)
    # today's refusal stays the default's: K = 2 without a key
    with pytest.raises(RuntimeError, match="relinearisation key"):
        op.run()
    assert lib().piehip_set_result_relin(None, 0) == pie.EINVAL
    assert lib().piehip_get_result_relin(cc._h, None) == pie.EINVAL
    assert lib().piehip_get_result_components(cc._h, None) == pie.EINVAL
    assert lib().piehip_client_decrypt_deg2(cc._h, None, None, 1, 2, None) == pie.EINVAL
    # the captured graph and unrelinearised results exclude each other, whichever comes second
    cc.load_relin_key(evks[0])
    cc.set_graph(True)
    assert lib().piehip_set_result_relin(cc._h, 0) == pie.ESTATE
    assert b"graph" in lib().piehip_last_error()
    assert op.resultRelin
    op.setResultRelin(True)                    # what the graph hands out: accepted
    op.run()
    assert (op.getResultList() == ref[0]).all()
    cc.set_graph(False)
    op.setResultRelin(False)
    assert lib().piehip_set_graph(cc._h, 1) == pie.ESTATE
    assert b"set_result_relin" in lib().piehip_last_error()
    op.run()
    assert (op.getResultList() == deg2[0]).all()
    # the gather of a sharded server refuses three-component rows, before it looks at its communicator
    p = u64p()
    assert lib().piehip_gather_results_host(cc._h, b, 0, C.byref(p)) == pie.ESTATE
    assert b"piehip_set_result_relin" in lib().piehip_last_error()
    assert lib().piehip_gather_results(cc._h, b, 0, C.c_void_p(op.resultsDevicePtr())) == pie.ESTATE
    assert b"piehip_set_result_relin" in lib().piehip_last_error()
    op.run()
    assert (op.getResultList() == deg2[0]).all()
    cc.close()
    # a query-sliced handle: the setting is refused there, and a handle with the setting refuses a sliced load
    cc = pie.PieContext(N, L, T16)
    sl = pie.QuerySlicedBatchedFHEHIPPIE([cc], vectorizedHCT=db, preCalcRandomMask=masks)
    assert lib().piehip_set_result_relin(cc._h, 0) == pie.ESTATE
    assert b"sliced" in lib().piehip_last_error()
    del sl
    cc.close()
    cc = pie.PieContext(N, L, T16)
    assert lib().piehip_set_result_relin(cc._h, 0) == 0
    with pytest.raises(RuntimeError, match="piehip_set_result_relin"):
        pie.QuerySlicedBatchedFHEHIPPIE([cc], vectorizedHCT=db, preCalcRandomMask=masks)
    cc.close()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,t", [(4096, 3, T16), (16384, 4, T32)])
def test_client_reads_three_component_rows(ob, pie, N, L, t):
    """a real client against a server that holds NO EvalMult key: exact intersection from three-component rows at keep = L and
    keep = 1, budgets positive, piehip_client_decrypt_deg2 equal to the oracle's decryption of the same rows word for word"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    k, e, K, E, b = 2, 16, 2, 5, 4
    o, cc = _contexts(ob, pie, N, L, t)
    rng = np.random.default_rng(N)
    items = np.unique(rng.integers(1, min(t, 1 << 31), 400, dtype=np.uint64))[:150]
    rng.shuffle(items)
    server, clientSet = items[:140].copy(), np.concatenate([items[:5], items[140:150]])
    op = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=dict(k=k, e=e, K=K, E=E, b=b, hash_seed=4242, evict_seed=3,
                                                                    shuffle_seed=6, mask_seed=7))
    op.setResultRelin(False)
    cl = BatchedFHEPSIClient(cc, k, e, K, E, b, hashSeed=4242)
    cl.runSetUpPhase()               # (the EvalMult key it makes stays with the client)
    minus, idx = cl.runOfflinePhase(clientSet)
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    for keep in (L, 1):
        op.setResultLimbs(keep)
        op.run()
        rows = op.getResultList().copy()
        assert rows.shape == (b, 3, keep, N)
        got = cl.extractIntersection(rows, limbs=keep)
        assert sorted(int(v) for v in got) == sorted(int(v) for v in items[:5]), "keep = %d" % keep
        ok = o if keep == L else reduced_oracle(ob, o, keep)
        sk = np.ascontiguousarray(cl.sk[:keep])
        dec = [ok.decrypt_slots(sk, rows[bn], cl.B) for bn in range(b)]
        print("N=%d t=%d keep=%d: noise budget of the three-component rows min %d bits" % (N, t, keep, min(d[1] for d in dec)))
        assert min(d[1] for d in dec) >= 1
        assert (cl.batchedDecryptedResult == np.stack([d[0] for d in dec])).all()
    cc.close()
