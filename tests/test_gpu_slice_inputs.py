"""The inputs of a query-sliced handle (include/piehip.h "Query slices"; csrc/piehip_slice.cpp, set_piece): the unseeded setters in
their three forms -- a hand-cut slice in host memory (piehip_set_*_slice_q), the whole query in host memory (piehip_set_*_slice_from_q)
and a hand-cut slice in device memory (piehip_set_*_slice_device_q) -- for the index matrix and the minus element.  The seeded forms
are in tests/test_gpu_query_slices_seeded.py.

N = 4096, L = 4, K = 2, E = 3, b = 2, a batch of two, three handles: the eight units split 2 + 3 + 3, the middle handle's range [2, 5)
starts inside inner hash function 0 and ends inside 1.  The two queries of the batch hold different data, and each has device copies
of its own on every handle.  The oracle's results are computed once for the module.  At most six handles per process at a time."""
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T32
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -2
u64p = C.POINTER(C.c_uint64)
N, L, K, E, B, NQ, G, T = 4096, 4, 2, 3, 2, 2, 3, T32


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _lib():
    from nested_hashing_psi_amd import _lib as l
    return l.lib()


def _P(a):
    return a.ctypes.data_as(u64p)


@pytest.fixture(scope="module")
def world(ob):
    """database, masks, key, the two queries of the batch and what the oracle makes of each; nobody writes to any of it"""
    o = ob.Oracle(N, L, T)
    rng = np.random.default_rng(41)
    w = dict(o=o, db=rand_limbs(rng, o.q, (K, B, E), N), masks=rand_limbs(rng, o.q, (B,), N), evk=rand_limbs(rng, o.q, (L, 2), N))
    w["queries"] = [dict(idx=rand_limbs(rng, o.q, (K, E, 2), N), minus=rand_limbs(rng, o.q, (2,), N)) for _ in range(NQ)]
    w["want"] = [o.pie_run(x["idx"], x["minus"], w["db"], w["masks"], w["evk"]) for x in w["queries"]]
    assert not (w["queries"][0]["idx"] == w["queries"][1]["idx"]).all()
    return w


def _operator(pie, w, ccs):
    op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=w["db"], preCalcRandomMask=w["masks"])
    op.setQueryBatch(NQ)
    for cc in ccs:
        cc.load_relin_key(w["evk"])
    assert [tuple(u) for u in op.unitSlices] == [(0, 2), (2, 5), (5, 8)]
    return op


def _cut(x, ul, uh):
    """the units [ul, uh) of a query by the definition: limb u % L of inner hash function u // L -- [u_n][E][2][N], [u_n][2][N]"""
    si = np.ascontiguousarray(np.stack([x["idx"][u // L, :, :, u % L] for u in range(ul, uh)]))
    sm = np.ascontiguousarray(np.stack([x["minus"][:, u % L] for u in range(ul, uh)]))
    assert si.shape == (uh - ul, E, 2, N) and sm.shape == (uh - ul, 2, N)
    return si, sm


def _run(op):
    op.run()
    return [op.sliceAccumulators(g).copy() for g in range(G)], op.getResultList().copy()


def test_unseeded_slice_form_equals_whole_query_form(pie, world):
    """piehip_set_index_slice_q / piehip_set_minus_slice_q fed with hand-cut slices on fresh handles, the facade's setIndex /
    setMinusCompareElement (piehip_set_*_slice_from_q) on other fresh handles: every handle's accumulators are the same words, the
    result lists are the same words, and each query's results are the oracle's."""
    lib = _lib()
    ccs = [pie.PieContext(N, L, T) for _ in range(2 * G)]
    try:
        assert (ccs[0].q == world["o"].q).all()
        cut, whole = _operator(pie, world, ccs[:G]), _operator(pie, world, ccs[G:])
        for i, x in enumerate(world["queries"]):
            for g, (ul, uh) in enumerate(cut.unitSlices):
                si, sm = _cut(x, ul, uh)
                assert lib.piehip_set_index_slice_q(cut.ccs[g]._h, i, _P(si)) == 0
                assert lib.piehip_set_minus_slice_q(cut.ccs[g]._h, i, _P(sm)) == 0
            whole.setIndex(x["idx"], query=i)
            whole.setMinusCompareElement(x["minus"], query=i)
        a, b = _run(cut), _run(whole)
        for g in range(G):
            assert a[0][g].shape == (B, NQ, cut.unitSlices[g][1] - cut.unitSlices[g][0], 2, N)
            assert (a[0][g] == b[0][g]).all(), "accumulators of handle %d differ" % g
        assert a[1].shape == b[1].shape == (NQ, B, 2, L, N) and (a[1] == b[1]).all()
        for i in range(NQ):
            assert (a[1][i] == world["want"][i]).all(), i
    finally:
        for cc in ccs:
            cc.close()


def test_refusals_of_the_unseeded_setters(ob, pie):
    """the six unseeded setters (slice, whole-query and device form; index and minus): null input and q >= nq give PIEHIP_EINVAL, a
    handle that is not query-sliced PIEHIP_ESTATE, a null handle PIEHIP_EINVAL, each with a message.  A handle without units returns
    PIEHIP_OK.  Nothing of a refused call reaches the handle: the round completes afterwards with the inputs set before."""
    import torch
    N, L, K, E, b, t = 4096, 2, 2, 2, 2, T32
    lib = _lib()
    o = ob.Oracle(N, L, t)
    ccs = [pie.PieContext(N, L, t) for _ in range(2)]
    plain = pie.PieContext(N, L, t)

    def refused(rc, code):
        assert rc == code and lib.piehip_last_error().decode()

    try:
        rng = np.random.default_rng(42)
        db, masks, evk = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=db, preCalcRandomMask=masks, unitSlices=[(0, 4), (4, 4)])
        for cc in ccs:
            cc.load_relin_key(evk)
        idx, minus = rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)
        op.setIndex(idx)
        op.setMinusCompareElement(minus)
        # junk of every form, each large enough for handle 0's four units should a call go through
        ji, jm = rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)
        si = np.ascontiguousarray(np.stack([ji[u // L, :, :, u % L] for u in range(4)]))
        sm = np.ascontiguousarray(np.stack([jm[:, u % L] for u in range(4)]))
        di, dm = torch.from_numpy(si.view(np.int64)).cuda(), torch.from_numpy(sm.view(np.int64)).cuda()
        torch.cuda.synchronize()
        setters = [(lib.piehip_set_index_slice_q, _P(si)), (lib.piehip_set_minus_slice_q, _P(sm)),
                   (lib.piehip_set_index_slice_from_q, _P(ji)), (lib.piehip_set_minus_slice_from_q, _P(jm)),
                   (lib.piehip_set_index_slice_device_q, C.c_void_p(di.data_ptr())),
                   (lib.piehip_set_minus_slice_device_q, C.c_void_p(dm.data_ptr()))]
        h0, h1 = ccs[0]._h, ccs[1]._h
        for h in (h0, h1):    # a handle with units and one without: the arguments are checked on both
            for f, p in setters:
                refused(f(h, 0, None), EINVAL)
                refused(f(h, 1, p), EINVAL)
        for f, p in setters:
            refused(f(plain._h, 0, p), ESTATE)
            refused(f(None, 0, p), EINVAL)
            assert f(h1, 0, p) == 0          # no units: PIEHIP_OK
        op.run()
        assert (op.getResultList() == o.pie_run(idx, minus, db, masks, evk)).all()
    finally:
        for cc in ccs + [plain]:
            cc.close()


def test_shrinking_the_batch_forgets_caller_owned_slices(pie, world):
    """device arrays for queries 0 and 1, then a batch of one, then a batch of two again: query 1's pointers are forgotten (the rule
    of piehip_set_query_batch; the caller may have freed them), so piehip_run_slice refuses with PIEHIP_ESTATE until query 1 is set
    again.  Query 0 keeps its arrays.  Then the round runs and gives the oracle's results."""
    import torch
    lib = _lib()
    ccs = [pie.PieContext(N, L, T) for _ in range(G)]
    try:
        op = _operator(pie, world, ccs)
        dev = [[[torch.from_numpy(a.view(np.int64)).cuda() for a in _cut(x, ul, uh)] for ul, uh in op.unitSlices] for x in world["queries"]]
        torch.cuda.synchronize()

        def set_device(i):
            for g, cc in enumerate(ccs):
                assert lib.piehip_set_index_slice_device_q(cc._h, i, C.c_void_p(dev[i][g][0].data_ptr())) == 0
                assert lib.piehip_set_minus_slice_device_q(cc._h, i, C.c_void_p(dev[i][g][1].data_ptr())) == 0

        set_device(0)
        set_device(1)
        op.setQueryBatch(1)
        op.setQueryBatch(NQ)
        for cc in ccs:
            assert lib.piehip_run_slice(cc._h) == ESTATE and lib.piehip_last_error().decode()
        set_device(1)
        got = _run(op)[1]
        for i in range(NQ):
            assert (got[i] == world["want"][i]).all(), i
    finally:
        for cc in ccs:
            cc.close()
