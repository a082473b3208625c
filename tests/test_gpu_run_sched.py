"""The queue and ordering state of a run() (csrc/piehip_ctx.hpp, Sched) where it can go wrong once it is a value handed down and no
longer fields of the handle: two ragged queue groups with results on the device and in host memory (the release of the second
group: recorded in front of the key-switch MAC, behind the whole group when K = 1, in front of the limb-drop kernel when the results
are reduced), a batch's mask and key selection next to an entry point that has neither, and runs that follow each other without a wait.

The smallest ring of the suite (N = 4096, L = 2, E = 2), b = 3 bin layers on two queues (2 + 1).  Bit for bit against the oracle.
"""
import numpy as np
import pytest

from tests.param_chains import T16
from tests.test_gpu_parity import rand_limbs
from tests.test_result_limbs import mod_reduce_exact

pytestmark = pytest.mark.gpu

N, L, E, B = 4096, 2, 2, 3


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


@pytest.fixture(scope="module")
def cases(ob):
    """(K, nq) -> database, masks, the handle's key, one key per query (all different), the queries and the oracle's results
    [nq][b][2][L][N]: computed once per shape, read by every test that uses the shape"""
    o = ob.Oracle(N, L, T16)
    made = {}

    def oracle_results(c, queries):
        return np.stack([o.pie_run(idx, minus, c["db"], c["masks"], c["evks"][i] if len(queries) > 1 else c["evk"])
                         for i, (idx, minus) in enumerate(queries)])

    def get(K, nq):
        if (K, nq) not in made:
            rng = np.random.default_rng(1000 + 10 * K + nq)
            c = {"o": o, "K": K, "nq": nq, "db": rand_limbs(rng, o.q, (K, B, E), N), "masks": rand_limbs(rng, o.q, (B,), N),
                 "evk": rand_limbs(rng, o.q, (L, 2), N), "evks": [rand_limbs(rng, o.q, (L, 2), N) for _ in range(nq)],
                 "queries": [(rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)) for _ in range(nq)],
                 "oracle_results": oracle_results}
            c["want"] = oracle_results(c, c["queries"])
            for a in (c["db"], c["masks"], c["evk"], c["want"]):
                a.setflags(write=False)
            made[K, nq] = c
        return made[K, nq]
    return get


def _operator(pie, c, queues=2):
    """a handle with the case's database on `queues` queues; a batch has a key per query, none of them the handle's"""
    cc = pie.PieContext(N, L, T16)
    assert (cc.q == c["o"].q).all()
    cc.load_relin_key(c["evk"])
    cc.set_run_streams(queues)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=c["db"], preCalcRandomMask=c["masks"])
    if c["nq"] > 1:
        op.setQueryBatch(c["nq"])
        for i, evk in enumerate(c["evks"]):
            cc.load_relin_key(evk, query=i)
    return cc, op


def _set_queries(op, queries):
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus, query=i)
        op.setIndex(idx, query=i)


def _device_results(op):
    """getResultList as [nq][b][2][keep][N]"""
    got = op.getResultList()
    return got[None] if op.nq == 1 else got


def _host_results(op, queries):
    """piehip_run_host of the queries into a zeroed host array, as [nq][b][2][keep][N]"""
    idx, minus = np.stack([q[0] for q in queries]), np.stack([q[1] for q in queries])
    if op.nq == 1:
        return op.runHost(idx[0], minus[0]).copy()[None]
    return op.runHost(idx, minus).transpose(1, 0, 2, 3, 4).copy()


@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_two_ragged_queues(pie, cases, K, nq):
    """groups of 2 and 1 bin layers; results read from the device, then brought down by piehip_run_host (the second group starts
    behind the first group's release, each group downloads its own rows).  K = 1: nobody but run_on_queues records the release"""
    c = cases(K, nq)
    cc, op = _operator(pie, c)
    _set_queries(op, c["queries"])
    op.run()
    assert (_device_results(op) == c["want"]).all()
    assert (_host_results(op, c["queries"]) == c["want"]).all()
    assert (_device_results(op) == c["want"]).all()      # the device list behind the host-results run
    cc.close()


def test_two_ragged_queues_reduced_results(pie, cases):
    """L - 1 result limbs: the chain runs ungated into the full rows, the reduction carries the gate and the release"""
    c = cases(2, 3)
    want = mod_reduce_exact(c["o"], c["want"], L - 1)
    cc, op = _operator(pie, c)
    op.setResultLimbs(L - 1)
    _set_queries(op, c["queries"])
    op.run()
    assert (_device_results(op) == want).all()
    assert (_host_results(op, c["queries"]) == want).all()
    cc.close()


def test_nothing_leaks_between_entry_points(pie, cases):
    """run() of a batch of three with a key per query, then piehip_eval_mult with relinearisation on the same handle, then run()
    again with one query changed: the product takes the handle's key for every row (not key r % 3 of the batch), the second run
    its per-query keys and masks again"""
    c = cases(2, 3)
    o = c["o"]
    cc, op = _operator(pie, c)
    _set_queries(op, c["queries"])
    op.run()
    assert (_device_results(op) == c["want"]).all()
    rng = np.random.default_rng(4242)
    a, b = rand_limbs(rng, o.q, (3, 2), N), rand_limbs(rng, o.q, (3, 2), N)
    assert (cc.EvalMult(a[0], b[0], relin=True) == o.mul(a[0], b[0], c["evk"])).all()                        # two fresh ciphertexts
    assert (cc.EvalMult(a, b, relin=True) == np.stack([o.mul(a[i], b[i], c["evk"]) for i in range(3)])).all()  # ... and three rows of them
    queries = list(c["queries"])
    queries[1] = (rand_limbs(rng, o.q, (2, E, 2), N), rand_limbs(rng, o.q, (2,), N))
    want = c["want"].copy()
    want[1] = o.pie_run(queries[1][0], queries[1][1], c["db"], c["masks"], c["evks"][1])
    assert not (want[1] == c["want"][1]).all()
    _set_queries(op, queries)
    op.run()
    assert (_device_results(op) == want).all()
    cc.close()


def test_back_to_back_runs(pie, cases):
    """three run() calls into the same result buffer, another query in device memory before each, no wait in between: the queues wait
    for the handle's stream and the handle's stream joins them lazily.  One read at the end: the last query's results"""
    import torch
    c = cases(2, 1)
    o = c["o"]
    rng = np.random.default_rng(77)
    queries = [c["queries"][0]] + [(rand_limbs(rng, o.q, (2, E, 2), N), rand_limbs(rng, o.q, (2,), N)) for _ in range(2)]
    queries = [queries[1], queries[2], queries[0]]       # the shared case last: its results are known
    dev = [(torch.from_numpy(idx.view(np.int64)).cuda(), torch.from_numpy(minus.view(np.int64)).cuda()) for idx, minus in queries]
    torch.cuda.synchronize()
    cc, op = _operator(pie, c)
    for d_idx, d_minus in dev:
        op.setMinusCompareElementDevice(d_minus.data_ptr())
        op.setIndexDevice(d_idx.data_ptr())
        op.run(sync=False)
    assert (_device_results(op) == c["want"]).all()
    # ... and behind unchanged inputs, where the queues do not wait for the handle's stream but the result-writing kernels do
    op.setMinusCompareElementDevice(dev[0][1].data_ptr())
    op.setIndexDevice(dev[0][0].data_ptr())
    for _ in range(3):
        op.run(sync=False)
    assert (_device_results(op)[0] == o.pie_run(queries[0][0], queries[0][1], c["db"], c["masks"], c["evk"])).all()
    cc.close()
