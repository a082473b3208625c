"""Query slices ACROSS PROCESSES (include/piehip.h: piehip_rccl_scatter_query, piehip_rccl_exchange_accumulators,
piehip_build_db_sliced, piehip_slice_host_buffers_q; the plan: csrc/exchange_plan.h) on the one GPU of the test box.

  test_slice_ranks        tests/slice_ranks_main.cpp as 1 to 5 processes over the test-only transport of tests/fake_rccl, which each
                          process loads itself from the path it is given: two rounds of scatter, run_slice, exchange, run_chain, gather;
                          the root's gathered list against the oracle's run() of every query, all words equal
  test_refusals           the two collectives without a communicator, on an unsliced handle, with a null handle (no transport needed)
  test_build_db_sliced    three handles built with piehip_build_db_sliced evaluate what piehip_run evaluates on a piehip_build_db
                          handle with the same seeds, word for word; a set that cannot be placed is PIEHIP_EHASH
What this cannot show: RCCL itself, xGMI, bandwidth.  At most five rank processes and this one hold the GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import hashing_cases as hc
from tests import slice_ranks_util as sr
from tests.slice_ranks_util import T16, T32

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, EHASH = -1, -2, -5


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return sr.build_programs(tmp_path_factory.mktemp("slice_ranks"), ["slice_ranks_main"])


@pytest.mark.parametrize("G,root,N,L,K,E,b,nq", [
    (1, 0, 4096, 2, 2, 3, 3, 2),      # own block only
    (2, 0, 4096, 2, 2, 3, 3, 1),      # no lane order; 1 + 2 layers
    (2, 1, 8192, 2, 2, 3, 3, 3),      # X placed lane-ordered; root != 0; one EvalMult key per query
    (3, 1, 8192, 3, 3, 2, 2, 2),      # K = 3; b < G: rank 0 has no chain side
    (4, 2, 16384, 2, 2, 3, 5, 2),     # folded ring; one unit each; blocks of 0.5 and 1 MiB in both directions of a pair, past the
                                      # socket buffer: the case the posting order exists for
    (5, 4, 4096, 2, 2, 3, 14, 1),     # K L < G: rank 0 has no units; the last rank is root
    (3, 0, 4096, 4, 2, 3, 4, 1),      # eight units as 2 + 3 + 3; the middle slice spans two hash functions
])
def test_slice_ranks(ob, built, tmp_path, G, root, N, L, K, E, b, nq):
    fake, exes = built
    t = T16 if N < 8192 else T32
    own_keys = (G, root, N) == (2, 1, 8192)
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(7000 + 100 * G + 10 * b + nq)
    q = o.moduli[:L]
    db, masks = sr.rand_limbs(rng, q, (K, b, E), N), sr.rand_limbs(rng, q, (b,), N)
    keys = [sr.rand_limbs(rng, q, (L, 2), N) for _ in range(nq if own_keys else 1)]
    queries = [(sr.rand_limbs(rng, q, (K, E, 2), N), sr.rand_limbs(rng, q, (2,), N)) for _ in range(nq)]
    db.tofile(tmp_path / "db.bin")
    masks.tofile(tmp_path / "masks.bin")
    for i, key in enumerate(keys):
        key.tofile(tmp_path / ("evk%d.bin" % i))
    for i, (idx, minus) in enumerate(queries):
        idx.tofile(tmp_path / ("idx%d.bin" % i))
        minus.tofile(tmp_path / ("minus%d.bin" % i))
    procs = [subprocess.Popen([exes["slice_ranks_main"], fake] + [str(v) for v in (r, G, root, N, L, t, K, E, b, nq, tmp_path)] +
                              (["keys"] if own_keys else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(G)]
    for r, (rc, so, se) in enumerate(sr.wait_all(procs)):
        assert rc == 0, "rank %d: %s %s" % (r, so, se)
    want = {}
    for rnd in range(2):
        got = np.fromfile(tmp_path / ("out%d.bin" % rnd), dtype=np.uint64).reshape(b, nq, 2, L, N)
        for i in range(nq):
            src, key = (i + rnd) % nq, i if own_keys else 0    # round 1 wrote query (i + 1) % nq into place i; the key stays the place's
            if (src, key) not in want:
                want[src, key] = o.pie_run(queries[src][0], queries[src][1], db, masks, keys[key])
            assert (got[:, i] == want[src, key]).all(), "round %d, query %d of the batch" % (rnd, i)


def test_refusals(pie_mod):
    """before anything is queued, and without a transport: RCCL is never initialised here"""
    from nested_hashing_psi_amd import _lib
    lib = _lib.lib()
    N, L, K, E, b = 4096, 2, 2, 2, 2
    sliced, plain = pie_mod.PieContext(N, L, T16), pie_mod.PieContext(N, L, T16)
    try:
        rng = np.random.default_rng(3)
        pts = sr.rand_limbs(rng, sliced.moduli[:1], (K * L, b, E), N)[..., 0, :].copy()
        masks = sr.rand_limbs(rng, sliced.moduli[:L], (b,), N)
        u64p = C.POINTER(C.c_uint64)
        assert lib.piehip_load_db_sliced(sliced._h, K, b, E, 0, K * L, pts.ctypes.data_as(u64p), 0, b, masks.ctypes.data_as(u64p)) == 0
        for h, what in ((sliced._h, "no communicator"), (plain._h, "an unsliced handle")):
            assert lib.piehip_rccl_exchange_accumulators(h) == ESTATE, what
            assert lib.piehip_rccl_scatter_query(h, 0) == ESTATE, what
        assert b"communicator" in lib.piehip_last_error()
        assert lib.piehip_rccl_exchange_accumulators(None) == EINVAL
        assert lib.piehip_rccl_scatter_query(None, 0) == EINVAL
        # a refused call changes nothing: the handle still evaluates (nothing was marked put, so the chain is refused as ever)
        assert lib.piehip_run_chain(sliced._h) == ESTATE
    finally:
        sliced.close()
        plain.close()


def test_build_db_sliced(ob, pie_mod):
    pie = pie_mod
    N, L, t, k, e, K, E, b, nS = 4096, 2, T16, 2, 40, 2, 6, 5, 300
    rng = np.random.default_rng(11)
    items = hc.distinct(rng, t, nS)
    hp = dict(k=k, e=e, K=K, b=b, E=E, hash_seed=987654321, evict_seed=5, shuffle_seed=6, mask_seed=7)
    ccs = [pie.PieContext(N, L, t) for _ in range(4)]
    try:
        o = ob.Oracle(N, L, t)
        evk = sr.rand_limbs(rng, o.moduli[:L], (L, 2), N)
        for cc in ccs:
            cc.load_relin_key(evk)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs[:3], serverSet=items, hashParams=hp)
        ref = pie.BatchedFHEHIPPIE(ccs[3], serverSet=items, hashParams=hp)
        idx, minus = sr.rand_limbs(rng, o.moduli[:L], (K, E, 2), N), sr.rand_limbs(rng, o.moduli[:L], (2,), N)
        for x in (op, ref):
            x.setMinusCompareElement(minus)
            x.setIndex(idx)
            x.run()
        got, want = op.getResultList(), ref.getResultList()
        assert got.shape == want.shape == (b, 2, L, N)
        assert (got == want).all(), "slices built with piehip_build_db_sliced differ from the database of piehip_build_db"
        # the failure path: one item more than the table has cells
        case = hc.BY_NAME["fails-wave"]
        bad = hc.items_of(case)
        u64p = C.POINTER(C.c_uint64)
        from nested_hashing_psi_amd import _lib
        rc = _lib.lib().piehip_build_db_sliced(ccs[0]._h, bad.ctypes.data_as(u64p), len(bad), case.k, case.e, case.K, case.b, case.E,
                                               987654321, 5, 6, 7, 0, case.K * L, 0, case.b)
        assert rc == EHASH, _lib.lib().piehip_last_error()
        assert b"Cuckoo" in _lib.lib().piehip_last_error()
    finally:
        for cc in ccs:
            cc.close()
