"""run() on contexts whose column sums are reduced by folding (q = 2^60 - d, d < 2^27: csrc/stage_a_common.h, colacc_fold) against
o.pie_run, every result row bit for bit, and the selection rule at its edge.

  default chains   N = 16384 (the smallest folded ring) at L = 2 and L = 4, K = 2, b = 2, E = 3, a batch of three queries on two
                   queues; K = 3 once; the same at N = 8192 (lane order without outer-stage folding) and at N = 32768, L = 6.
                   Each context must report the folded kind (PieContext.reduction(): piehip_get_reduction, the plan's decision).
  supplied chains  N = 16384, L = 2, the default chain with its first Q modulus replaced by
                     the smallest prime = 1 (mod 2N) above 2^60 - 2^27 (d just under the bound): the folded kind;
                     the largest such prime below 2^60 - 2^27 (d just over it): the Barrett kind;
                   both found by search on the CPU, both against the oracle.
"""
import numpy as np
import pytest

from tests.param_chains import T32, prime_above, split, uniform
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu
BOUND = 1 << 27   # csrc/kernels.hpp: COLACC_FOLD_MAX_D


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _run(ob, pie, N, L, K, kind, q=None, p=None, nq=3, b=2, E=3):
    o = ob.Oracle(N, L, T32, q, p)
    cc = pie.PieContext(N, L, T32, q, p)
    assert (cc.moduli == o.moduli).all()
    assert cc.reduction() == kind, ([(1 << 60) - int(v) for v in o.moduli[:2 * L + 1]], cc.reduction())
    rng = np.random.default_rng(N + 16 * L + K)
    db, masks = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N)
    keys = [rand_limbs(rng, o.q, (L, 2), N) for _ in range(nq)]
    queries = [(rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)) for _ in range(nq)]
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    cc.load_relin_key(keys[0])
    op.setQueryBatch(nq)
    for i in range(nq):
        cc.load_relin_key(keys[i], query=i)
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus, query=i)
        op.setIndex(idx, query=i)
    cc.set_run_streams(2)
    op.run()
    got = op.getResultList()
    cc.close()
    for i, (idx, minus) in enumerate(queries):
        want = o.pie_run(idx, minus, db, masks, keys[i])
        assert (got[i] == want).all(), (N, L, K, i, np.argwhere(got[i] != want)[:4].tolist())


@pytest.mark.parametrize("N,L,K", [
    (16384, 2, 2),
    (16384, 4, 2),
    (16384, 2, 3),
    (8192, 2, 2),
    (8192, 4, 2),
    (32768, 6, 2),
])
def test_default_chains_fold_and_match_the_oracle(ob, pie, N, L, K):
    _run(ob, pie, N, L, K, "fold")


def _edge_primes(N):
    under = prime_above(N, (1 << 60) - BOUND)[0]
    over = uniform(N, 1, (1 << 60) - BOUND)[0]
    assert 0 < (1 << 60) - under < BOUND <= (1 << 60) - over and over >> 59 == 1
    assert under % (2 * N) == 1 and over % (2 * N) == 1
    return under, over


@pytest.mark.parametrize("side", ["under", "over"])
def test_supplied_modulus_at_the_bound_selects_the_kind(ob, pie, side):
    N, L = 16384, 2
    under, over = _edge_primes(N)
    q, p = split([under if side == "under" else over] + uniform(N, 2 * L), L)
    _run(ob, pie, N, L, 2, "fold" if side == "under" else "barrett", q, p)
