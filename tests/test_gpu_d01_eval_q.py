"""The relinearising product with the Q limbs of d0 and d1 left in EVALUATION form (NttPlan::d01_eval_q).

Where the plan switches the schedule on (the 16-coefficient lane order with the fused tensor launch: rings of 8192, 16384 and 32768
coefficients, every modulus of 60 bits) the tensor launch transforms 3M - 2L limbs per row instead of 3M, scale-and-round computes
components 0 and 1 from their P limbs alone, and the key-switch MAC adds [t P^-1]_{q_j} (a (x) b)_j, formed from the QP operands.
tests/test_d01_eval_q_identity.py shows on the CPU why that is exact; here everything is compared with the oracle bit for bit.

The cases are the ones the schedule adds:
  * L = 2, 4 and 7 -- at L = 7 column 0 of the MAC's accumulator holds L products, the unnormalised d01 word and the new term;
  * operand residues at their extremes (all q - 1, all 0, alternating), which drive the unreduced sums in the MAC;
  * 1, 3 and 5 rows: the last block of the tensor launch's item dealing (blocks of 24 over the 3 (L + 1) 2^s0 kept triples of a row)
    is ragged at L = 2 and 4 (at L = 7 a row is exactly one or two blocks), and the MAC's two-rows-per-thread pairing has a last
    row without a partner;
  * run() with K = 3 (the path once without and once with the mask), a batch of three queries with their own keys, one query per
    run (X's Q limbs then come from the inverse launch's copy, not from stage A), on one and on two queues;
  * the profile classes that tell which schedule ran, and the key switches that run without a product (rotations).
No case is skipped: a shape that cannot run fails.
"""
import numpy as np
import pytest

from tests.param_chains import T32, uniform_chain
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu

RINGS = [8192, 16384, 32768]
LIMBS = [2, 4, 7]


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _patterns(rng, q, N):
    """ciphertext rows [4][2][L][N]: all q - 1, all 0, alternating 0 / q - 1, uniform"""
    L = len(q)
    top = np.broadcast_to((q - np.uint64(1))[:, None], (2, L, N)).copy()
    alt = top.copy()
    alt[..., 0::2] = 0
    return np.stack([top, np.zeros_like(top), alt, rand_limbs(rng, q, (2,), N)])


def _kept_triples(N, L, rows):
    """items of the tensor launch that are dealt in blocks of 24: rows x 3 x (L + 1) P limbs x slices per limb"""
    return rows * 3 * (L + 1) * (2 if N >= 16384 else 1)


@pytest.mark.parametrize("L", LIMBS)
@pytest.mark.parametrize("N", RINGS)
def test_eval_mult_relin(ob, pie, N, L):
    """EvalMult(relin=True) against o.mul: the extremes against themselves and their neighbours (4 rows), then 1, 3 and 5 rows"""
    o = ob.Oracle(N, L, T32)
    cc = pie.PieContext(N, L, T32)
    rng = np.random.default_rng(N + L)
    evk = rand_limbs(rng, o.q, (L, 2), N)
    cc.load_relin_key(evk)
    pat = _patterns(rng, o.q, N)

    def check(a, b):
        want = np.stack([o.mul(a[i], b[i], evk) for i in range(a.shape[0])])
        assert (cc.EvalMult(a, b, relin=True) == want).all()

    for shift in range(2):
        check(pat, np.roll(pat, shift, axis=0))
    for rows in (1, 3, 5):
        if L != 7:
            assert _kept_triples(N, L, rows) % 24 != 0
        a = np.stack([pat[(i + 3) % 4] for i in range(rows)])
        b = np.stack([pat[(2 * i + 3) % 4] if i % 2 else rand_limbs(rng, o.q, (2,), N) for i in range(rows)])
        check(a, b)
    cc.close()


def _run_case(ob, pie, N, L, K, nq, streams, b=3, E=3, extreme=False, chain_below=None, profile=False):
    """run() of nq queries (their own EvalMult keys when nq > 1) on `streams` queues against o.pie_run; returns the profile"""
    q, p = uniform_chain(N, L, chain_below) if chain_below else (None, None)
    o = ob.Oracle(N, L, T32, q, p)
    cc = pie.PieContext(N, L, T32, q, p)
    rng = np.random.default_rng(N + 16 * L + K + nq)
    db, masks = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N)
    keys = [rand_limbs(rng, o.q, (L, 2), N) for _ in range(nq)]
    queries = [(rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)) for _ in range(nq)]
    if extreme:  # every residue of the first query and of the database at q - 1: the largest accumulators and products
        top = o.q - np.uint64(1)
        queries[0][0][...] = top[:, None]
        queries[0][1][...] = top[:, None]
        db[...] = top[:, None]
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    cc.load_relin_key(keys[0])
    if nq > 1:
        op.setQueryBatch(nq)
        for i in range(nq):
            cc.load_relin_key(keys[i], query=i)
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus, query=i)
        op.setIndex(idx, query=i)
    cc.set_run_streams(streams)
    if profile:
        cc.set_profiling(True)
    op.run()
    prof = cc.profile() if profile else None
    if profile:
        cc.set_profiling(False)
    got = op.getResultList()
    for i, (idx, minus) in enumerate(queries):
        want = o.pie_run(idx, minus, db, masks, keys[i])
        assert ((got if nq == 1 else got[i]) == want).all(), (N, L, K, nq, streams, i)
    cc.close()
    return prof


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("N,L,K,nq", [
    (8192, 2, 3, 1),     # unfolded ring; K = 3: one product without the mask, one with it; X from the inverse launch's copy
    (8192, 4, 2, 3),     # ... a batch of three with their own keys: X from stage A
    (16384, 4, 3, 3),    # the headline ring and chain, K = 3, batch of three
    (16384, 7, 2, 1),    # column headroom, one query
    (16384, 2, 2, 3),
    (32768, 2, 3, 1),    # folded slices of 2^14
    (32768, 7, 2, 3),    # column headroom, batch of three: two rows per thread, the last one alone
    (32768, 4, 2, 1),
])
def test_run(ob, pie, N, L, K, nq, streams):
    _run_case(ob, pie, N, L, K, nq, streams)


@pytest.mark.parametrize("N,L,nq", [(8192, 7, 1), (16384, 7, 3), (32768, 4, 3)])
def test_run_extreme_residues(ob, pie, N, L, nq):
    """database and first query at q - 1 everywhere"""
    _run_case(ob, pie, N, L, 2, nq, 1, extreme=True)


def test_profile_tells_the_schedule(ob, pie):
    """With the schedule on, the key-switch MAC reads the four QP operands at its L limbs: 8N 4L bytes per row more than on a context
    whose plan declines (a chain below 60 bits).  No launch is added: the classes the two contexts share -- the declining chain also
    declines the fused tensor launch and the digit lift in the forward launch, so the transform classes differ between them, as
    tests/test_gpu_fused_tensor.py pins -- have the same launch counts, and the schedule's own counts are those of the fused one."""
    N, L, b = 16384, 2, 2
    on = _run_case(ob, pie, N, L, 2, 1, 1, b=b, profile=True)
    off = _run_case(ob, pie, N, L, 2, 1, 1, b=b, chain_below=1 << 50, profile=True)
    assert on["relin"]["alg_bytes"] - off["relin"]["alg_bytes"] == 8.0 * N * 4 * L * b
    for cls in ("stage_a_mac", "expand", "scale_round", "relin"):
        assert on[cls]["launches"] == off[cls]["launches"] == 1, cls
    assert on["tensor_ntt_inv"]["launches"] == 1 and on["ntt_inv"]["launches"] == 1 and on["ntt_fwd"]["launches"] == 2
    assert "tensor" not in on and "digits" not in on
    assert on["tensor_ntt_inv"]["alg_bytes"] == 8.0 * N * b * 7 * (2 * L + 1)
    assert on["scale_round"]["alg_bytes"] == off["scale_round"]["alg_bytes"]


@pytest.mark.parametrize("N,L", [(8192, 2), (16384, 4), (32768, 7)])
def test_key_switch_without_product(ob, pie, N, L):
    """EvalAutomorphism calls the key switch without a product: no QP operands, results as before"""
    o = ob.Oracle(N, L, T32)
    cc = pie.PieContext(N, L, T32)
    rng = np.random.default_rng(N - L)
    x = rand_limbs(rng, o.q, (2,), N)
    rk = rand_limbs(rng, o.q, (L, 2), N)
    for g in (5, 2 * N - 1):
        assert (cc.EvalAutomorphism(x, g, rk) == o.automorph(x, g, rk)).all()
    cc.close()
