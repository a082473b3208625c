"""The tensor product formed in the load phase of the inverse transform (ntt16_kernel.h, TENSOR instantiation).

Where the 16-coefficient kernel runs a context's lane-ordered transforms (rings of 8192, 16384 and 32768 coefficients) and every
modulus has 60 bits, EvalMult and run() issue one launch for the tensor product and the inverse transform of its result.
Everything is compared against the CPU oracle, bit for bit.  The cases here are the ones the fused load phase adds: operand
residues at their extremes (d1 = a0 b1 + a1 b0 is handed to the inverse butterflies as the unreduced sum of two reduced
products, which has to stay below 4q), row counts that leave the last block of the item dealing (blocks of 24) ragged, and the
profile classes that tell which schedule ran.  No case is skipped: a shape that cannot run fails.
"""
import numpy as np
import pytest

from tests.param_chains import T16, T32, uniform_chain
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu

SHAPES = [(8192, 3, T32), (16384, 4, T32), (32768, 3, T32)]


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _items(N, L, rows):
    """items of the fused launch: rows x 3 result polynomials x M limbs x slices per limb"""
    return rows * 3 * (2 * L + 1) * (2 if N >= 16384 else 1)


def _patterns(rng, q, N):
    """ciphertext rows [4][2][L][N]: all q - 1, all 0, alternating 0 / q - 1, uniform"""
    L = len(q)
    top = np.broadcast_to((q - np.uint64(1))[:, None], (2, L, N)).copy()
    alt = top.copy()
    alt[..., 0::2] = 0
    return np.stack([top, np.zeros_like(top), alt, rand_limbs(rng, q, (2,), N)])


def _check_mult(o, cc, evk, a, b):
    n = a.shape[0]
    assert (cc.EvalMult(a, b, relin=False) == np.stack([o.mul_tensor(a[i], b[i]) for i in range(n)])).all()
    assert (cc.EvalMult(a, b, relin=True) == np.stack([o.mul(a[i], b[i], evk) for i in range(n)])).all()


@pytest.mark.parametrize("N,L,t", SHAPES)
def test_product_cases(ob, pie, N, L, t):
    """each pattern against itself (q - 1 times q - 1) and against its neighbour, with and without relinearisation"""
    o = ob.Oracle(N, L, t)
    cc = pie.PieContext(N, L, t)
    rng = np.random.default_rng(N + 1)
    evk = rand_limbs(rng, o.q, (L, 2), N)
    cc.load_relin_key(evk)
    pat = _patterns(rng, o.q, N)
    for shift in range(2):
        _check_mult(o, cc, evk, pat, np.roll(pat, shift, axis=0))
    cc.close()


@pytest.mark.parametrize("N,L,t", SHAPES)
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_odd_row_counts(ob, pie, N, L, t, rows):
    """the item count is not a multiple of 24: the last items are dealt in natural order"""
    assert _items(N, L, rows) % 24 != 0
    o = ob.Oracle(N, L, t)
    cc = pie.PieContext(N, L, t)
    rng = np.random.default_rng(N + rows)
    evk = rand_limbs(rng, o.q, (L, 2), N)
    cc.load_relin_key(evk)
    pat = _patterns(rng, o.q, N)
    a = np.stack([pat[(i + 3) % 4] for i in range(rows)])
    b = np.stack([pat[(2 * i + 3) % 4] if i % 2 else rand_limbs(rng, o.q, (2,), N) for i in range(rows)])
    _check_mult(o, cc, evk, a, b)
    cc.close()


def _profiled_run(ob, pie, N, L, t, chain_below=None):
    q, p = uniform_chain(N, L, chain_below) if chain_below else (None, None)
    o = ob.Oracle(N, L, t, q, p)
    cc = pie.PieContext(N, L, t, q, p)
    rng = np.random.default_rng(N + L)
    K, E, b = 2, 3, 2
    db, masks, evk = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
    idx, minus = rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    cc.set_run_streams(1)
    cc.set_profiling(True)
    op.run()
    prof = cc.profile()
    cc.set_profiling(False)
    assert (op.getResultList() == o.pie_run(idx, minus, db, masks, evk)).all()
    cc.close()
    return prof


def test_profile_classes_fused(ob, pie):
    """one queue group, one product (K = 2): the two-launch schedule has two inverse launches (the accumulators', the tensor
    result's) and one tensor launch; the fused one has the accumulators' inverse launch and one tensor_ntt_inv launch"""
    prof = _profiled_run(ob, pie, 16384, 2, T32)
    assert prof["tensor_ntt_inv"]["launches"] == 1
    assert "tensor" not in prof
    assert prof["ntt_inv"]["launches"] == 1
    assert prof["tensor_ntt_inv"]["alg_bytes"] == 8.0 * 16384 * 2 * 7 * 5


@pytest.mark.parametrize("N,L,t,below", [(4096, 2, T16, None), (16384, 2, T32, 1 << 50)])
def test_profile_classes_two_launches(ob, pie, N, L, t, below):
    """small rings and chains outside (2^59, 2^60) keep the tensor kernel and the plain inverse transform"""
    prof = _profiled_run(ob, pie, N, L, t, below)
    assert prof["tensor"]["launches"] == 1
    assert "tensor_ntt_inv" not in prof
    assert prof["ntt_inv"]["launches"] == 2
