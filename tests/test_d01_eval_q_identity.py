"""Why the relinearising product may leave the Q limbs of d0 and d1 in EVALUATION form (NttPlan::d01_eval_q).

Scale-and-round by t/P (po_scale_round_tp) computes, for output limb k of a polynomial d over QP in COEFFICIENT form,

    out_k = d_k [t P^-1]_{q_k}  +  sum_j yp_j tQF[j][k]  +  itot        (mod q_k)

where yp_j, itot and the rounding depend on the L + 1 P limbs of d only.  The Q limb d_k enters as a product with one constant,
coefficient by coefficient, in its own limb -- and the negacyclic transform of limb k is linear over Z_{q_k}.  d0 and d1 of a
relinearising product go from scale-and-round straight into a forward transform, so

    NTT_k(out_k) = c_k d_k^(eval) + NTT_k(scale_round(d with its Q limbs zeroed)_k),       c_k = [t P^-1]_{q_k}

with d_k^(eval) the tensor product as it is before its inverse transform.  Both sides are canonical residues: equal word for word.
This is checked here on the CPU oracle alone, for every limb count and for chains of mixed widths.
"""
import numpy as np
import pytest

from tests.param_chains import NAMED, T16, T32, named_chain
from tests.test_gpu_parity import rand_limbs


def _mulmod_const(v, c, q):
    """(v * c) mod q, element-wise, exact (Python integers)"""
    return np.array([(int(x) * c) % q for x in v], dtype=np.uint64)


def _check_identity(o, seed):
    N, L, M = o.N, o.L, o.M
    rng = np.random.default_rng(seed)
    mods = o.moduli[:M]
    d_eval = rand_limbs(rng, mods, (), N)                       # [M][N], EVALUATION form over QP
    d_coef = np.stack([o.intt(a, d_eval[a]) for a in range(M)])
    # today's path: every limb inverse-transformed, scale-and-round, forward transform
    out = o.scale_round_tp(d_coef)
    want = np.stack([o.ntt(k, out[k]) for k in range(L)])
    # the schedule's path: the Q limbs never leave EVALUATION form
    d_ponly = d_coef.copy()
    d_ponly[:L] = 0
    out_p = o.scale_round_tp(d_ponly)
    P = 1
    for p in o.p:
        P *= int(p)
    for k in range(L):
        q = int(o.q[k])
        c = (o.t % q) * pow(P % q, -1, q) % q
        got = (o.ntt(k, out_p[k]).astype(object) + _mulmod_const(d_eval[k], c, q).astype(object)) % q
        assert (got.astype(np.uint64) == want[k]).all(), (N, L, k)


@pytest.mark.parametrize("L", [2, 3, 4, 5, 6, 7])
def test_identity_every_limb_count(ob, L):
    N = {2: 4096, 3: 8192, 4: 16384}.get(L, 4096)
    _check_identity(ob.Oracle(N, L, T32), 100 + L)


@pytest.mark.parametrize("name", NAMED)
def test_identity_mixed_width_chains(ob, name):
    """the identity does not depend on the widths of the moduli (the GPU schedule does: it wants 60-bit chains)"""
    N, L = 4096, 3
    q, p = named_chain(N, L, name)
    _check_identity(ob.Oracle(N, L, T16, q, p), 200 + len(name))
