"""The 16-coefficient transforms at ArithKind::fold (csrc/ntt16_kernel.h: butterflies and canonical store reduce by folding with d where
q = 2^60 - d), one launch per child process on the crafted limbs of tests/transform_inputs.py, against the oracle's ntt / intt.

Chain: fold_edge -- every d just under the selection bound 2^27, where a fold adds the most -- with 2 limbs, at the smallest ring each
geometry exists at: N = 8192 (one 2^13 slice per limb, unfolded: the inverse stores canonical coefficients), N = 16384 (two folded
2^13 slices) and N = 32768 (two folded 2^14 slices: four stages in pass 1).  Launches: forward in lane order with and without
lazy_out, on the families and on every representative below 8q; the forward launch with the key-switch digit items riding (their
store is the canonical one: fold, then one conditional subtraction); inverse from standard order and from lane order, on the families
and on every representative below 4q; the tensor launch.

The helpers are those of tests/test_gpu_transform_routes.py (_plain: bit for bit where the output is canonical; congruent and below
8q per word behind lazy_out; below 4q per word and exact after the outer stage and N^-1, in exact integers, behind a folded inverse;
the limb behind the last item untouched) and of tests/test_gpu_lazy_inputs.py (the tensor case).  The program prints the kind that ran
only for the tensor launch; that the plain launches take the fold kind on this chain is the launcher's rule (launch_ntt16: every
modulus of the launch inside NttPlan::fold_mod_count), and tests/test_fold_bfly_listing.py shows that the fold-kind kernels hold the
folding blocks.
"""
import functools

import numpy as np
import pytest

from tests import lazy_inputs as lz
from tests import test_gpu_lazy_inputs as li
from tests import test_gpu_transform_routes as tr

pytestmark = pytest.mark.gpu
CHAIN, L = "fold_edge", 2
RINGS = [8192, 16384, 32768]

# the route and plan tables of tests/test_gpu_transform_routes.py are keyed by chain: this chain decides as the default one does
for _N in RINGS:
    tr.ROUTE.setdefault((CHAIN, _N), tr.ROUTE[("default", _N)])
    tr.PLAN.setdefault((CHAIN, _N), tr.PLAN[("default", _N)])


def _fold(N):
    return li._lane_rule(N)[0]


def test_the_chain_folds_and_sits_at_the_bound():
    for N in RINGS:
        o = tr._ctx(CHAIN, N, L)
        ms = [int(v) for v in o.moduli][:o.M]
        assert len(ms) == 2 * L + 1 and all((1 << 26) < (1 << 60) - m < (1 << 27) for m in ms)


@pytest.mark.parametrize("lazy_out", [0, 1])
@pytest.mark.parametrize("N", RINGS)
def test_forward_lane_order(N, lazy_out):
    tr._plain(CHAIN, N, 0, 1, _fold(N), L=L, lazy_out=lazy_out)


@pytest.mark.parametrize("N", RINGS)
def test_forward_on_every_representative_below_8q(N):
    tr._plain(CHAIN, N, 0, 1, _fold(N), L=L, lazy=8, n=6, lazy_out=1)


@pytest.mark.parametrize("sigma", [0, 1], ids=["std", "lane"])
@pytest.mark.parametrize("N", RINGS)
def test_inverse(N, sigma):
    tr._plain(CHAIN, N, 1, sigma, _fold(N), L=L)


@pytest.mark.parametrize("sigma", [0, 1], ids=["std", "lane"])
@pytest.mark.parametrize("N", RINGS)
def test_inverse_on_every_representative_below_4q(N, sigma):
    tr._plain(CHAIN, N, 1, sigma, _fold(N), L=L, lazy=4, n=6)


@pytest.mark.parametrize("N", RINGS)
def test_digits_ride_on_the_forward_launch(N):
    """nb L L digit items behind the 2 nb L limbs of d0, d1 (lazy_out): the digits leave canonical, through the folded store"""
    fold = _fold(N)
    o = tr._ctx(CHAIN, N, L)
    n = tr.NB * 2 * L
    x, mis, want = tr._crafted(CHAIN, N, L, 0, fold, n, 0, L, 4, 0)
    d2, dig_want = tr._digits(CHAIN, N, L)
    got, plan, _ = li._run("ntt", o, {"data": x, "d2": d2}, {"data": (n, N), "dig": (tr.NB, L, L, N)}, nlimbs=n, nb=tr.NB, sigma=1, fold=fold,
                           digits=1, lazy_out=1)
    assert plan["digits_with_d01"] == 1 and plan["fold_moduli"] == 1 and (plan["kernel"], plan["s0"], plan["global_stages"]) == ("blocked16", fold, 0)
    m = li._lane(o, plan, got)
    tr._check_limbs(o, got["data"], want, mis, 0, 1, fold, 1, "N=%d d0, d1 beside the digits" % N)
    bad = np.argwhere(got["dig"] != dig_want[..., m])
    assert not len(bad), "first of %d: bin %d residue %d into modulus %d, lane position %d" % ((len(bad),) + tuple(bad[0]))


@functools.lru_cache(maxsize=1)
def _tensor_case(N):
    """e[nb][4][M][N] over [0, 8q) in lane order and the COEFFICIENT form of its tensor product, d[nb][3][M][N]"""
    nb = 2
    o = tr._ctx(CHAIN, N, L)
    qs, ps = li._mods(o)
    e = lz.lazy_array(qs + ps, lambda q: 8 * q, (nb, 4), N, np.random.default_rng(N + 3))
    _, sl, kp, T = li._lane_rule(N)
    m = lz.lane_map(N, sl, T, kp)
    t = lz.ref_tensor(e, qs + ps)
    std = np.empty_like(t)
    std[..., m] = t
    d = np.stack([np.stack([np.stack([o.intt(a, std[r, c, a]) for a in range(o.M)]) for c in range(3)]) for r in range(nb)])
    return o, e, d


@pytest.mark.parametrize("N", RINGS)
def test_tensor_launch(N):
    o, e, d = _tensor_case(N)
    M, nb = o.M, e.shape[0]
    qs, ps = li._mods(o)
    got, plan, _ = li._run("ntt16_tensor", o, {"e": e}, {"d": (nb, 3, M, N)}, nb=nb)
    li._check_kind(plan, CHAIN, "fold")
    assert plan["fused_tensor"] == 1 and plan["fold"] == _fold(N)
    li._lane(o, plan, got)
    out = got["d"]
    for r in range(nb):
        for c in range(3):
            for a in range(M):
                q = (qs + ps)[a]
                if plan["fold"]:
                    assert (out[r, c, a] < np.uint64(4 * q)).all(), "row %d component %d limb %d leaves [0, 4q)" % (r, c, a)
                    assert (lz.fold_load(out[r, c, a], *lz.fold_w(o, a)) == d[r, c, a]).all(), "row %d component %d limb %d" % (r, c, a)
                else:
                    assert (out[r, c, a] == d[r, c, a]).all(), "row %d component %d limb %d" % (r, c, a)


def test_nothing_stopped_the_program():
    assert not li._stopped
