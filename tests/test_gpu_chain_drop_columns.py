"""The limb drop's three device forms on crafted accumulator columns (tests/coeff_columns.py: drop_families), bit for bit against the
exact definition: limb_drop_kernel through piehip_mod_reduce, and chain_drop_kernel / drop_limbs inside expand_both_drop_kernel
through run() with chain limbs (include/piehip.h "Chain limbs").

Every run() of tests/test_gpu_chain_limbs.py hands these kernels uniform accumulators, which meet the branch of the centred drop --
and the ends of its one-word operand -- with probability about 2^-59 a coefficient; tests/test_chain_drop_columns.py shows on the CPU
that a drop whose threshold is off by one passes 2000 uniform columns and fails the columns used here.  The columns plant the dropped
residue of EVERY step (the derived ones too), kept residues at 0 and q_i - 1 in front of a step, and the level's own digit extremes,
ties and windows behind the drop, on both members of every folded pair (ccol.tile).

run() gets them as in test_run_with_crafted_index (tests/test_gpu_coeff_columns.py): database plaintexts 1, E = 1, minus = 0, so stage
A hands the crafted index ciphertexts themselves to the chain.  The reference is chain_layer_exact (tests/test_chain_limbs.py).  No
tolerance and no skip: a shape that cannot run fails.

The conversions behind the drop exist once per kind of the column-sum reduction, and a level has a kind of its
own: the points on barrett_60, fold_edge, last_q_over and last_p_over (tests/param_chains.py) assert the kinds of parent and level
(REDUCTION) from PieContext.reduction() before they compare a word.
"""
import os

import numpy as np
import pytest

from tests import coeff_columns as ccol
from tests.param_chains import T32
from tests.test_chain_drop_columns import CASES, MOD_REDUCE, case_families, case_id, chain_moduli
from tests.test_gpu_chain_limbs import _by_query, _exact
from tests.test_gpu_parity import rand_limbs
from tests.test_result_limbs import mod_reduce_exact
from tests.test_result_relin import chain_inputs

pytestmark = pytest.mark.gpu

# The one switch of the route assertions: the library as built by default has the fused conversion; a library built with
# -DPIEHIP_CHAIN_DROP_FUSED=0 (the A/B build of DESIGN.md section 4e) has none, and every point marked "fused" below must then show
# the drop kernel's class instead.  Run this file against such a build with PIEHIP_TEST_CHAIN_DROP_FUSED=0.
CHAIN_DROP_FUSED = os.environ.get("PIEHIP_TEST_CHAIN_DROP_FUSED", "1") != "0"

# What enqueue_chain_bins (piehip_run.cpp) makes of each point, written out rather than computed by the library's rule, so that a
# change of the rule shows:
#   fused     expand_both_drop_kernel<L, Lc, XDROP>: the parent and the level fold (N = 16384, 32768), every level modulus in
#             (2^59, 2^60), a pair the kernel is built for.  K = 3 runs both forms: XDROP for the first product, Y alone dropped
#             in the second.  No launch of class limb_drop
#   folded    chain_drop_kernel<true> behind the parent's folded inverse transform (it reads through fold_load), then
#             expand_both_plain_kernel<true>: a folded ring with a pair the fused kernel is not built for, or a chain outside
#             (2^59, 2^60)
#   unfolded  chain_drop_kernel<false>, then expand_both_plain_kernel<false> -- <true> at one_p_61, whose 61-bit P prime keeps the
#             parent from folding while the level, without that prime, folds
# (chain, N, L, Lc): (route, K, b)
ROUTES = {
    (None, 16384, 2, 1): ("fused", 3, 1), (None, 16384, 3, 2): ("fused", 3, 1), (None, 16384, 4, 3): ("fused", 3, 1),
    (None, 16384, 4, 2): ("fused", 3, 1), (None, 16384, 5, 4): ("fused", 3, 1), (None, 16384, 6, 5): ("fused", 3, 1),
    (None, 16384, 7, 6): ("fused", 3, 1),
    (None, 32768, 3, 2): ("fused", 2, 1),
    (None, 16384, 5, 2): ("folded", 3, 1), (None, 16384, 7, 1): ("folded", 2, 1),
    (1 << 50, 16384, 3, 2): ("folded", 2, 1), (1 << 50, 32768, 5, 3): ("folded", 2, 1),
    (None, 2048, 4, 2): ("unfolded", 3, 1), (None, 4096, 4, 3): ("unfolded", 3, 1), (None, 8192, 4, 3): ("unfolded", 2, 1),
    (None, 65536, 3, 2): ("unfolded", 2, 1), (1 << 61, 4096, 3, 2): ("unfolded", 3, 1),
    ("q0_wide", 4096, 3, 2): ("unfolded", 3, 1), ("q0_wide", 4096, 3, 1): ("unfolded", 3, 1),
    ("q_narrow_p_wide", 4096, 3, 2): ("unfolded", 3, 1), ("q_narrow_p_wide", 4096, 3, 1): ("unfolded", 3, 1),
    ("barrett_edges", 4096, 3, 2): ("unfolded", 3, 1), ("barrett_edges", 4096, 3, 1): ("unfolded", 3, 1),
    ("q_last_wide", 4096, 3, 2): ("unfolded", 3, 1), ("q_last_wide", 4096, 3, 1): ("unfolded", 3, 1),
    ("one_p_61", 16384, 3, 2): ("unfolded", 2, 1),
    # the Barrett kind of the column-sum reduction (expand_both_drop_kernel with and without XDROP, a non-adjacent pair,
    # expand_both_plain_kernel<true, 2, true> behind chain_drop_kernel<true>, slices of 2^14), d just under the folded kind's bound,
    # and a Barrett parent whose level folds: the load and the drop under the parent's constants, the conversion under the level's
    ("barrett_60", 16384, 3, 2): ("fused", 3, 1), ("barrett_60", 16384, 4, 2): ("fused", 3, 1), ("barrett_60", 16384, 5, 2): ("folded", 3, 1),
    ("barrett_60", 32768, 3, 2): ("fused", 2, 1),
    ("fold_edge", 16384, 3, 2): ("fused", 3, 1), ("fold_edge", 16384, 5, 2): ("folded", 3, 1),
    ("last_q_over", 16384, 3, 2): ("fused", 3, 1), ("last_p_over", 16384, 3, 2): ("fused", 3, 1),
}
# (parent, level): PieContext.reduction() and reduction(level=Lc) of the points that name a chain by its kind; every default-chain
# point is ("fold", "fold")
REDUCTION = {"barrett_60": ("barrett", "barrett"), "fold_edge": ("fold", "fold"), "last_q_over": ("barrett", "fold"),
             "last_p_over": ("barrett", "fold")}
BATCH_POINT = (None, 16384, 4, 3)     # fused; K = 2, b = 2, a batch of three
DEG2_POINTS = [(None, 16384, 4, 3), (None, 4096, 4, 3)]
assert set(ROUTES) | {BATCH_POINT} | set(DEG2_POINTS) <= set(CASES)   # the CPU file has checked the families of every point


def _drop_launched(route):
    return route != "fused" or not CHAIN_DROP_FUSED


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _context(pie, o, case):
    q, p = chain_moduli(*case[:3])
    cc = pie.PieContext(o.N, o.L, o.t, q, p)
    assert (cc.moduli == o.moduli).all()
    return cc


def _crafted_ct(o, fam, seed):
    """one ciphertext [2][L][N] in EVALUATION form, both components tiled with every column of `fam`, a different seed each"""
    return np.stack([ccol.ntt_q(o, ccol.tile(fam, o.N, np.random.default_rng(seed + c))) for c in range(2)])


def _profiled(cc, fn):
    cc.set_profiling(True)
    out = fn()
    prof = cc.profile()
    cc.set_profiling(False)
    return out, prof


# ---- (a) piehip_mod_reduce: limb_drop_kernel<L, keep> -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=case_id(c)) for c in MOD_REDUCE])
def test_mod_reduce_on_crafted_columns(pie, case):
    """two ciphertexts whose four polynomials hold every column of drop_families(L -> keep): all 21 pairs of the default chain, and
    both keeps of L = 3 on the chains where the drop's offset spans several q_i (q0_wide), some 2^14 of them (q_last_wide), where the
    moduli are outside (2^59, 2^60) and at the edges of the one-word Barrett"""
    o, _, fam = case_families(case)
    keep = case[3]
    x = np.stack([_crafted_ct(o, fam, 1000 * i + 8 * o.L + keep) for i in range(2)])
    want = mod_reduce_exact(o, x, keep)
    cc = _context(pie, o, case)
    got = cc.mod_reduce(x, keep)
    cc.close()
    assert got.shape == (2, 2, keep, o.N)
    bad = np.argwhere(got != want)
    assert not len(bad), "%d words differ, first at ciphertext %d component %d limb %d position %d" % ((len(bad),) + tuple(bad[0]))


# ---- (b) run() with chain limbs ------------------------------------------------------------------------------------------------------
def _setup(ob, pie, case, K, b, nq, relin=True):
    """(o, cc, op, queries, db, masks, evks): database plaintexts 1, E = 1, minus = 0; the crafted query is the only one, or sits in
    slot 1 of a batch of three between two uniform ones"""
    o, _, fam = case_families(case)
    N, L = o.N, o.L
    rng = np.random.default_rng(N + 8 * L + case[3])
    db = np.ones((K, b, 1, L, N), dtype=np.uint64)
    zero = np.zeros((2, L, N), dtype=np.uint64)
    masks, evk = rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
    crafted = np.stack([_crafted_ct(o, fam, 100 * h + L) for h in range(K)]).reshape(K, 1, 2, L, N)
    # stage A hands the index ciphertexts themselves to the chain: asserted from the oracle
    assert all((a == crafted[h, 0]).all() for h, a in enumerate(chain_inputs(o, crafted, zero, db, b - 1)))
    idxs = [crafted] if nq == 1 else [rand_limbs(rng, o.q, (K, 1, 2), N), crafted, rand_limbs(rng, o.q, (K, 1, 2), N)]
    queries = [(idx, zero) for idx in idxs]
    cc = _context(pie, o, case)
    if relin:
        cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    if nq > 1:
        op.setQueryBatch(nq)
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus, query=i)
        op.setIndex(idx, query=i)
    return o, cc, op, queries, db, masks, [evk if relin else None] * nq


def _run(cc, op):
    op.run()
    return _by_query(op, op.getResultList()).copy()


def _check_route(prof, route):
    assert ("limb_drop" in prof) == _drop_launched(route), "route %s, fused build %s: classes %s" % (route, CHAIN_DROP_FUSED, sorted(prof))
    assert "expand" in prof


@pytest.mark.parametrize("case", [pytest.param(c, id="%s-%s-K%d" % (case_id(c), r[0], r[1])) for c, r in ROUTES.items()])
def test_run_drops_crafted_accumulators(ob, pie, case):
    """one query, every word against the definition, on the route ROUTES names; the profiled run gives the same bits and shows the
    drop kernel's class exactly where the route has a drop kernel"""
    route, K, b = ROUTES[case]
    Lc = case[3]
    o, cc, op, queries, db, masks, evks = _setup(ob, pie, case, K, b, 1)
    want = _exact(ob, o, queries, db, masks, evks, Lc)
    with pytest.raises(RuntimeError):
        cc.reduction(level=Lc)                      # a level no schedule has named yet
    op.setChainLimbs(Lc)
    if case[0] is None or case[0] in REDUCTION:
        assert (cc.reduction(), cc.reduction(level=Lc)) == REDUCTION.get(case[0], ("fold", "fold")), "the kinds of parent and level"
        assert cc.reduction(level=o.L) == cc.reduction()
    got = _run(cc, op)
    assert got.shape == (1, b, 2, Lc, o.N)
    assert (got == want).all()
    got, prof = _profiled(cc, lambda: _run(cc, op))
    cc.close()
    assert (got == want).all()
    _check_route(prof, route)


def test_run_drops_crafted_accumulators_in_a_batch(ob, pie):
    """the fused conversion at C3's pair with K = 2, b = 2 and a batch of three, the crafted query in slot 1 between uniform ones, on
    one queue and on two"""
    case, K, b, nq = BATCH_POINT, 2, 2, 3
    Lc = case[3]
    o, cc, op, queries, db, masks, evks = _setup(ob, pie, case, K, b, nq)
    want = _exact(ob, o, queries, db, masks, evks, Lc)
    op.setChainLimbs(Lc)
    for queues in (1, 2):
        cc.set_run_streams(queues)
        got = _run(cc, op)
        assert got.shape == (nq, b, 2, Lc, o.N)
        for i in range(nq):
            assert (got[i] == want[i]).all(), "query %d of the batch, %d queue(s)" % (i, queues)
    cc.set_run_streams(1)
    _, prof = _profiled(cc, lambda: _run(cc, op))
    cc.close()
    _check_route(prof, "fused")


# ---- (c) degree-2 results ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id="%s-%s" % (case_id(c), ROUTES[c][0])) for c in DEG2_POINTS])
def test_degree_two_results_of_crafted_accumulators(ob, pie, case):
    """piehip_set_result_relin(0), K = 2, no key loaded: the dropped crafted X and Y go through the level's conversions and tensor
    product into deg2_finish (the fused point) or the three-component mask multiply (the unfolded one)"""
    route, K, b = ROUTES[case][0], 2, 1
    Lc = case[3]
    o, cc, op, queries, db, masks, evks = _setup(ob, pie, case, K, b, 1, relin=False)
    want = _exact(ob, o, queries, db, masks, evks, Lc, relin_last=False)
    op.setChainLimbs(Lc)
    op.setResultRelin(False)
    got, prof = _profiled(cc, lambda: _run(cc, op))
    cc.close()
    assert got.shape == (1, b, 3, Lc, o.N)
    assert (got == want).all()
    _check_route(prof, route)
