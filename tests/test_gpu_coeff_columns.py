"""The base conversions and the digit lifts on crafted COEFFICIENT-form columns (tests/coeff_columns.py), bit for bit against the oracle.

The other GPU tests hand the product chain EVALUATION rows that are uniform or constant; after the inverse transform the conversion
kernels then see uniform columns, or one coefficient and N - 1 zeros.  Here every operand is the oracle's forward transform of a
polynomial whose columns are digit extremes, rounding ties and digit-lift windows, placed on both members of every folded pair
(n, n + N/2) and on n = 0, 1, N/2 - 1, N/2, N - 1.  tests/test_coeff_columns.py shows on the CPU that these columns are where claimed
and that the tie columns sit where the oracle's fixed-point rounding departs from exact rounding.

The points are the smallest shapes that own each route of ntt_plan_decide (kernels_ntt.hip); ROUTES lists, per point, what the plan
decides there, and the tests assert from cc.profile() the classes that tell the routes apart.  REDUCTION lists, per point, the kind
of the column-sum reduction its context selects; every context is asked for it before it computes, so each
point says which of the two instantiations of the conversions, scale-and-round and the fused tensor product it holds.  No tolerance
and no skip: a shape that cannot run fails.
"""
import functools

import numpy as np
import pytest

from tests import coeff_columns as ccol
from tests import param_chains as pc
from tests.param_chains import T32, T48
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu

# (chain, N, L): None is the default chain, an int the uniform chain below it, a string a chain of param_chains.chain_by_name
# barrett_60 and fold_edge: the fused rings under the Barrett kind of the column-sum reduction and under the folded kind with d just
# below its bound -- 8192 the smallest fused ring, not folded; 16384 at L = 4, 6 (the 124-bit form of
# scale-and-round's reduction) and 7 (its 128-bit fallback beside column-accumulator conversions); 32768 on slices of 2^14
POINTS = ([(None, N, L) for N, L in [(256, 2), (4096, 3), (8192, 2), (8192, 7), (16384, 4), (16384, 7), (32768, 2), (32768, 7), (65536, 3)]]
          + [(1 << 50, 16384, 7), (1 << 50, 32768, 5), (1 << 61, 4096, 3), (1 << 61, 32768, 4)]
          + [(name, 4096, 3) for name in pc.NAMED] + [("q0_wide", 16384, 5)]
          + [("barrett_60", 8192, 2), ("barrett_60", 16384, 4), ("barrett_60", 16384, 6), ("barrett_60", 16384, 7), ("barrett_60", 32768, 2)]
          + [("fold_edge", 16384, 4), ("fold_edge", 16384, 6), ("fold_edge", 32768, 2)])
ONE_LIMB = (None, 256, 1)


# What ntt_plan_decide makes of each point, written out rather than computed by the library's rule, so that a change of the rule shows:
#   lane      the register-blocked transforms and their lane order (every modulus and t below 2^60, N >= 4096)
#   fused     tensor product in the load phase of the inverse transform (fused_tensor; with it d01_eval_q and x_direct): the
#             16-coefficient kernel (N = 8192 .. 32768) on a chain with every modulus in (2^59, 2^60)
#   mult_dig  the digits class of a relinearising product: absent where the lane-order lift is fused into the 32-coefficient forward
#             transform (N = 4096) or rides in the 16-coefficient launch of d0, d1 (Ntt16Digits, 60-bit chains); present where
#             digits_kernel<FOLD> runs (FOLD at N = 16384, 32768 on other chains; unfolded elsewhere)
#   auto_dig  the digits class of a key switch in standard order: absent where lift_digit is fused into the 32-coefficient forward
#             transform (lane order, N <= 16384); present where digits_kernel<false> runs
# (lane, fused, mult_dig, auto_dig):
ROUTES = {
    (None, 256, 2): (False, False, True, True), (None, 256, 1): (False, False, True, True),
    (None, 4096, 3): (True, False, False, False),
    (None, 8192, 2): (True, True, False, False), (None, 8192, 7): (True, True, False, False),
    (None, 16384, 4): (True, True, False, False), (None, 16384, 7): (True, True, False, False),
    (None, 32768, 2): (True, True, False, True), (None, 32768, 7): (True, True, False, True),
    (None, 65536, 3): (True, False, True, True),
    (1 << 50, 16384, 7): (True, False, True, False), (1 << 50, 32768, 5): (True, False, True, True),
    (1 << 61, 4096, 3): (False, False, True, True), (1 << 61, 32768, 4): (False, False, True, True),
    ("q0_wide", 4096, 3): (True, False, False, False), ("q_narrow_p_wide", 4096, 3): (True, False, False, False),
    ("one_p_61", 4096, 3): (False, False, True, True), ("barrett_edges", 4096, 3): (True, False, False, False),
    ("q0_wide", 16384, 5): (True, False, True, False),
    ("barrett_60", 8192, 2): (True, True, False, False),
    ("barrett_60", 16384, 4): (True, True, False, False), ("barrett_60", 16384, 6): (True, True, False, False),
    ("barrett_60", 16384, 7): (True, True, False, False), ("barrett_60", 32768, 2): (True, True, False, True),
    ("fold_edge", 16384, 4): (True, True, False, False), ("fold_edge", 16384, 6): (True, True, False, False),
    ("fold_edge", 32768, 2): (True, True, False, True),
}
# How each point's context reduces its variable x variable column sums (PieContext.reduction()), written out like ROUTES: "fold" (every
# Q and P modulus 2^60 - d, d < 2^27), "barrett" (every one in (2^59, 2^60), some d >= 2^27), "wide" (some modulus outside)
REDUCTION = {
    (None, 256, 2): "fold", (None, 256, 1): "fold", (None, 4096, 3): "fold", (None, 8192, 2): "fold", (None, 8192, 7): "fold",
    (None, 16384, 4): "fold", (None, 16384, 7): "fold", (None, 32768, 2): "fold", (None, 32768, 7): "fold", (None, 65536, 3): "fold",
    (1 << 50, 16384, 7): "wide", (1 << 50, 32768, 5): "wide", (1 << 61, 4096, 3): "wide", (1 << 61, 32768, 4): "wide",
    ("q0_wide", 4096, 3): "wide", ("q_narrow_p_wide", 4096, 3): "wide", ("one_p_61", 4096, 3): "wide", ("barrett_edges", 4096, 3): "barrett",
    ("q0_wide", 16384, 5): "wide",
    ("barrett_60", 8192, 2): "barrett", ("barrett_60", 16384, 4): "barrett", ("barrett_60", 16384, 6): "barrett",
    ("barrett_60", 16384, 7): "barrett", ("barrett_60", 32768, 2): "barrett",
    ("fold_edge", 16384, 4): "fold", ("fold_edge", 16384, 6): "fold", ("fold_edge", 32768, 2): "fold",
}
assert set(REDUCTION) == set(ROUTES) == set(POINTS) | {ONE_LIMB}


def _pid(point):
    chain, N, L = point
    name = "default" if chain is None else chain if isinstance(chain, str) else "below2^%d" % (chain.bit_length() - 1)
    return "%s-%d-%d" % (name, N, L)


def _params(points):
    return [pytest.param(p, id=_pid(p)) for p in points]


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


@functools.lru_cache(maxsize=2)
def _oracle(point, t=T32):
    from oracle import binding as ob
    chain, N, L = point
    if chain is None:
        return ob.Oracle(N, L, t)
    q, p = pc.uniform_chain(N, L, chain) if isinstance(chain, int) else pc.chain_by_name(N, L, chain)
    return ob.Oracle(N, L, t, q, p)


def _context(pie, o, point):
    cc = pie.PieContext(o.N, o.L, o.t, o.q, o.p)
    assert (cc.moduli == o.moduli).all()
    assert cc.reduction() == REDUCTION[point], "the reduction kind of %s" % _pid(point)
    return cc


def _profiled(cc, fn):
    cc.set_profiling(True)
    out = fn()
    prof = cc.profile()
    cc.set_profiling(False)
    return out, prof


# ---- (a) the conversions by themselves -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("point,t,kind", [pytest.param(p, T32, kind, id="%s-kind%d" % (_pid(p), kind)) for p in POINTS + [ONE_LIMB] for kind in (0, 1, 2)]
                         + [pytest.param((None, 16384, 4), T48, 2, id="default-16384-4-T48-kind2")])
def test_base_convert(pie, point, t, kind):
    """piehip_base_convert: the unfolded instances of expand_core (kind 0), scale_pq_core (1) and the scale-and-round kernel (2), in
    their mad (60-bit chains) and generic arithmetic.  Kinds 0 and 1 take every family over Q, kind 2 the digit extremes over QP and
    the ties of round(t d/P) -- t enters that tie, hence the second plaintext modulus at (16384, 4)"""
    o = _oracle(point, t)
    N = o.N
    rng = np.random.default_rng(N + 7 * o.L + kind)
    cc = _context(pie, o, point)
    if kind == 2:
        fam = ccol.qp_families(o, rng)
        x = np.stack([ccol.tile(fam, N, rng) for _ in range(3)])
        want = np.stack([o.scale_round_tp(v) for v in x])
    else:
        fam = ccol.q_families(o)
        x = np.stack([ccol.tile(fam, N, rng) for _ in range(2)])
        want = np.stack([(o.scale_pq_expand if kind else o.expand_q_to_qp)(v) for v in x])
    got = cc.base_convert(kind, x)
    cc.close()
    bad = np.argwhere(got != want)
    where = ccol.tile_map(fam, N)
    assert not len(bad), "first of %d: poly %d limb %d n %d, family %s" % ((len(bad),) + tuple(bad[0]) + (where.get(int(bad[0][2]), ("uniform",))[0],))


# ---- (b) the product chain -----------------------------------------------------------------------------------------------------
def _crafted_ct(o, fam, rng):
    return np.stack([ccol.ntt_q(o, ccol.tile(fam, o.N, rng)) for _ in range(2)])


@pytest.mark.parametrize("point", _params(POINTS + [ONE_LIMB]))
def test_eval_mult(pie, point):
    """EvalMult on operands whose four polynomials are tiled with every family: X meets expand, Y scale_pq, in expand_both_kernel --
    FOLD at N = 16384 and 32768 in lane order, YIN / LZ / SKIPQ where the inverse transform of X leaves its Q limbs in the QP array
    (xq_reuse: lane order without global stages) -- then the tensor launch (fused into the inverse transform where ROUTES says
    `fused`; there a relinearising product also leaves the Q limbs of d0, d1 in EVALUATION form, d01_eval_q) and scale-and-round.
    One row (a, b) and two rows (a, b), (b, a): the families swap between X and Y.  The one-limb point has no key switch"""
    o = _oracle(point)
    lane, fused, mult_dig, _ = ROUTES[point]
    rng = np.random.default_rng(o.N + o.L)
    fam = ccol.q_families(o)
    a, b = _crafted_ct(o, fam, rng), _crafted_ct(o, fam, rng)
    d_ab, d_ba = o.mul_tensor(a, b), o.mul_tensor(b, a)
    cc = _context(pie, o, point)
    got, prof = _profiled(cc, lambda: cc.EvalMult(a, b, relin=False))
    assert (got == d_ab).all()
    assert ("tensor_ntt_inv" in prof) == fused and ("tensor" in prof) == (not fused)
    assert (cc.EvalMult(np.stack([a, b]), np.stack([b, a]), relin=False) == np.stack([d_ab, d_ba])).all()
    if point != ONE_LIMB:
        evk = rand_limbs(rng, o.q, (o.L, 2), o.N)
        cc.load_relin_key(evk)
        r_ab, r_ba = o.relin(d_ab, evk), o.relin(d_ba, evk)
        got, prof = _profiled(cc, lambda: cc.EvalMult(a, b, relin=True))
        assert (got == r_ab).all()
        assert ("tensor_ntt_inv" in prof) == fused and ("digits" in prof) == mult_dig
        assert (cc.EvalMult(np.stack([a, b]), np.stack([b, a]), relin=True) == np.stack([r_ab, r_ba])).all()
    cc.close()


# ---- (c) digit lifts in standard order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_name", ["5", "2N-1"])
@pytest.mark.parametrize("point", _params(POINTS))
def test_automorphism_lifts_windows(pie, point, g_name):
    """EvalAutomorphism of c with c1 = ntt(sigma_1/g(w)), w tiled with the lift windows and digit extremes: the key switch lifts the
    columns of w itself.  lift_digit fused into the 32-coefficient forward transform where ROUTES says auto_dig is absent,
    digits_kernel<false> and a plain transform elsewhere (no lane order, or N >= 32768); q_i >= 2 q_j (barrett128) on q0_wide"""
    o = _oracle(point)
    N, L = o.N, o.L
    qs, _ = ccol.moduli(o)
    g = 5 if g_name == "5" else 2 * N - 1
    rng = np.random.default_rng(N + L + g)
    w = ccol.tile(ccol.window_families(o), N, rng)
    c = np.stack([rand_limbs(rng, o.q, (), N), ccol.ntt_q(o, ccol.sigma(w, pow(g, -1, 2 * N), qs))])
    rk = rand_limbs(rng, o.q, (L, 2), N)
    want = o.automorph(c, g, rk)
    cc = _context(pie, o, point)
    got, prof = _profiled(cc, lambda: cc.EvalAutomorphism(c, g, rk))
    cc.close()
    assert (got == want).all()
    assert ("digits" in prof) == ROUTES[point][3]


# ---- (d) digit lifts in lane order -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", _params(POINTS))
def test_relin_lifts_crafted_d2(pie, point):
    """EvalMult(relin=True) whose d2 holds the lift windows and digit extremes in every coefficient (coeff_columns.solve_d2 steers
    it from outside: a1 constant, b1 solved per coefficient).  The lane-order lifts: fused into the 32-coefficient forward transform
    at N = 4096, Ntt16Digits at N = 8192 .. 32768 on 60-bit chains (mult_dig absent in ROUTES), digits_kernel<true> on the folded
    other chains (1 << 50 and q0_wide at 16384, 32768), digits_kernel<false> elsewhere"""
    o = _oracle(point)
    rng = np.random.default_rng(o.N + 3 * o.L)
    fam = ccol.window_families(o)
    targets = fam["windows"] + fam["digits"]
    a, b = ccol.d2_operands(o, targets, rng)
    d = o.mul_tensor(a, b)
    d2 = ccol.intt_q(o, d[2])
    for n in (0, 1, len(targets) - 1, o.N // 2, o.N - 1):
        assert tuple(int(v) for v in d2[:, n]) == targets[n % len(targets)]
    evk = rand_limbs(rng, o.q, (o.L, 2), o.N)
    want = o.relin(d, evk)
    cc = _context(pie, o, point)
    cc.load_relin_key(evk)
    got, prof = _profiled(cc, lambda: cc.EvalMult(a, b, relin=True))
    cc.close()
    assert (got == want).all()
    assert ("digits" in prof) == ROUTES[point][2]


# ---- (e) run(): X from stage A ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", _params(POINTS))
def test_run_with_crafted_index(pie, point):
    """run() with K = 2, E = 1, database plaintexts 1 and minus = 0: stage A hands the index ciphertexts themselves to the product, so
    the product's operands are the crafted ones.  One query, and a batch of three with the crafted query in slot 1 -- where ROUTES
    says `fused`, stage A of a batch writes X in lane order into the QP array (x_direct) and expand_both_kernel reuses those Q limbs
    (xq_reuse) -- on one queue and on two"""
    o = _oracle(point)
    N, L = o.N, o.L
    K, E, b, nq = 2, 1, 2, 3
    rng = np.random.default_rng(N + 5 * L)
    fam = ccol.q_families(o)
    crafted = np.stack([_crafted_ct(o, fam, rng), _crafted_ct(o, fam, rng)]).reshape(K, E, 2, L, N)
    db = np.ones((K, b, E, L, N), dtype=np.uint64)
    zero = np.zeros((2, L, N), dtype=np.uint64)
    masks, evk = rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
    queries = [rand_limbs(rng, o.q, (K, E, 2), N), crafted, rand_limbs(rng, o.q, (K, E, 2), N)]
    want = [o.pie_run(idx, zero, db, masks, evk) for idx in queries]
    # the product's operands are the index ciphertexts: asserted from the oracle
    prod = o.mul(crafted[0, 0], crafted[1, 0], evk)
    assert (want[1] == np.stack([o.mul_plain(prod, masks[bn]) for bn in range(b)])).all()
    cc = _context(pie, o, point)
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    for queues in (1, 2):
        cc.set_run_streams(queues)
        op.setQueryBatch(1)
        op.setIndex(crafted)
        op.setMinusCompareElement(zero)
        op.run()
        assert (op.getResultList() == want[1]).all(), "one query, %d queue(s)" % queues
        op.setQueryBatch(nq)
        for i, idx in enumerate(queries):
            op.setIndex(idx, query=i)
            op.setMinusCompareElement(zero, query=i)
        op.run()
        got = op.getResultList()
        for i in range(nq):
            assert (got[i] == want[i]).all(), "query %d of the batch, %d queue(s)" % (i, queues)
    cc.close()
