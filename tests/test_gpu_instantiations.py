"""One case per compiled kernel that the rest of the GPU suite never launched (profiles/instantiation_coverage/before_unlaunched.txt:
the suite traced with rocprofv3, set against the device listings by tools/instantiation_coverage.py) and that the product can reach.

The limb count, the arithmetic kind and the flags are template arguments of the conversion kernels, so every instantiation has its
own unrolled CRT sums and reduction blocks; a case here is the smallest call whose host-side dispatch selects the instantiation its
id names.  ROWS states, per instantiation, the dispatcher and the condition read there.  Every output word is compared with the
oracle or the exact definition, bit for bit; where the profile can tell the route (class counts of PieContext.profile(), the kinds
of PieContext.reduction()), the case asserts it first.  No tolerance and no skip: a shape that cannot run fails.

Arithmetic kinds (ArithKind 0, 1, 2 = wide, barrett, fold; tests/param_chains.py): the default chain folds, barrett_60 is of the Barrett
kind, the uniform chain below 2^50 is wide.  one_p_61 and barrett_one_p_61 carry one 61-bit P prime: the parent has no lazy transforms
(no lane order, no folding) while every level below L has.

Inputs: the conversions and the drops get the crafted columns of tests/coeff_columns.py (digit extremes, ties, lift windows, the
drop's branch at every step), beside one uniform draw and the 0 / q - 1 pattern of extreme_run (tests/test_gpu_envelope.py).

tests/test_instantiation_coverage.py checks on the CPU that every name of before_unlaunched.txt has a row here or a reason in
profiles/instantiation_coverage/unreachable.txt.
"""
import numpy as np
import pytest

from tests import coeff_columns as ccol
from tests import param_chains as pc
from tests.param_chains import T32
from tests.test_chain_drop_columns import case_families, make_oracle
from tests.test_gpu_chain_drop_columns import _check_route, _profiled, _run, _setup
from tests.test_gpu_chain_limbs import _exact as chain_limbs_exact
from tests.test_gpu_chain_schedule import _exact as chain_schedule_exact
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu

KIND = ("wide", "barrett", "fold")                 # ArithKind, in the enum's order
KIND_CHAIN = (1 << 50, "barrett_60", None)         # a chain of each kind (chain_moduli of tests/test_chain_drop_columns.py)
# (parent, level) kinds of the chains the chain-limbs rows use
CHAIN_KINDS = {None: ("fold", "fold"), "barrett_60": ("barrett", "barrett"), 1 << 50: ("wide", "wide"),
               "one_p_61": ("wide", "fold"), "barrett_one_p_61": ("wide", "barrett")}
FUSED_PAIRS = {(2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6), (4, 2), (6, 4)}   # PIE_CHAIN_DROP_PAIRS (kernels_chain_drop.hip)


def b_(v):
    return "true" if v else "false"


ROWS = []   # (instantiation as tools/isa_compare.py prints it, driver, arguments, the host condition that selects it)


def row(name, driver, args, why):
    assert name not in [r[0] for r in ROWS], name
    ROWS.append((name, driver, args, why))


# ---- piehip_base_convert at N = 64: launch_expand_common / launch_scale_round, with_u32<1, 7>(L), with_arith(plan) ------------------
for S, L, K in [(S, L, K) for S in (0, 1) for L, K in ((1, 0), (1, 1), (5, 2), (6, 0))]:
    row("expand_kernel<%s, false, %du, (ArithKind)%d, false>" % (b_(S), L, K), "base_convert", (S, L, K),
        "launch_expand_common: piehip_base_convert kind %d (scale = %s), L = %d, a %s chain" % (S, b_(S), L, KIND[K]))
for L, K in ((5, 2), (6, 0)):
    row("scale_round_kernel<false, %du, (ArithKind)%d, false, false>" % (L, K), "base_convert", (2, L, K),
        "launch_scale_round: piehip_base_convert kind 2 (fold, p_only01, p_only2 all false), L = %d, a %s chain" % (L, KIND[K]))

# ---- piehip_eval_mult: launch_expand_pair (x.poly == y.poly), with_bools(fold = plan.fold, x.q_ready = plan.xq_reuse) ----------------
# plan.fold: N = 16384, 32768 in lane order.  plan.xq_reuse: lane order without global stages (N = 4096 .. 32768, moduli below 2^60).
for F, Q, N, LK in [
        (0, 0, 2048, ((1, 0), (1, 1), (2, 1), (4, 1), (5, 1), (5, 2), (6, 0), (6, 1), (7, 0), (7, 1))),
        (0, 1, 4096, ((1, 0), (4, 0), (4, 1), (5, 0), (5, 1), (5, 2), (6, 0), (6, 1), (6, 2), (7, 0), (7, 1))),
        (1, 1, 16384, ((1, 0), (3, 0), (6, 0)))]:
    for L, K in LK:
        row("expand_both_kernel<%s, %du, (ArithKind)%d, %s>" % (b_(F), L, K, b_(Q)), "eval_mult", (N, L, K, False),
            "launch_expand_pair: EvalMult at N = %d (plan.fold %s, plan.xq_reuse %s), L = %d, a %s chain" % (N, b_(F), b_(Q), L, KIND[K]))

# ---- enqueue_mul -> launch_scale_round(fold = plan.fold, p_only01 = relin && plan.d01_eval_q) ---------------------------------------
# plan.d01_eval_q = plan.fused_tensor: the 16-coefficient kernel (N = 8192 .. 32768) on a chain of a column-accumulator kind
for L, K in ((1, 0), (6, 0)):
    row("scale_round_kernel<true, %du, (ArithKind)%d, false, false>" % (L, K), "eval_mult", (16384, L, K, True),
        "launch_scale_round: EvalMult on the folded ring 16384, a wide chain (no fused tensor product, so p_only01 false), L = %d" % L)
for L, K in ((1, 1), (1, 2), (3, 1)):
    row("scale_round_kernel<true, %du, (ArithKind)%d, false, false>" % (L, K), "eval_mult", (16384, L, K, False),
        "launch_scale_round: EvalMult(relin = false) on the folded ring 16384 (fold_comp2, p_only01 false), L = %d, %s" % (L, KIND[K]))
for L, K in ((4, 1), (5, 1), (5, 2), (6, 1), (6, 2), (7, 1)):
    row("scale_round_kernel<false, %du, (ArithKind)%d, true, false>" % (L, K), "eval_mult", (8192, L, K, True),
        "launch_scale_round: relinearising EvalMult at N = 8192 (plan.d01_eval_q, no folding), L = %d, %s" % (L, KIND[K]))
# run() without the last relinearisation: launch_scale_round(.., fold_comp2, p_only01, p_only2) where plan.result_eval_q
for F, N, LK in [(0, 8192, ((1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (4, 1), (4, 2), (5, 1), (5, 2), (6, 1), (6, 2), (7, 1), (7, 2))),
                 (1, 16384, ((1, 1), (1, 2), (3, 1), (4, 1), (5, 1), (5, 2), (6, 1)))]:
    for L, K in LK:
        row("scale_round_kernel<%s, %du, (ArithKind)%d, true, true>" % (b_(F), L, K), "run_deg2", (N, L, K),
            "launch_scale_round: run() with piehip_set_result_relin(0) at N = %d (plan.result_eval_q, plan.fold %s), L = %d, %s"
            % (N, b_(F), L, KIND[K]))

# ---- run() with chain limbs, the drop kernel's route: launch_chain_drop(fold = top.plan->fold), then launch_expand_pair (x.plain) ----
# enqueue_chain_bins takes it where the fused conversion does not apply: an unfolded parent, a wide level, or a pair not in FUSED_PAIRS


def chain_row(name, chain, N, L, Lc, K=2):
    fused = (N in (16384, 32768) and CHAIN_KINDS[chain][0] != "wide" and CHAIN_KINDS[chain][1] != "wide" and (L, Lc) in FUSED_PAIRS)
    folded = N in (16384, 32768) and chain not in ("one_p_61", "barrett_one_p_61")
    route = "fused" if fused else "folded" if folded else "unfolded"
    row(name, "chain", ((chain, N, L, Lc), K, route),
        "enqueue_chain_bins: run() with chain limbs %d of %d at N = %d, chain %s, K = %d: route %s"
        % (Lc, L, N, "default" if chain is None else chain, K, route))


for L, Lc in [(L, Lc) for L in (5, 6, 7) for Lc in range(1, L)]:
    chain_row("chain_drop_kernel<false, %du, %du>" % (L, Lc), None, 4096, L, Lc)
for L, Lc in [(3, 1), (4, 1), (5, 1), (6, 1), (6, 2), (6, 3), (7, 2), (7, 3), (7, 4), (7, 5)]:      # pairs the fused kernel is not built for
    chain_row("chain_drop_kernel<true, %du, %du>" % (L, Lc), None, 16384, L, Lc)
for L, Lc in [(2, 1), (4, 2), (5, 4), (6, 4), (6, 5), (7, 6)]:                                          # built pairs: a wide chain
    chain_row("chain_drop_kernel<true, %du, %du>" % (L, Lc), 1 << 50, 16384, L, Lc)
for Lc, K in [(Lc, K) for Lc in (3, 4, 5, 6) for K in (0, 1, 2) if (Lc, K) != (3, 2)]:
    chain_row("expand_both_plain_kernel<false, %du, (ArithKind)%d>" % (Lc, K), KIND_CHAIN[K], 4096, Lc + 1, Lc)
chain_row("expand_both_plain_kernel<true, 1u, (ArithKind)0>", 1 << 50, 16384, 2, 1)
chain_row("expand_both_plain_kernel<true, 1u, (ArithKind)1>", "barrett_60", 16384, 3, 1)
chain_row("expand_both_plain_kernel<true, 3u, (ArithKind)1>", "barrett_60", 16384, 5, 3)
for Lc in (4, 5):
    chain_row("expand_both_plain_kernel<true, %du, (ArithKind)0>" % Lc, 1 << 50, 16384, Lc + 1, Lc)
    chain_row("expand_both_plain_kernel<true, %du, (ArithKind)1>" % Lc, "barrett_60", 16384, 7, Lc)
    chain_row("expand_both_plain_kernel<true, %du, (ArithKind)2>" % Lc, None, 16384, 7, Lc)
# six limbs on a folded level: (7, 6) is a fused pair, so the column-accumulator kinds get here only behind a parent that does not fold
chain_row("expand_both_plain_kernel<true, 6u, (ArithKind)0>", 1 << 50, 16384, 7, 6)
chain_row("expand_both_plain_kernel<true, 6u, (ArithKind)1>", "barrett_one_p_61", 16384, 7, 6)
chain_row("expand_both_plain_kernel<true, 6u, (ArithKind)2>", "one_p_61", 16384, 7, 6)

# ---- the fused route: launch_expand_pair (y.src_L > L), PIE_CHAIN_DROP_PAIRS, with_bools(xdrop) ---------------------------------------
# XDROP: the first product (X an accumulator on the parent's limbs); false: a later product of K = 3, X on the level with its Q limbs
for L, Lc in ((2, 1), (4, 3), (5, 4), (6, 4), (7, 6)):
    chain_row("expand_both_drop_kernel<%du, %du, true, (ArithKind)1>" % (L, Lc), "barrett_60", 16384, L, Lc)
for L, Lc in ((2, 1), (4, 3), (5, 4), (6, 4), (6, 5), (7, 6)):
    chain_row("expand_both_drop_kernel<%du, %du, false, (ArithKind)1>" % (L, Lc), "barrett_60", 16384, L, Lc, K=3)
chain_row("expand_both_drop_kernel<6u, 4u, false, (ArithKind)2>", None, 16384, 6, 4, K=3)
# PIE_CHAIN_DROP_TRIPLES: a chain schedule whose second product lies below the first (Y from LY limbs, X from LX, both to LC)
for LY, LX, LC in ((4, 3, 2), (6, 4, 3)):
    row("expand_both_drop_xy_kernel<%du, %du, %du, (ArithKind)1>" % (LY, LX, LC), "schedule", ("barrett_60", 16384, LY, (LX, LC)),
        "launch_expand_pair: chain schedule (%d, %d) on L = %d, K = 3, barrett_60 at N = 16384 (y.src_L = %d, x.src_L = %d)" % (LX, LC, LY, LY, LX))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def extreme_limbs(rng, q, shape, N):
    """the 0 / q - 1 pattern of extreme_run (tests/test_gpu_envelope.py; the same positions from N = 256 on): runs of q - 1 and of 0 at
    the start, q - 1 at the start of the second half and at the end, uniform elsewhere"""
    a = rand_limbs(rng, q, shape, N)
    w = min(64, N // 4)
    for i in range(len(q)):
        a[..., i, 0:w] = q[i] - np.uint64(1)
        a[..., i, w:2 * w] = 0
        a[..., i, N // 2:N // 2 + w // 2] = q[i] - np.uint64(1)
        a[..., i, N - w // 2:] = q[i] - np.uint64(1)
    return a


def _context(pie, o, chain, kind):
    q, p = (None, None) if chain is None else (o.q, o.p)
    cc = pie.PieContext(o.N, o.L, o.t, q, p)
    assert (cc.moduli == o.moduli).all()
    assert cc.reduction() == kind, "the reduction kind"
    return cc


def _first_bad(got, want):
    bad = np.argwhere(got != want)
    return "%d words differ, first at %s" % (len(bad), tuple(bad[0]) if len(bad) else None)


# ---- drivers ------------------------------------------------------------------------------------------------------------------------
def base_convert(ob, pie, which, L, K):
    """every crafted column of the chain (as many polynomials of 64 coefficients as they need), the 0 / q - 1 pattern and a uniform
    draw; kinds 0 and 1 take polynomials in pairs, kind 2 in triples"""
    N = 64
    o = make_oracle(KIND_CHAIN[K], N, L)
    rng = np.random.default_rng(64 * L + 8 * K + which)
    fam = ccol.qp_families(o, rng) if which == 2 else ccol.q_families(o)
    mods = np.array(fam.moduli, dtype=np.uint64)
    cols = [c for cs in fam.values() for c in cs]
    x = [ccol.columns_polys(cols, fam.moduli, N), extreme_limbs(rng, mods, (1,), N), rand_limbs(rng, mods, (1,), N)]
    group = 3 if which == 2 else 2
    pad = -sum(len(v) for v in x) % group
    if pad:
        x.append(rand_limbs(rng, mods, (pad,), N))
    x = np.ascontiguousarray(np.concatenate(x))
    conv = (o.expand_q_to_qp, o.scale_pq_expand, o.scale_round_tp)[which]
    want = np.stack([conv(v) for v in x])
    cc = _context(pie, o, KIND_CHAIN[K], KIND[K])
    got = cc.base_convert(which, x)
    cc.close()
    assert (got == want).all(), _first_bad(got, want)


def eval_mult(ob, pie, N, L, K, relin):
    """three rows in one call: operands tiled with every family of tests/coeff_columns.py (X meets expand, Y scale_pq), the 0 / q - 1
    pattern, a uniform draw"""
    chain = KIND_CHAIN[K]
    o = make_oracle(chain, N, L)
    rng = np.random.default_rng(N + 16 * L + K)
    fam = ccol.q_families(o)
    crafted = [np.stack([ccol.ntt_q(o, ccol.tile(fam, N, rng)) for _ in range(2)]) for _ in range(2)]
    x = np.stack([crafted[0], extreme_limbs(rng, o.q, (2,), N), rand_limbs(rng, o.q, (2,), N)])
    y = np.stack([crafted[1], extreme_limbs(rng, o.q, (2,), N), rand_limbs(rng, o.q, (2,), N)])
    want = [o.mul_tensor(a, b) for a, b in zip(x, y)]
    cc = _context(pie, o, chain, KIND[K])
    if relin:
        evk = extreme_limbs(rng, o.q, (L, 2), N)
        cc.load_relin_key(evk)
        want = [o.relin(d, evk) for d in want]
    want = np.stack(want)
    got, prof = _profiled(cc, lambda: cc.EvalMult(x, y, relin=relin))
    cc.close()
    fused = N in (8192, 16384, 32768) and K != 0          # plan.fused_tensor: the 16-coefficient kernel, column-accumulator kinds
    assert ("tensor_ntt_inv" in prof) == fused and ("tensor" in prof) == (not fused), sorted(prof)
    assert prof["expand"]["launches"] == 1 and prof["scale_round"]["launches"] == 1      # one launch of each for the three rows
    assert (got == want).all(), _first_bad(got, want)


def run_deg2(ob, pie, N, L, K):
    """run() with K = 2, E = 1, database plaintexts 1 and minus = 0, no key: stage A hands the index ciphertexts themselves to the one
    product, which leaves as three components through deg2_finish.  The crafted query, then the 0 / q - 1 pattern"""
    chain = KIND_CHAIN[K]
    o = make_oracle(chain, N, L)
    rng = np.random.default_rng(N + 32 * L + K)
    fam = ccol.q_families(o)
    db = np.ones((2, 1, 1, L, N), dtype=np.uint64)
    zero = np.zeros((2, L, N), dtype=np.uint64)
    masks = rand_limbs(rng, o.q, (1,), N)
    crafted = np.stack([np.stack([ccol.ntt_q(o, ccol.tile(fam, N, rng)) for _ in range(2)]) for _ in range(2)]).reshape(2, 1, 2, L, N)
    queries = [(crafted, zero), (extreme_limbs(rng, o.q, (2, 1, 2), N), extreme_limbs(rng, o.q, (2,), N))]
    want = chain_limbs_exact(ob, o, queries, db, masks, [None, None], L, relin_last=False)
    cc = _context(pie, o, chain, KIND[K])
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    op.setResultRelin(False)
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus)
        op.setIndex(idx)
        got, prof = _profiled(cc, lambda: _run(cc, op))
        assert "deg2_finish" in prof and "tensor_ntt_inv" in prof, sorted(prof)
        assert got.shape == (1, 1, 3, L, N)
        assert (got[0] == want[i]).all(), "query %d: %s" % (i, _first_bad(got[0], want[i]))
    cc.close()


def chain(ob, pie, case, K, route):
    """tests/test_gpu_chain_drop_columns.py's run(): the accumulators are index ciphertexts tiled with drop_families of the pair (the
    drop's branch at every step, the level's own digit extremes, ties and windows behind it), b = 1"""
    name, N, L, Lc = case
    o, cc, op, queries, db, masks, evks = _setup(ob, pie, case, K, 1, 1)
    want = chain_limbs_exact(ob, o, queries, db, masks, evks, Lc)
    op.setChainLimbs(Lc)
    assert (cc.reduction(), cc.reduction(level=Lc)) == CHAIN_KINDS[name], "the kinds of parent and level"
    got, prof = _profiled(cc, lambda: _run(cc, op))
    cc.close()
    _check_route(prof, route)
    assert got.shape == (1, 1, 2, Lc, N)
    assert (got == want).all(), _first_bad(got, want)


def schedule(ob, pie, name, N, L, sched):
    """K = 3, E = 2, b = 1 under a chain schedule: a uniform query, then the 0 / q - 1 pattern in every array of the query"""
    K, E = 3, 2
    o = make_oracle(name, N, L)
    rng = np.random.default_rng(N + 8 * L + sum(sched))
    db, masks, evk = rand_limbs(rng, o.q, (K, 1, E), N), rand_limbs(rng, o.q, (1,), N), rand_limbs(rng, o.q, (L, 2), N)
    queries = [(rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)),
               (extreme_limbs(rng, o.q, (K, E, 2), N), extreme_limbs(rng, o.q, (2,), N))]
    want = chain_schedule_exact(ob, o, queries, db, masks, [evk, evk], sched)
    cc = _context(pie, o, name, CHAIN_KINDS[name][0])
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    op.setChainSchedule(sched)
    for lv in sched:
        assert cc.reduction(level=lv) == CHAIN_KINDS[name][1]
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus)
        op.setIndex(idx)
        got, prof = _profiled(cc, lambda: _run(cc, op))
        _check_route(prof, "fused")
        assert got.shape == (1, 1, 2, sched[-1], N)
        assert (got[0] == want[i]).all(), "query %d: %s" % (i, _first_bad(got[0], want[i]))
    cc.close()


DRIVERS = {"base_convert": base_convert, "eval_mult": eval_mult, "run_deg2": run_deg2, "chain": chain, "schedule": schedule}


@pytest.mark.parametrize("driver,args", [pytest.param(r[1], r[2], id=r[0]) for r in ROWS])
def test_instantiation(ob, pie_mod, driver, args):
    DRIVERS[driver](ob, pie_mod, *args)
