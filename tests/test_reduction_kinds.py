"""The chains that put a context on either side of the folded reduction's selection bound (tests/param_chains.py: fold_edge,
barrett_60, last_q_over, last_p_over, q4_over), on the CPU: that they exist with the d claimed at every (N, L) the GPU files use,
which kind each must select -- recomputed here from the rule (include/piehip.h, piehip_get_reduction: every Q and P modulus in
(2^59, 2^60); then folded when every d = 2^60 - q is below 2^27), never from the library --, the kind of every level of the chains
whose levels differ from their parent, and that the tables of kinds the GPU files assert say the same.  Then the model of the folded
block (tests/fold_reduce.py, as tests/test_fold_reduce.py runs it) on the d at both ends of fold_edge.

A level of Lc limbs keeps q_0 .. q_{Lc-1} and p_0 .. p_Lc (piehip_set_chain_schedule builds it by HostParams::init on the parent's
arrays with L = Lc): param_chains.level_chain.
"""
import pytest

from oracle import exact as ex
from tests import fold_reduce as fr
from tests import param_chains as pc
from tests.test_fold_reduce import _check

BOUND = 1 << 27   # csrc/kernels.hpp: COLACC_FOLD_MAX_D
assert BOUND == pc.FOLD_MAX_D == fr.SELECT_MAX_D


def _gpu_points():
    """{(chain, N, L): [(limbs, kind), ..]} -- every point of the GPU files that names one of these chains, with the kinds that file
    asserts: of the context itself (limbs = L) and of its levels"""
    from tests import test_gpu_chain_drop_columns as drop
    from tests import test_gpu_chain_schedule as sched
    from tests import test_gpu_coeff_columns as cols
    from tests import test_gpu_lazy_inputs as lazy
    pts = {}
    for chain, N, L, kind in lazy.KIND_POINTS:
        pts.setdefault((None if chain == "default" else chain, N, L), []).append((L, kind))
    for (chain, N, L), kind in cols.REDUCTION.items():
        pts.setdefault((chain, N, L), []).append((L, kind))
    for (chain, N, L, Lc) in drop.ROUTES:
        if chain is None or chain in drop.REDUCTION:
            parent, level = drop.REDUCTION.get(chain, ("fold", "fold"))
            pts.setdefault((chain, N, L), []).extend([(L, parent), (Lc, level)])
    for N, L, chain, _, schedule, _, _, _ in sched.POINTS:
        if chain is None or chain in sched.REDUCTION:
            pts.setdefault((chain, N, L), []).extend((lv, "fold" if chain is None else sched.REDUCTION[chain][lv]) for lv in (L,) + tuple(schedule))
    return pts


def _moduli(chain, N, L):
    if chain is None:
        return pc.uniform_chain(N, L)
    return pc.uniform_chain(N, L, chain) if isinstance(chain, int) else pc.chain_by_name(N, L, chain)


def _d(q, p):
    return [(1 << 60) - int(v) for v in list(q) + list(p)]


def test_edge_chains_have_the_d_claimed():
    """fold_edge: d in (2^26, 2^27), within [0x69fffff, 0x7f6bfff] over the three fused rings; barrett_60: d in (2^27, 2^28), within
    [0x8043fff, 0x98dffff]; the primes are distinct, = 1 (mod 2N), and each chain is the nearest 2L + 1 to the bound on its side"""
    seen = [k for k in _gpu_points() if k[0] in ("fold_edge", "barrett_60")]
    assert {k[0] for k in seen} == {"fold_edge", "barrett_60"}
    for chain, N, L in seen + [(c, N, 7) for c in ("fold_edge", "barrett_60") for N in (8192, 16384, 32768)]:
        q, p = pc.chain_by_name(N, L, chain)
        ms = [int(v) for v in q] + [int(v) for v in p]
        assert len(ms) == len(set(ms)) == 2 * L + 1 and all(m % (2 * N) == 1 and ex.is_prime(m) for m in ms)
        d = _d(q, p)
        if chain == "fold_edge":
            assert all((1 << 26) < v < BOUND for v in d) and 0x69fffff <= min(d) and max(d) <= 0x7f6bfff, (N, L, [hex(v) for v in d])
            assert ms == sorted(ms) and ms == pc.prime_above(N, (1 << 60) - BOUND, 2 * L + 1)
        else:
            assert all(BOUND < v < (1 << 28) for v in d) and 0x8043fff <= min(d) and max(d) <= 0x98dffff, (N, L, [hex(v) for v in d])
            assert ms == sorted(ms, reverse=True) and ms == pc.uniform(N, 2 * L + 1, (1 << 60) - BOUND)
    # no prime = 1 (mod 2N) lies between the two chains' nearest members: they are neighbours across the bound
    for N in (8192, 16384, 32768):
        under, over = int(pc.fold_edge(N, 2)[0][0]), int(pc.barrett_60(N, 2)[0][0])
        assert pc.prime_above(N, over)[0] == under and over < (1 << 60) - BOUND < under
    assert not {"fold_edge", "barrett_60", "last_q_over", "last_p_over", "q4_over"} & set(pc.NAMED) and len(pc.NAMED) == 4


def test_one_modulus_over_the_bound_is_where_claimed():
    """last_q_over, last_p_over, q4_over: the default chain with exactly one modulus replaced, by barrett_60's first prime, at
    q_{L-1}, p_L and q_4"""
    for name, N, L, at in (("last_q_over", 16384, 3, 2), ("last_p_over", 16384, 3, 6), ("q4_over", 16384, 6, 4)):
        q, p = pc.chain_by_name(N, L, name)
        got, dflt = [int(v) for v in q] + [int(v) for v in p], pc.uniform(N, 2 * L + 1)
        over = int(pc.barrett_60(N, L)[0][0])
        assert [i for i in range(2 * L + 1) if got[i] != dflt[i]] == [at] and got[at] == over
        assert BOUND <= (1 << 60) - over < (1 << 28) and len(set(got)) == 2 * L + 1


@pytest.mark.parametrize("point", sorted(_gpu_points(), key=str), ids=lambda k: "%s-%d-%d" % (k[0] if isinstance(k[0], str) else "default" if k[0] is None else "below2^%d" % (k[0].bit_length() - 1), k[1], k[2]))
def test_kinds_the_gpu_files_assert_follow_from_the_rule(point):
    """every (context or level, kind) a GPU file writes down for this point, against the rule applied to the moduli that context keeps"""
    chain, N, L = point
    q, p = _moduli(chain, N, L)
    for limbs, kind in _gpu_points()[point]:
        assert 1 <= limbs <= L
        lq, lp = pc.level_chain(q, p, limbs)
        assert len(lq) == limbs and len(lp) == limbs + 1
        ms = [int(v) for v in lq] + [int(v) for v in lp]
        small = all((m >> 59) == 1 for m in ms)                      # (2^59, 2^60): the top bit of 60 set, nothing above
        want = "wide" if not small else "fold" if all((1 << 60) - m < BOUND for m in ms) else "barrett"
        assert kind == want == pc.reduction_kind(lq, lp), (point, limbs, kind, want)


def test_every_level_of_the_mixed_chains():
    """the parent is of the Barrett kind; last_q_over and last_p_over fold on EVERY level below L (the level drops q_{L-1} and p_L);
    q4_over is of the Barrett kind on level 5, which keeps q_4, and folds from level 4 down"""
    for name, N, L in (("last_q_over", 16384, 3), ("last_p_over", 16384, 3), ("q4_over", 16384, 6)):
        q, p = pc.chain_by_name(N, L, name)
        assert pc.reduction_kind(q, p) == "barrett"
        for Lc in range(1, L):
            lq, lp = pc.level_chain(q, p, Lc)
            d = _d(lq, lp)
            want = "barrett" if (name == "q4_over" and Lc == 5) else "fold"
            assert pc.reduction_kind(lq, lp) == want and (max(d) < BOUND) == (want == "fold"), (name, Lc)
    for chain in ("fold_edge", "barrett_60"):   # ... and a chain of one kind keeps it on every level
        q, p = pc.chain_by_name(16384, 6, chain)
        assert {pc.reduction_kind(*pc.level_chain(q, p, Lc)) for Lc in range(1, 7)} == {"fold" if chain == "fold_edge" else "barrett"}


@pytest.mark.parametrize("bits", [123, 124])
@pytest.mark.parametrize("N", [16384, 32768])
def test_fold_model_at_both_ends_of_fold_edge(N, bits):
    """the model checks of tests/test_fold_reduce.py -- fold_reduce.crafted and 2000 random columns, at sums below 2^123 and below
    2^124 -- on the largest and the smallest d of fold_edge's 15 primes"""
    d = _d(*pc.fold_edge(N, 7))
    for v in (max(d), min(d)):
        assert v < fr.MAX_D[bits]
        seen = {}
        for name, c in fr.crafted(v, bits):
            seen[name] = _check(c, v, bits, name)
        top = ((1 << bits) >> 60) - 1
        assert seen["bound - 1"]["n2"] == top and seen["c0 ones, n1 ones"]["n1"] == fr.M64
        rng = fr.rng_for(v, bits)
        for c in fr.random_columns(rng, bits, 2000):
            _check(c, v, bits, "random")
