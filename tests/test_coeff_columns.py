"""The crafted coefficient columns of tests/coeff_columns.py: that the builders deliver what they claim, and the C oracle against exact
arithmetic (oracle/exact.py) on every family.

The oracle rounds with a sum of truncated 60-bit fractions; tests/arith_check/chk_modarith.h states the contract of one fraction
(fixfrac): it is below the true value by less than 2^-59, two units of 2^-60.  A rounding over n terms can therefore differ from exact
rounding only where the exact value is within 2n units of a half-integer, and then by one.  The tests take 2n + 2 as the zone (n = L
for a rounding over the Q limbs, L + 1 over the P limbs): outside it the oracle must equal exact arithmetic, inside it the rounded
integer may be off by one -- every limb of the output then moves together -- and nothing else is allowed.  The tie families sit inside
that zone on purpose: they are the columns the GPU kernels have to reproduce bit for bit (tests/test_gpu_coeff_columns.py).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact as ex
from tests import coeff_columns as ccol
from tests import param_chains as pc

T32 = pc.T32
N = 64

CHAINS = [None, 1 << 50, 1 << 61] + list(pc.NAMED)


def _chain_id(chain):
    return "default" if chain is None else chain if isinstance(chain, str) else "below2^%d" % (chain.bit_length() - 1)


def _oracle(ob, L, chain, n=N):
    if chain is None:
        return ob.Oracle(n, L, T32)
    q, p = pc.uniform_chain(n, L, chain) if isinstance(chain, int) else pc.named_chain(n, L, chain)
    return ob.Oracle(n, L, T32, q, p)


# barrett_edges holds two special primes in Q: it has no chain of one limb
CASES = [pytest.param(L, chain, id="L%d-%s" % (L, _chain_id(chain))) for chain in CHAINS for L in (1, 3, 7)
         if not (L == 1 and chain == "barrett_edges")]


def _apply(fn, cols, nin, n=N):
    """fn over the columns, N coefficients a call"""
    out = []
    for s in range(0, len(cols), n):
        part = cols[s:s + n]
        got = fn(ccol.columns_poly(part, range(nin), n))
        out += ccol.cols_of(got)[:len(part)]
    return out


# ---- the builders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chain", CASES)
def test_digit_extremes_have_their_digits(ob, L, chain):
    o = _oracle(ob, L, chain)
    qs, ps = ccol.moduli(o)
    for mods in (qs, qs + ps):
        cols = ccol.digit_extremes(mods)
        assert len(cols) == len(mods) + 3
        assert [ccol.digits_of(c, mods) for c in cols] == ccol.digit_sets(mods)
        assert all(0 <= x < m for c in cols for x, m in zip(c, mods))
    # all q_i - 1: the largest rounding count, v = L
    Q = ex.prod(qs)
    x = ex.crt(ccol.digit_extremes(qs)[0], qs)
    assert (sum((q - 1) * (Q // q) for q in qs) - ex.centered(x, Q)) // Q == L


@pytest.mark.parametrize("L,chain", CASES)
def test_ties_sit_where_stated(ob, L, chain):
    """the exact pre-rounding value of tie column k is |k| units of 2^-60 from a half-integer, to within one unit and one integer step
    (a step is below a unit on every chain of two limbs or more; the columns of a one-limb chain are neighbouring integers)"""
    o = _oracle(ob, L, chain)
    qs, ps = ccol.moduli(o)
    Q, P = ex.prod(qs), ex.prod(ps)
    ks = ccol.tie_ks(L)
    assert set(ks) >= {0, 1, -1, 2, -2, 3, -3, 4, -4, L, -L, 2 * L + 2, -(2 * L + 2), 64, -64, 1 << 10, -(1 << 10)}
    fams = [(ccol.ties_expand(o), Q, lambda x: (x, Q)),                                            # x / Q
            (ccol.ties_expand(o), Q, lambda x: (ex.rnd_div(P * ex.centered(x, Q), Q), P)),         # round(P x/Q) / P
            (ccol.ties_scale_first(o), Q, lambda x: (P * x, Q)),                                   # P x / Q
            (ccol.ties_scale_round(o, np.random.default_rng(L)), P, lambda d: (o.t * d, P))]       # t d / P
    for n, (fam, M, value) in enumerate(fams):
        step = Fraction(1 << 60, M)
        tol = 1 + step + Fraction(1 << 60, P)
        if L > 1:
            assert tol < 2 and abs(ccol.tie_unit(M) * step - 1) < Fraction(1, 1 << 20)
        for k in ks:
            dist = ccol.tie_distance(*value(fam[k]))
            assert abs(dist - abs(k) * ccol.tie_unit(M) * step) < tol, "family %d, k = %d: %.3f units" % (n, k, float(dist))
        for lab in ("floor", "floor+1"):
            assert ccol.tie_distance(*value(fam[lab])) < tol
    e = ccol.ties_expand(o)
    assert (e["floor"], e["floor+1"], e["x=0"], e["x=1"], e["x=-1"]) == (Q // 2, Q // 2 + 1, 0, 1, Q - 1)
    r = ccol.ties_scale_round(o, np.random.default_rng(L))
    assert all(0 <= d < Q * P for d in r.values()) and len({d // P for d in r.values()}) > len(ks) // 2


@pytest.mark.parametrize("L,chain", CASES)
def test_lift_windows_hold_every_edge(ob, L, chain):
    o = _oracle(ob, L, chain)
    qs, _ = ccol.moduli(o)
    cols = ccol.lift_windows(qs)
    for i, qi in enumerate(qs):
        seen = {c[i] for c in cols}
        assert all(0 <= v < qi for v in seen)
        assert {qi - 1, (qi - 1) // 2, (qi + 1) // 2} <= seen
        for j, qj in enumerate(qs):
            if qj < qi:
                assert {qj - 1, qj, qj + 1, qi % qj} <= seen
                if qi >= 2 * qj:
                    for m in (1, 2, qi // qj):
                        assert {m * qj - 1, m * qj, m * qj + 1} <= seen
    if chain == "q0_wide" and L > 1:
        assert qs[0] >= 2 * qs[1]                      # the Barrett branch is there to be reached


@pytest.mark.parametrize("n", [256, 4096])
@pytest.mark.parametrize("L", [1, 2, 7])
def test_tile_places_the_families(ob, L, n):
    if L == 7 and n == 256:
        n = 512
    o = _oracle(ob, L, None, n)
    fam = ccol.q_families(o)
    where = ccol.tile_map(fam, n)
    for pos in (0, 1, n // 2 - 1, n // 2, n - 1):
        assert pos in where
    names = [k for k, v in fam.items() if v]
    for pos, (name, col) in where.items():
        assert col in fam[name]
        if pos < n // 2 and len(names) > 1:
            assert where[pos + n // 2][0] != name, "folded pair (%d, %d) holds one family" % (pos, pos + n // 2)
    placed = {(name, col) for name, col in where.values()}
    assert placed == {(name, col) for name, cols in fam.items() for col in cols}      # every column is there
    rng = np.random.default_rng(1)
    poly = ccol.tile(fam, n, rng)
    assert poly.shape == (L, n) and all((poly[i] < np.uint64(q)).all() for i, q in enumerate(fam.moduli))
    for pos, (_, col) in where.items():
        assert tuple(int(v) for v in poly[:, pos]) == col
    rest = [pos for pos in range(n) if pos not in where]
    assert len(rest) > 0 and len({int(v) for v in poly[0, rest]}) > len(rest) // 2    # the rest is not constant
    with pytest.raises(ValueError):
        ccol.tile_map(fam, 16)


@pytest.mark.parametrize("g_of", [lambda n: 5, lambda n: 2 * n - 1, lambda n: pow(5, -1, 2 * n)], ids=["5", "2N-1", "1/5"])
def test_sigma_is_the_automorphism(ob, g_of):
    """the vectorised per-limb sigma against the coefficient-list one of tests/test_oracle_exact.py, and sigma_g sigma_1/g = id"""
    from tests.test_oracle_exact import sigma as sigma_list
    o = _oracle(ob, 2, None)
    qs, _ = ccol.moduli(o)
    g = g_of(N)
    poly = ccol.uniform_poly(qs, N, np.random.default_rng(g))
    poly[:, 3] = 0
    got = ccol.sigma(poly, g, qs)
    for i, q in enumerate(qs):
        assert [int(v) for v in got[i]] == sigma_list([int(v) for v in poly[i]], g, q)
    assert (ccol.sigma(got, pow(g, -1, 2 * N), qs) == poly).all()


# ---- d2 of a product, steered from outside ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chain", [pytest.param(L, c, id="L%d-%s" % (L, _chain_id(c)))
                                     for L, c in [(2, None), (3, None), (7, None), (3, "q0_wide"), (5, "q0_wide"), (3, 1 << 50), (3, 1 << 61),
                                                  (3, "q_narrow_p_wide"), (3, "one_p_61"), (3, "barrett_edges")]])
def test_solve_d2_hits_every_target(ob, L, chain):
    """every window column and digit extreme is reached, and the oracle's own d2 = intt(mul_tensor(a, b)[2]) holds exactly those residues"""
    n = 256 if L == 7 else N
    o = _oracle(ob, L, chain, n)
    qs, _ = ccol.moduli(o)
    fam = ccol.window_families(o)
    targets = fam["windows"] + fam["digits"]
    assert len(targets) <= n
    sol = ccol.solve_d2(o, targets)
    assert sol.count(None) == 0, "%d of %d targets missed" % (sol.count(None), len(sol))
    Q = ex.prod(qs)
    for b, col in zip(sol, targets):
        assert 2 * abs(b) < Q and ccol.reduce_col(ccol.exact_d2(o, b), qs) == col
    a, b = ccol.d2_operands(o, targets, np.random.default_rng(L))
    d2 = ccol.cols_of(ccol.intt_q(o, o.mul_tensor(a, b)[2]))
    assert d2 == [targets[i % len(targets)] for i in range(n)]


# ---- the C oracle against exact arithmetic ------------------------------------------------------------------------------------------
def _in_zone(num, den, terms):
    return ccol.tie_distance(num, den) <= 2 * terms + 2


def _expand(o):
    """expand: P limb j is exact, or exact -+ (Q mod p_j) in every P limb at once, the latter only within 2L + 2 units of a tie.
    Returns (columns, columns on which the oracle differs from exact), as the two helpers below"""
    L = o.L
    qs, ps = ccol.moduli(o)
    Q = ex.prod(qs)
    fam = ccol.q_families(o)
    cols = [c for v in fam.values() for c in v]
    got = _apply(o.expand_q_to_qp, cols, L)
    want = ex.expand_q_to_qp(cols, qs, ps)
    differ = 0
    for col, g, w in zip(cols, got, want):
        if g == w:
            continue
        differ += 1
        x = ex.crt(col, qs)
        assert _in_zone(x, Q, L), "column %r differs outside the zone" % (col,)
        xh = ex.centered(x, Q)
        assert g in [col + tuple((xh + s * Q) % p for p in ps) for s in (-1, 1)], "column %r: not a rounding step" % (col,)
    return len(cols), differ


def _scale_pq_allowed(x, qs, ps):
    """output columns of scale_pq that the contract allows for input x (an integer in [0, Q))"""
    Q, P = ex.prod(qs), ex.prod(ps)
    L = len(qs)
    xh = ex.centered(x, Q)
    x1 = ex.rnd_div(P * xh, Q)
    firsts = (-1, 0, 1) if _in_zone(P * xh, Q, L) else (0,)
    out = []
    for d1 in firsts:
        xs = (x1 + d1) % P
        seconds = (-1, 0, 1) if _in_zone(xs, P, L + 1) else (0,)
        for d2 in seconds:
            c = ex.centered(xs, P) + d2 * P
            out.append(tuple(c % q for q in qs) + tuple(xs % p for p in ps))
    return out


def _scale_pq(o):
    """scale_pq: x' = round(P x/Q) is exact or off by one (P limbs -+ 1), only within 2L + 2 units of its tie; the centred lift of x'
    out of P is exact or off by one step (Q limb i -+ (P mod q_i)), only within 2(L + 1) + 2 units of its tie"""
    L = o.L
    qs, ps = ccol.moduli(o)
    fam = ccol.q_families(o)
    cols = [c for v in fam.values() for c in v]
    got = _apply(o.scale_pq_expand, cols, L)
    want = ex.scale_pq_expand(cols, qs, ps)
    differ = 0
    for col, g, w in zip(cols, got, want):
        allowed = _scale_pq_allowed(ex.crt(col, qs), qs, ps)
        assert w in allowed
        assert g in allowed, "column %r: %r is not within a rounding step of %r" % (col, g, w)
        differ += g != w
    return len(cols), differ


def _scale_round(o):
    """scale-and-round: round(t d/P) is exact, or off by one (every Q limb -+ 1) only within 2(L + 1) + 2 units of a tie"""
    L = o.L
    qs, ps = ccol.moduli(o)
    P = ex.prod(ps)
    mods = qs + ps
    fam = ccol.qp_families(o, np.random.default_rng(7 * L))
    cols = [c for v in fam.values() for c in v]
    got = _apply(o.scale_round_tp, cols, 2 * L + 1)
    want = ex.scale_round_tp(cols, qs, ps, o.t)
    differ = 0
    for col, g, w in zip(cols, got, want):
        if g == w:
            continue
        differ += 1
        d = ex.centered(ex.crt(col, mods), P * ex.prod(qs))
        assert _in_zone(o.t * d, P, L + 1), "column %r differs outside the zone" % (col,)
        assert g in [tuple((v + s) % q for v, q in zip(w, qs)) for s in (-1, 1)], "column %r: not a rounding step" % (col,)
    return len(cols), differ


CONVERSIONS = {"expand": _expand, "scale_pq": _scale_pq, "scale_round": _scale_round}


@pytest.mark.parametrize("conv", list(CONVERSIONS))
@pytest.mark.parametrize("L,chain", CASES)
def test_conversion_against_exact(ob, L, chain, conv):
    """the oracle equals exact arithmetic outside the zone of 2n + 2 units around a tie and is within one rounding step inside it"""
    ncols, differ = CONVERSIONS[conv](_oracle(ob, L, chain))
    print("L=%d %s %s: %d columns, the oracle differs from exact on %d" % (L, _chain_id(chain), conv, ncols, differ))


@pytest.mark.parametrize("conv", list(CONVERSIONS))
def test_tie_families_reach_the_zone(ob, conv):
    """the tie families are where the oracle's rounding departs from exact rounding: on the 60-bit chain with L = 7 -- up to fourteen
    units of truncation -- some column of each conversion differs"""
    ncols, differ = CONVERSIONS[conv](_oracle(ob, 7, None))
    assert differ > 0, "%d columns, none inside the sensitive zone" % ncols


# ---- the digit lift against its definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chain", [pytest.param(L, c, id="L%d-%s" % (L, _chain_id(c))) for c in CHAINS for L in (3, 7)])
@pytest.mark.parametrize("g_of", [lambda n: 5, lambda n: 2 * n - 1], ids=["5", "2N-1"])
def test_digit_lift_against_definition(ob, L, chain, g_of):
    """the oracle's key switch with a key that isolates digit i (its first component 1 in every limb, everything else 0): limb j of the
    output is the transform of the lift of residue limb i into q_j, which is centred(v, q_i) mod q_j for every window value v"""
    o = _oracle(ob, L, chain)
    qs, _ = ccol.moduli(o)
    g = g_of(N)
    cols = ccol.lift_windows(qs) + ccol.digit_extremes(qs)
    for s in range(0, len(cols), N):
        w = ccol.columns_poly(cols[s:s + N], qs, N)
        c = np.zeros((2, L, N), dtype=np.uint64)
        c[1] = ccol.ntt_q(o, ccol.sigma(w, pow(g, -1, 2 * N), qs))
        for i, qi in enumerate(qs):
            rk = np.zeros((L, 2, L, N), dtype=np.uint64)
            rk[i, 0] = 1
            out = o.automorph(c, g, rk)
            assert (out[1] == 0).all()
            dig = ccol.intt_q(o, out[0])
            for j, qj in enumerate(qs):
                want = [ccol.lift_definition(int(v), qi, qj) for v in w[i]]
                assert [int(v) for v in dig[j]] == want, "digit %d in limb %d" % (i, j)
