"""The crafted columns of the limb drop (tests/coeff_columns.py: undrop, drop_families): that the builders deliver what they claim,
that the kernels' one-word operand stays inside its contract on them, and that they see what uniform columns do not.

The drop of limb l takes r = c mod q_l centred and leaves c_i <- (c_i - r) q_l^-1 mod q_i (tests/test_result_limbs.py pins this
residue form on whole integers).  The device forms -- limb_drop_kernel, chain_drop_kernel and drop_limbs inside
expand_both_drop_kernel (kernels_chain_drop.hip) -- branch on the sign mask s = [c_l > (q_l - 1)/2] and hand the Shoup product the word
x = c_i - c_l + off + (s & (q_l - off)), off the smallest multiple of q_i that is >= (q_l - 1)/2 (params.cpp).  A drop of several
limbs meets DERIVED residues from its second step on, so planting edges in the residues as given reaches the first step only: the
families here are built backwards (undrop) from the residue every step is to meet.

CASES holds every (chain, N, L, Lc) of tests/test_gpu_chain_drop_columns.py (which asserts so) and all 21 pairs of the default chain.

Columns per family, default chain: `final` has as many as the level's own families plus three -- 45, 54, 59, 64, 73, 78 at Lc = 1 .. 6
(45 at Lc = 1 on every chain, 54 or 60 at Lc = 2 on the others) -- and `kept` 8 (2 (L - Lc) - 1): 8 at Lc = L - 1, 24 at L - 2, up to
88 at (7, 1).  A drop with its threshold off by one differs from the definition on 5 to 15 of the `final` columns, on 2 of the `kept`
columns at Lc = L - 1 and on 4 elsewhere, and on none of 2000 uniform columns: test_wrong_models_pass_uniform_columns prints the
counts of every case.
"""
import functools

import numpy as np
import pytest

from oracle import exact as ex
from tests import coeff_columns as ccol
from tests import param_chains as pc
from tests.test_chain_limbs import level_oracle
from tests.test_result_limbs import drop_limbs_coeff

T32 = pc.T32

DEFAULT_PAIRS = [(L, Lc) for L in range(2, 8) for Lc in range(1, L)]
EDGE_CHAINS = ["q0_wide", "q_narrow_p_wide", "barrett_edges", "q_last_wide", 1 << 50, 1 << 61]
# piehip_mod_reduce: (chain, N, L, keep)
MOD_REDUCE = [(None, 1024, L, Lc) for L, Lc in DEFAULT_PAIRS] + [(c, 1024, 3, keep) for c in EDGE_CHAINS for keep in (2, 1)]
# run() with chain limbs: (chain, N, L, Lc)
RUN = ([(None, 16384, L, Lc) for L, Lc in [(2, 1), (3, 2), (4, 3), (4, 2), (5, 4), (6, 5), (7, 6), (5, 2), (7, 1)]]
       + [(None, 32768, 3, 2), (1 << 50, 16384, 3, 2), (1 << 50, 32768, 5, 3)]
       + [(None, 2048, 4, 2), (None, 4096, 4, 3), (None, 8192, 4, 3), (None, 65536, 3, 2), (1 << 61, 4096, 3, 2)]
       + [(c, 4096, 3, Lc) for c in ("q0_wide", "q_narrow_p_wide", "barrett_edges", "q_last_wide") for Lc in (2, 1)]
       + [("one_p_61", 16384, 3, 2)]
       # both kinds of the column-sum reduction on the folded rings (param_chains: barrett_60, fold_edge), and parents of the Barrett kind
       # whose level folds (last_q_over, last_p_over)
       + [("barrett_60", 16384, 3, 2), ("barrett_60", 16384, 4, 2), ("barrett_60", 16384, 5, 2), ("barrett_60", 32768, 3, 2)]
       + [("fold_edge", 16384, 3, 2), ("fold_edge", 16384, 5, 2), ("last_q_over", 16384, 3, 2), ("last_p_over", 16384, 3, 2)])
CASES = MOD_REDUCE + RUN


def chain_id(chain):
    return "default" if chain is None else chain if isinstance(chain, str) else "below2^%d" % (chain.bit_length() - 1)


def case_id(case):
    chain, N, L, Lc = case
    return "%s-%d-%dto%d" % (chain_id(chain), N, L, Lc)


def chain_moduli(chain, N, L):
    """(q, p) for the oracle and the library: None for the default chain"""
    if chain is None:
        return None, None
    return pc.uniform_chain(N, L, chain) if isinstance(chain, int) else pc.chain_by_name(N, L, chain)


@functools.lru_cache(maxsize=4)
def make_oracle(chain, N, L, t=T32):
    from oracle import binding as ob
    q, p = chain_moduli(chain, N, L)
    return ob.Oracle(N, L, t, q, p)


@functools.lru_cache(maxsize=4)
def case_families(case):
    """(parent oracle, level oracle, drop_families) of a case"""
    from oracle import binding as ob
    chain, N, L, Lc = case
    o = make_oracle(chain, N, L)
    ol = level_oracle(ob, o, Lc)
    return o, ol, ccol.drop_families(o, ol, Lc)


PARAMS = [pytest.param(c, id=case_id(c)) for c in CASES]


def _rows(cols, n):
    """columns -> n object arrays of residues"""
    return [np.array([int(c[i]) for c in cols], dtype=object) for i in range(n)]


# ---- the builders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARAMS)
def test_builders_deliver_their_claims(ob, case):
    """drop_limbs_coeff, one limb at a time: the residue dropped from a `final` column at step l is the planted r_l mod q_l and the
    result is y; a `kept` column shows its claimed state -- kept residues all 0 or all q_i - 1, limb l at its edge -- in front of
    step l"""
    o, ol, fam = case_families(case)
    qs, _ = ccol.moduli(o)
    L, Lc = case[2], case[3]
    assert fam.moduli == tuple(qs) and len(fam["final"]) == len(fam.claims["final"]) and len(fam["kept"]) == len(fam.claims["kept"])
    assert all(0 <= v < q for cols in fam.values() for c in cols for v, q in zip(c, qs))
    lvl_cols = [c for cols in ccol.q_families(ol).values() for c in cols]
    ys = [y for y, _ in fam.claims["final"]]
    QLc = ex.prod(qs[:Lc])
    assert {ex.crt(c, qs[:Lc]) for c in lvl_cols} | {0, 1, QLc - 1} == set(ys)     # every level column is behind some drop
    pats = ccol.drop_patterns(qs, Lc)
    assert all(p in [pat for _, pat in fam.claims["final"]] for p in pats)             # ... and every pattern in front of one
    half = {l: (qs[l] - 1) // 2 for l in range(Lc, L)}
    for v in (0, 1, -1):
        assert {l: v for l in half} in pats
    for sgn in (1, -1):
        assert {l: sgn * half[l] for l in half} in pats
        for l in half:
            assert {j: sgn * half[j] if j == l else 0 for j in half} in pats and {j: sgn if j == l else 0 for j in half} in pats
    cur = _rows(fam["final"], L)
    for l in range(L - 1, Lc - 1, -1):
        assert [int(v) for v in cur[l]] == [pat[l] % qs[l] for _, pat in fam.claims["final"]], "step %d" % l
        cur = drop_limbs_coeff(cur, qs[:l + 1], l)
    assert [ex.crt([int(cur[i][k]) for i in range(Lc)], qs[:Lc]) for k in range(len(ys))] == ys
    cur = _rows(fam["kept"], L)
    seen = set()
    for l in range(L - 1, Lc - 1, -1):
        for k, (cl, state, _) in enumerate(fam.claims["kept"]):
            if cl == l:
                assert tuple(int(cur[i][k]) for i in range(l + 1)) == state
                assert state[:l] in (tuple(0 for _ in range(l)), tuple(qs[i] - 1 for i in range(l)))
                seen.add((l, state[0] != 0, state[l]))
        cur = drop_limbs_coeff(cur, qs[:l + 1], l)
    assert seen == {(l, low, v) for l in range(Lc, L) for low in (False, True) for v in (0, half[l], half[l] + 1, qs[l] - 1)}


def test_undrop_is_the_inverse_of_the_drop(ob):
    """on random y and random centred r, a chain with a wide last limb: the drop returns y and meets r at every step"""
    q, _ = pc.q_last_wide(64, 4)
    qs = [int(v) for v in q]
    rng = np.random.default_rng(3)
    for l_from in (1, 2, 3):
        for _ in range(20):
            y = int.from_bytes(rng.bytes(32), "little") % ex.prod(qs[:l_from])
            rs = {l: int(rng.integers(-((qs[l] - 1) // 2), (qs[l] - 1) // 2 + 1)) for l in range(l_from, 4)}
            cur = _rows([ccol.undrop(y, l_from, qs, rs)], 4)
            for l in range(3, l_from - 1, -1):
                assert int(cur[l][0]) == rs[l] % qs[l]
                cur = drop_limbs_coeff(cur, qs[:l + 1], l)
            assert ex.crt([int(v[0]) for v in cur], qs[:l_from]) == y


# ---- the kernels' operand -------------------------------------------------------------------------------------------------------
def drop_off(ql, qi):
    """DevConsts::drop_off[l][i] as params.cpp computes it: the smallest multiple of q_i that is >= (q_l - 1)/2"""
    half = (ql - 1) // 2
    return (half + qi - 1) // qi * qi


def kernel_x(ci, v, ql, qi):
    """the word limb_drop_kernel / drop_limbs hand to the Shoup product, in whole integers (no wrap)"""
    off = drop_off(ql, qi)
    s = v > (ql >> 1)            # (u64)((int64_t)((ql >> 1) - v) >> 63)
    return ci - v + off + ((ql - off) if s else 0)


@pytest.mark.parametrize("case", PARAMS)
def test_kernel_operand_stays_in_its_contract(ob, case):
    """0 <= x < 2^63 (shoup63 takes a < 2^63) and x = c_i - r (mod q_i) at every step of every crafted column, x q_l^-1 mod q_i is the
    definition's residue, and the `kept` family reaches the four ends of x for every pair (l, i): the smallest and largest word of
    either branch.  (off is a multiple of q_i and x + off stays below 2^63 as well: a kernel that adds q_l instead of q_l - off on the
    negative branch computes the same bits, so no test can tell the two apart.)"""
    o, _, fam = case_families(case)
    qs, _ = ccol.moduli(o)
    L, Lc = case[2], case[3]
    cols = fam["final"] + fam["kept"]
    cur = _rows(cols, L)
    for l in range(L - 1, Lc - 1, -1):
        ql, half = qs[l], (qs[l] - 1) // 2
        nxt = drop_limbs_coeff(cur, qs[:l + 1], l)
        for i in range(l):
            qi, off = qs[i], drop_off(ql, qs[i])
            assert off % qi == 0 and half <= off < half + qi
            xs = set()
            for k in range(len(cols)):
                ci, v = int(cur[i][k]), int(cur[l][k])
                x = kernel_x(ci, v, ql, qi)
                assert 0 <= x < 1 << 63
                assert x + off < 1 << 63         # `s & q_l` for `s & (q_l - off)` is the same residue, in contract: not an error
                assert (x - (ci - ex.centered(v, ql))) % qi == 0
                assert x * pow(ql, -1, qi) % qi == int(nxt[i][k])
                xs.add(x)
            assert {off - half, qi - 1 + off, 1, qi - 1 + half} <= xs, "limb %d into %d" % (l, i)
        cur = nxt


# ---- what uniform columns do not see --------------------------------------------------------------------------------------------
def drop_model(c, q, keep, negative):
    """drop_limbs_coeff with the branch as a parameter: negative(v, q_l) says which residues count as negative"""
    c = [np.array(v, dtype=object) for v in c]
    q = [int(v) for v in q]
    for l in range(len(q) - 1, keep - 1, -1):
        v = c[l]
        r = np.where(negative(v, q[l]), v - q[l], v)
        for i in range(l):
            c[i] = (c[i] - r) * pow(q[l], -1, q[i]) % q[i]
    return c[:keep]


MODELS = {
    "definition": lambda v, ql: v > (ql - 1) // 2,
    ">= for >": lambda v, ql: v >= (ql - 1) // 2,          # (q_l - 1)/2 taken as negative
    "> half + 1": lambda v, ql: v > (ql - 1) // 2 + 1,     # (q_l + 1)/2 taken as positive
}
UNIFORM_COLUMNS = 2000


def _misses(qs, Lc, cols, model):
    want = drop_limbs_coeff(_rows(cols, len(qs)), qs, Lc)
    got = drop_model(_rows(cols, len(qs)), qs, Lc, MODELS[model])
    bad = np.zeros(len(cols), dtype=bool)
    for w, g in zip(want, got):
        bad |= (w != g).astype(bool)
    return int(bad.sum())


@pytest.mark.parametrize("case", PARAMS)
def test_wrong_models_pass_uniform_columns(ob, case):
    """a drop whose threshold is off by one -- either way -- equals the definition on 2000 uniform columns and differs from it on at
    least one `final` and one `kept` column: the families see what uniform inputs (probability about 2^-59 a column) do not"""
    o, _, fam = case_families(case)
    qs, _ = ccol.moduli(o)
    L, Lc = case[2], case[3]
    rng = np.random.default_rng(L * 8 + Lc)
    uni = ccol.cols_of(ccol.uniform_poly(qs, UNIFORM_COLUMNS, rng))
    assert _misses(qs, Lc, uni + fam["final"] + fam["kept"], "definition") == 0
    for model in (">= for >", "> half + 1"):
        u, f, k = (_misses(qs, Lc, cols, model) for cols in (uni, fam["final"], fam["kept"]))
        print("%s: model '%s' differs on %d of %d uniform, %d of %d final, %d of %d kept columns"
              % (case_id(case), model, u, len(uni), f, len(fam["final"]), k, len(fam["kept"])))
        assert u == 0 and f >= 1 and k >= 1


# ---- the chain with a wide last limb ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1024, 4096])
def test_q_last_wide_is_accepted(ob, N):
    """the oracle takes the parent chain and the level prefixes the GPU tests use; the dropped modulus is 2^14 times a kept one, so
    the drop's offset spans about 2^14 multiples of q_i; NAMED has not grown"""
    L = 3
    q, p = pc.q_last_wide(N, L)
    assert [int(v).bit_length() for v in q] == [45, 45, 60] and [int(v).bit_length() for v in p] == [55] * 4
    assert "q_last_wide" not in pc.NAMED and len(pc.NAMED) == 4
    o = ob.Oracle(N, L, T32, q, p)
    assert (o.q == q).all() and (o.p == p).all()
    for i in range(L - 1):
        assert drop_off(int(q[2]), int(q[i])) // int(q[i]) >= 1 << 13
    for Lc in (2, 1):
        ol = level_oracle(ob, o, Lc)
        assert (ol.q == q[:Lc]).all() and (ol.p == p[:Lc + 1]).all()
        x = ccol.tile(ccol.q_families(ol), N, np.random.default_rng(Lc))
        assert ol.expand_q_to_qp(x).shape == (2 * Lc + 1, N)


@pytest.mark.parametrize("case", PARAMS)
def test_level_prefixes_are_accepted(ob, case):
    """every chain used here, and the level prefix of every case, is a chain the oracle takes; the families fit the ring they are
    tiled into"""
    o, ol, fam = case_families(case)
    assert (ol.q == o.q[:case[3]]).all() and (ol.p == o.p[:case[3] + 1]).all()
    assert fam.count() + 2 <= (1024 if case in MOD_REDUCE else case[1]) // 2       # ccol.tile places every column
