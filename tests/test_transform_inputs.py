"""tests/transform_inputs.py on the CPU: every family is where it claims to be, in plain integers.

The GPU test (tests/test_gpu_transform_routes.py) hands these limbs to one transform launch each and compares with the oracle's
ntt / intt.  What it relies on is shown here without a GPU: the stage networks of the module are the oracle's transforms, stage by
stage; the fast arithmetic the arrays are crafted with equals Python's; `const` gives a = b on every first-stage inverse butterfly;
`max` doubles along the inverse's sum path across the 4q threshold and then sits 2^s units below 8q; `alt s` puts (0, q - 1) and
(q - 1, 0) on the butterflies that are s apart, in both directions; the folded forms are the same networks entered one stage late
(forward) or left one stage early (inverse).

One family was replaced while this file was written.  `alt s` as plain runs of 0 and q - 1 in the transform's INPUT meets its
condition only at the first stage of a direction: a stage in front turns the runs into sums and twiddle products
(test_plain_runs_do_not_reach_a_later_stage).  The family is therefore DEFINED by its condition -- the residues in front of the stage
with distance s are the runs -- and its input is carried back through the stages in front in exact arithmetic.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests import coeff_columns as ccol
from tests import lazy_inputs as lz
from tests import param_chains as pc
from tests import transform_inputs as ti
from tests.param_chains import T32

DEFAULT_PRIME = int(ob.default_moduli(16384, 4)[0][0])
EDGE_LOW, EDGE_HIGH = 576460752304439297, 1152921504606748673   # barrett_edges at N = 16384: the first prime above 2^59, the last below 2^60


def _oracle(chain, N, L=2):
    if chain == "default":
        return ob.Oracle(N, L, T32)
    q, p = pc.named_chain(N, L, chain)
    return ob.Oracle(N, L, T32, q, p)


def test_fast_products_equal_python():
    rng = np.random.default_rng(5)
    for q in (DEFAULT_PRIME, EDGE_LOW, EDGE_HIGH, (1 << 61) - 1, T32, 65537):
        edge = np.array([0, 1, 2, q - 1, q - 2, q // 2, q // 2 + 1, (1 << 32) % q, ((1 << 32) - 1) % q], dtype=np.uint64)
        a = np.concatenate([np.repeat(edge, len(edge)), rng.integers(0, q, 1 << 14, dtype=np.uint64), q - 1 - rng.integers(0, min(q, 1 << 20), 1 << 12, dtype=np.uint64)])
        b = np.concatenate([np.tile(edge, len(edge)), rng.integers(0, q, 1 << 14, dtype=np.uint64), q - 1 - rng.integers(0, min(q, 1 << 20), 1 << 12, dtype=np.uint64)])
        assert (ti.mulmod(a, b, q) == ti.mulmod(a, b, q, exact=True)).all()
        assert (lz.obj(ti.addmod(a, b, q)) == (lz.obj(a) + lz.obj(b)) % q).all()
        assert (lz.obj(ti.submod(a, b, q)) == (lz.obj(a) - lz.obj(b)) % q).all()


@pytest.mark.parametrize("chain", ["default", "barrett_edges"])
@pytest.mark.parametrize("N", [256, 4096])
def test_stage_networks_are_the_oracles_transforms(chain, N):
    """both networks, every modulus (Q, P and t), both arithmetics; a stage undone gives the stage's input back"""
    o = _oracle(chain, N)
    rng = np.random.default_rng(N)
    for mi in range(o.M + 1):
        x = rng.integers(0, int(o.moduli[mi]), N, dtype=np.uint64)
        for exact in (True, False):
            st = ti.Stages(o, mi, exact)
            assert (st.run(x, False) == o.ntt(mi, x)).all() and (st.run(x, True) == o.intt(mi, x)).all()
            for inverse in (False, True):
                for t in st.distances(inverse):
                    assert (st.stage(st.stage(x, t, inverse), t, inverse, back=True) == x).all()


def test_const_gives_equal_operands_to_the_first_inverse_stage():
    N = 4096
    o = _oracle("default", N)
    sp = ti.specs(N, True)
    seen = set()
    for c in ("q-1", "1", "half"):
        for k in range(6):
            st = ti._stages(o, k % 2)
            x = ti.limb(("const", c), st, True, k, None)
            assert (x < np.uint64(st.q)).all()
            assert (x[0::2] == x[1::2]).all()   # the first inverse stage pairs (2i, 2i + 1): a - b + 4q is 4q exactly
            for h in range(2):
                half = x[h * (N // 2):(h + 1) * (N // 2)]
                assert (half == half[0]).all()
                seen.add((c, k % 2, int(half[0])))
    assert len(seen) == 3 * 6 * 2   # a tag per (limb, half): a misplaced limb or half shows
    assert ("const", "q-1") in sp and ("max",) in sp


@pytest.mark.parametrize("q", [DEFAULT_PRIME, EDGE_LOW, EDGE_HIGH])
def test_max_walks_the_sum_path_across_4q(q):
    """all q - 1: the word at position 0 (and at every multiple of 2^s) is a pure sum, 2^s (q - 1) in front of stage s as long as no
    subtraction has fired.  Stages 0 and 1 leave 2q - 2 and 4q - 4 (four units below the threshold: the block must NOT fire); from
    stage 2 on the sum is 8q - 2^(s+1) -- the block fires at every stage, on every prime -- and what it leaves is 2^(s+1) below 4q"""
    logN = 16
    path = ti.max_sum_path(q, logN)
    assert [f for _, f in path] == [False, False] + [True] * (logN - 2)
    a = q - 1
    for s, (sm, fired) in enumerate(path):
        assert a % q == ((1 << s) * (q - 1)) % q and (s > 2 or a == (1 << s) * (q - 1))
        assert sm == 2 * a and sm < 8 * q
        assert sm == (2 * q - 2 if s == 0 else (4 * q if s == 1 else 8 * q) - (1 << (s + 1)))
        a = sm - 4 * q if fired else sm
        assert 0 <= a < 4 * q


@pytest.mark.parametrize("chain", ["default", "barrett_edges"])
def test_max_sum_path_is_the_networks_position_zero(chain):
    """the residues the exact network holds at the multiples of 2^s in front of inverse stage s are 2^s (q - 1) mod q"""
    N = 256
    o = _oracle(chain, N)
    for mi in range(2):
        st = ti.Stages(o, mi, exact=True)
        x = ti.limb(("max",), st, True, 0, None)
        for s, t in enumerate(st.distances(True)):
            y = st.run(x, True, until=t)
            assert (lz.obj(y[::t]) == ((1 << s) * (st.q - 1)) % st.q).all()


def _pairs(y, s):
    Y = np.asarray(y).reshape(-1, 2, s)
    return Y[:, 0, :].ravel(), Y[:, 1, :].ravel()


@pytest.mark.parametrize("chain", ["default", "barrett_edges"])
@pytest.mark.parametrize("inverse,N,first", [(False, 256, 0), (False, 4096, 0), (False, 4096, 1), (True, 256, 0), (True, 4096, 0)],
                         ids=["forward-256", "forward-4096", "forward-4096-folded", "inverse-256", "inverse-4096"])
def test_alt_puts_both_pairs_on_the_stage_with_distance_s(chain, inverse, N, first):
    """exact network: in front of the stage with distance s every butterfly holds (0, q - 1) or (q - 1, 0), and both occur (s = N/2:
    one per limb, over the two limbs).  first = 1: a folded forward launch, entered behind the outer stage (a folded inverse runs the
    same stages as an unfolded one, from the start)"""
    o = _oracle(chain, N)
    sp = [s for s in ti.specs(N, inverse, first) if s[0] == "alt"]
    want_s = sorted(1 << k for k in range(N.bit_length() - 1 - (0 if inverse else first)))
    assert sorted({s[1] for s in sp}) == want_s
    for mi in (0, 1):
        exact, fast = ti.Stages(o, mi, exact=True), ti._stages(o, mi)
        q = exact.q
        kinds = {}
        for k, spec in enumerate(sp):
            x = ti.limb(spec, fast, inverse, k, None, first)
            assert (x < np.uint64(q)).all()
            assert (x == ti.limb(spec, exact, inverse, k, None, first)).all()
            a, b = _pairs(exact.run(x, inverse, until=spec[1], first=first), spec[1])
            lo, hi = (a == 0) & (b == np.uint64(q - 1)), (a == np.uint64(q - 1)) & (b == 0)
            assert (lo | hi).all()
            kinds.setdefault(spec[1], set()).update(([0] if lo.any() else []) + ([1] if hi.any() else []))
        assert all(v == {0, 1} for v in kinds.values()), kinds


def test_plain_runs_do_not_reach_a_later_stage():
    """why `alt s` is carried back: runs of 0 and q - 1 in the INPUT give the pairs only to the first stage"""
    N = 256
    o = _oracle("default", N)
    st = ti.Stages(o, 0, exact=True)
    q = st.q
    for inverse in (False, True):
        ds = st.distances(inverse)
        a, b = _pairs(st.run(ti.alt_pattern(q, N, ds[0]), inverse, until=ds[0]), ds[0])
        assert (((a == 0) & (b == q - 1)) | ((a == q - 1) & (b == 0))).all()
        for s in ds[1:]:
            a, b = _pairs(st.run(ti.alt_pattern(q, N, s), inverse, until=s), s)
            assert not (((a == 0) & (b == q - 1)) | ((a == q - 1) & (b == 0))).any()


def test_families_of_a_launch():
    """every limb of a launch of up to len(specs) limbs takes another family; delta and near are where claimed; all canonical"""
    for N in (256, 8192):
        o = _oracle("default", N)
        for inverse in (False, True):
            n = len(ti.specs(N, inverse))
            assert n == 4 + 10 + 2 + (N.bit_length() - 1) + 1
            x, took = ti.limbs(o, inverse, n, 0, o.M)
            assert len(set(took)) == n
            for k, spec in enumerate(took):
                q = int(o.moduli[k % o.M])
                assert (x[k] < np.uint64(q)).all()
                if spec[0] == "delta":
                    assert np.count_nonzero(x[k]) == 1 and int(x[k][spec[2]]) == (q - 1 if spec[1] == "q-1" else 1)
                if spec[0] == "near":
                    assert len(set(x[k].tolist())) == N and (x[k] >= np.uint64(q - (1 << 24))).all()
            assert {s[2] for s in took if s[0] == "delta"} == {0, 1, N // 2 - 1, N // 2, N - 1}
            x2, took2 = ti.limbs(o, inverse, 5, 2, 3, start=7)
            assert took2 == [ti.specs(N, inverse)[(7 + k) % n] for k in range(5)]


@pytest.mark.parametrize("chain", ["default", "barrett_edges"])
def test_folded_forms_are_the_same_networks(chain):
    """a folded forward launch takes what fold_store leaves and runs the stages behind the outer one; a folded inverse launch leaves
    what is in front of the outer stage, and fold_load (outer stage and N^-1) turns any representative of it into the coefficients"""
    N = 4096
    o = _oracle(chain, N)
    rng = np.random.default_rng(3)
    for mi in range(o.M):
        st = ti.Stages(o, mi)
        q, w = lz.fold_w(o, mi)
        assert w == int(st.tw[1])
        y = rng.integers(0, q, N, dtype=np.uint64)
        assert (st.run(y, False, first=1) == o.ntt(mi, lz.unfold_store(y, q, w))).all()
        z = st.run(y, True, until=N // 2)
        lazy = z + np.uint64(q) * rng.integers(0, 3, N, dtype=np.uint64)   # anywhere in [0, 4q)
        assert (lz.fold_load(lazy, q, w) == o.intt(mi, y)).all()


@pytest.mark.parametrize("chain", ["default", "barrett_edges"])
def test_digit_sources_hold_the_lift_windows_in_both_halves(chain):
    N, L = 4096, 3
    o = _oracle(chain, N, L)
    qs = [int(v) for v in o.q]
    d2 = ti.digit_source(o, 2)
    assert d2.shape == (2, L, N)
    for b in range(2):
        for i, qi in enumerate(qs):
            assert (d2[b, i] < np.uint64(qi)).all()
            for half in (d2[b, i, :N // 2], d2[b, i, N // 2:]):
                have = set(half.tolist())
                assert {0, qi // 2, qi // 2 + 1, qi - 1} <= have
    lifted = ti.lifted(o, d2)
    for n in list(range(64)) + list(range(N // 2, N // 2 + 64)):
        for i, qi in enumerate(qs):
            for j, qj in enumerate(qs):
                assert int(lifted[1, i, j, n]) == ccol.lift_definition(int(d2[1, i, n]), qi, qj)
