"""Every transform route alone: one launch of launch_ntt / launch_ntt16 (+ Ntt16Digits) / launch_ntt_digits per child process, on the
crafted limbs of tests/transform_inputs.py, against the oracle's ntt / intt (tests/test_transform_inputs.py shows on the CPU that
the limbs are where claimed; tests/test_oracle_exact.py pins the oracle's transforms to exact evaluation).

The program is tests/lazy_inputs (csrc/build/lazy_inputs_check): it makes a handle, prints what the context decided and the route of
the call, and launches on files this test writes; every output lies between guard words and is pre-filled with FILL.  _run and
_lane are those of tests/test_gpu_lazy_inputs.py, and so is the list that stops both files after a status that is neither 0 nor 2,
or a time limit (the limbs of one launch here lie under different moduli, so the congruence check runs limb by limb: _check_limbs).

The route of every point is WRITTEN OUT here (ROUTE and PLAN below), not computed by the library's rule, and asserted from the
program's `route` / `plan` lines.  L = 2 unless a case says otherwise; mode cases have nb = 3 bins.  164 cases, 117 s on an MI355X.
A plain case transforms one limb per family of its direction (29 to 33 limbs: every `alt s`, `const`, `delta`, `max`, `near`,
`rand`) at the head of an array one limb longer: that last limb must come back as it went in.

Per case, with no skip and no tolerance: the output bit for bit where it is canonical (every unfolded inverse, every forward store
without lazy_out); congruent and below 8q behind lazy_out; below 4q per word, and the exact coefficients after the outer stage and
N^-1 in exact integers, behind a folded inverse; guards intact; every word a mode does not write still FILL or still the input (the
skipped limbs, slots 2, 3 and the P limbs of the copy array, the whole copy array where the route does not honour NttExtra, the limb
behind the last item); the copy equal to the lane-ordered X limbs bit for bit; with x_lane_in the same data as with the X limbs in
standard order, and the copy array as it was.

Input ranges.  Forward: anything below 8q (ct_bfly, bfly<false>: "a, b in [0, 8q)"; the radix-2 kernel and
the global stages: canonical).  Inverse through the register-blocked kernels: their load phases hand the words straight to
gs_bfly / bfly<true>, whose contract is "a, b in [0, 4q)" -- the range the TENSOR load phase produces for the same butterflies -- so
those cells also run on every representative below 4q; the radix-2 inverse and the global stages state canonical and get canonical.
"""
import functools

import numpy as np
import pytest

from tests import lazy_inputs as lz
from tests import transform_inputs as ti
from tests.test_gpu_lazy_inputs import FILL, _lane, _lane_rule, _oracle, _run, _stopped

pytestmark = pytest.mark.gpu
NB, L2 = 3, 2
B61, B50 = 1 << 61, 1 << 50

# (chain, N) -> {(inverse, sigma, fold): (kernel, s0, global_stages)}: DESIGN.md section 5a, cell by cell
_R2, _B32, _B16 = "radix2", "blocked32", "blocked16"
ROUTE = {
    ("default", 256): {(i, 0, 0): (_R2, 0, 0) for i in (0, 1)},
    (B61, 4096): {(i, 0, 0): (_R2, 0, 0) for i in (0, 1)},
    (B61, 32768): {(i, 0, 0): (_R2, 1, 1) for i in (0, 1)},
    (B61, 65536): {(i, 0, 0): (_R2, 2, 2) for i in (0, 1)},
    ("default", 4096): {(i, s, 0): (_B32, 0, 0) for i in (0, 1) for s in (0, 1)},
    ("default", 8192): {(1, 0, 0): (_B16, 0, 0), (1, 1, 0): (_B16, 0, 0), (0, 1, 0): (_B16, 0, 0), (0, 0, 0): (_B32, 0, 0)},
    ("default", 16384): {(1, 0, 1): (_B16, 1, 0), (1, 1, 1): (_B16, 1, 0), (0, 1, 1): (_B16, 1, 0), (0, 0, 1): (_B32, 1, 0),
                         (0, 0, 0): (_B32, 0, 0), (1, 0, 0): (_B32, 0, 0)},
    ("default", 32768): {(1, 0, 1): (_B16, 1, 0), (1, 1, 1): (_B16, 1, 0), (0, 1, 1): (_B16, 1, 0), (0, 0, 1): (_B32, 1, 0),
                         (0, 0, 0): (_B32, 1, 1), (1, 0, 0): (_B32, 1, 1)},
    ("default", 65536): {(i, s, 0): (_B32, 2, 2) for i in (0, 1) for s in (0, 1)},
}
ROUTE[("barrett_edges", 8192)] = ROUTE[(B50, 8192)] = ROUTE[("default", 8192)]
# what the context decides, per (chain, N): the plan line
PLAN = {
    ("default", 4096): dict(lane_order=1, fold=0, small_moduli=1, xq_reuse=1, x_direct=0, digits_with_d01=0, digit_lift_std=1, digit_lift_lane=1),
    ("default", 8192): dict(lane_order=1, fold=0, small_moduli=1, xq_reuse=1, x_direct=1, digits_with_d01=1, digit_lift_std=1, digit_lift_lane=0),
    ("barrett_edges", 8192): dict(lane_order=1, fold=0, small_moduli=1, xq_reuse=1, x_direct=1, digits_with_d01=1, digit_lift_std=1, digit_lift_lane=0),
    (B50, 8192): dict(lane_order=1, fold=0, small_moduli=0, xq_reuse=1, x_direct=0, digits_with_d01=0, digit_lift_std=1, digit_lift_lane=0),
    ("default", 16384): dict(lane_order=1, fold=1, small_moduli=1, xq_reuse=1, x_direct=1, digits_with_d01=1, digit_lift_std=1, digit_lift_lane=0),
    ("default", 32768): dict(lane_order=1, fold=1, small_moduli=1, xq_reuse=1, x_direct=1, digits_with_d01=1, digit_lift_std=0, digit_lift_lane=0),
    ("default", 65536): dict(lane_order=1, fold=0, small_moduli=1, xq_reuse=0, x_direct=0, digits_with_d01=0, digit_lift_std=0, digit_lift_lane=0),
    ("default", 256): dict(lane_order=0, fold=0), (B61, 4096): dict(lane_order=0, fold=0), (B61, 32768): dict(lane_order=0, fold=0),
    (B61, 65536): dict(lane_order=0, fold=0),
}


@functools.lru_cache(maxsize=None)
def _ctx(chain, N, L):
    """the oracle context of a point, kept for the whole file (the stage tables of tests/transform_inputs.py hang on it)"""
    return _oracle.__wrapped__(chain, N, L)


def _check_plan(chain, N, plan, key):
    kernel, s0, gs = ROUTE[(chain, N)][key]
    assert (plan["kernel"], plan["s0"], plan["global_stages"]) == (kernel, s0, gs), plan
    assert plan["extra"] == (1 if kernel != _R2 and gs == 0 else 0)
    for k, v in PLAN[(chain, N)].items():
        assert plan[k] == v, (k, plan)


def _mods_all(o):
    return [int(v) for v in o.moduli]   # Q, P, t


def _map(N):
    _, sl, kp, T = _lane_rule(N)
    return lz.lane_map(N, sl, T, kp)


# ---- inputs and references, computed once per shape -------------------------------------------------------------------------------------
def _reference(o, x, mis, inverse, fold):
    """the oracle's transform of x[n][N] (any representative; limb k under modulus mis[k]): EVALUATION in standard order, or the
    COEFFICIENTS.  A folded forward launch is handed what fold_store leaves: the oracle transforms the coefficients behind it"""
    mods = _mods_all(o)
    want = np.empty_like(x)
    for k, mi in enumerate(mis):
        c = x[k] % np.uint64(mods[mi])
        if inverse:
            want[k] = o.intt(mi, c)
        else:
            want[k] = o.ntt(mi, lz.unfold_store(c, *lz.fold_w(o, mi)) if fold else c)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=6)
def _crafted(chain, N, L, inverse, fold, n, mod_base, mod_count, start, lazy):
    """(x[n][N] in the order the first stage reads, the modulus of every limb, the reference).  lazy: every representative below
    lazy * q (tests/lazy_inputs.py) instead of the families"""
    o = _ctx(chain, N, L)
    mis = [mod_base + k % mod_count for k in range(n)]
    if lazy:
        mods = _mods_all(o)
        rng = np.random.default_rng(N + 7 * lazy + inverse)
        x = np.stack([lz.lazy_limb(mods[mi], lazy * mods[mi], N, rng, shift=3 * k)[0] for k, mi in enumerate(mis)])
    else:
        x, _ = ti.limbs(o, bool(inverse), n, mod_base, mod_count, start, first=1 if (fold and not inverse) else 0)
    x.setflags(write=False)
    return x, mis, _reference(o, x, mis, inverse, fold)


def _check_limbs(o, got, want, mis, inverse, sigma, fold, lazy_out, what, keep=None):
    """got[n][N] as the launch left it against want[n][N] (standard order); keep: limbs the launch must not have touched -> their input"""
    mods = _mods_all(o)
    m = _map(o.N) if sigma and not inverse else None
    for k, mi in enumerate(mis):
        q, g = mods[mi], got[k]
        if keep is not None and k in keep:
            assert (g == keep[k]).all(), "%s: limb %d was not to be touched" % (what, k)
            continue
        w = want[k] if m is None else want[k][m]
        if inverse and fold:
            assert (g < np.uint64(4 * q)).all(), "%s: limb %d leaves [0, 4q)" % (what, k)
            assert (lz.fold_load(g, *lz.fold_w(o, mi)) == w).all(), "%s: limb %d, after the outer stage and N^-1" % (what, k)
        elif lazy_out:
            assert (g < np.uint64(8 * q)).all(), "%s: limb %d leaves [0, 8q)" % (what, k)
            assert (g % np.uint64(q) == w).all(), "%s: limb %d (mod q)" % (what, k)
        else:
            bad = np.flatnonzero(g != w)
            assert not len(bad), "%s: limb %d (modulus %d): first of %d at position %d: %d for %d" % (what, k, mi, len(bad), bad[0], g[bad[0]], w[bad[0]])


def _plain(chain, N, inverse, sigma, fold, L=L2, mod_base=0, mod_count=None, slots=0, lazy=0, lazy_out=0, n=None, start=0):
    """one launch_ntt over n limbs and one limb behind them"""
    o = _ctx(chain, N, L)
    mod_count = mod_count or L
    n = n or len(ti.specs(N, bool(inverse), 1 if (fold and not inverse) else 0))
    x, mis, want = _crafted(chain, N, L, inverse, fold, n, mod_base, mod_count, start, lazy)
    mem = x[:, _map(N)] if (inverse and sigma) else x
    tail = np.arange(N, dtype=np.uint64)[None, :] + np.uint64(12345)
    opts = dict(nlimbs=n, data_limbs=n + 1, inverse=inverse, sigma=sigma, fold=fold, mod_base=mod_base, mod_count=mod_count, lazy_out=lazy_out)
    if slots:
        opts["slots"] = slots
    got, plan, _ = _run("ntt", o, {"data": np.concatenate([mem, tail])}, {"data": (n + 1, N)}, **opts)
    _check_plan(chain, N, plan, (inverse, sigma, fold))
    if sigma:
        _lane(o, plan, got)
    if slots:
        assert plan["transform_cus"] == (slots + 1) // 2
    what = "N=%d %s%s%s" % (N, "inverse" if inverse else "forward", " lane order" if sigma else "", " folded" if fold else "")
    _check_limbs(o, got["data"][:n], want, mis, inverse, sigma, fold, lazy_out, what)
    assert (got["data"][n] == tail[0]).all(), what + ": the limb behind the last item was written"
    return plan


# ---- every cell on the families ----------------------------------------------------------------------------------------------------------
CELLS = [(c, N) + key for (c, N), cells in ROUTE.items() for key in sorted(cells)]


def _cell_id(c):
    chain, N, inverse, sigma, fold = c
    return "%s-%d-%s-%s%s" % ({B61: "61bit", B50: "50bit"}.get(chain, chain), N, "inv" if inverse else "fwd", "lane" if sigma else "std", "-folded" if fold else "")


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_route_on_families(cell):
    """every cell of the route table: one limb per family, Q moduli, the whole grid"""
    chain, N, inverse, sigma, fold = cell
    _plain(chain, N, inverse, sigma, fold)


# one point per kernel instantiation: radix-2 (+ global stages), 32-coefficient <12> / <13> / <14> (one slice, folded slices, behind
# global stages), 16-coefficient <13> / <14>, each direction and order it is launched in
INSTANCES = [("default", 256, 0, 0, 0), ("default", 256, 1, 0, 0), (B61, 32768, 0, 0, 0), (B61, 32768, 1, 0, 0),
             ("default", 4096, 0, 0, 0), ("default", 4096, 0, 1, 0), ("default", 4096, 1, 0, 0), ("default", 4096, 1, 1, 0),
             ("default", 8192, 0, 0, 0), ("default", 16384, 0, 0, 1), ("default", 16384, 0, 0, 0), ("default", 16384, 1, 0, 0),
             ("default", 65536, 0, 1, 0), ("default", 65536, 1, 1, 0), ("default", 65536, 1, 0, 0),
             ("default", 8192, 1, 0, 0), ("default", 8192, 1, 1, 0), ("default", 8192, 0, 1, 0),
             ("default", 16384, 1, 0, 1), ("default", 16384, 0, 1, 1),
             ("default", 32768, 1, 0, 1), ("default", 32768, 1, 1, 1), ("default", 32768, 0, 1, 1), ("default", 32768, 0, 0, 1)]


@pytest.mark.parametrize("shape", ["slots1-qp", "slots3-p"])
@pytest.mark.parametrize("cell", INSTANCES, ids=_cell_id)
def test_route_persistent_loop_and_moduli(cell, shape):
    """the persistent loops with one workgroup slot (one CU: 1, 2 or 4 workgroups walk all items) and three (two CUs), on a QP-shaped
    call (mod_count = M) and on the P limbs alone (mod_base = L, mod_count = L + 1); the families start further on in their list"""
    chain, N, inverse, sigma, fold = cell
    if shape == "slots1-qp":
        _plain(chain, N, inverse, sigma, fold, slots=1, mod_base=0, mod_count=2 * L2 + 1, start=3)
    else:
        _plain(chain, N, inverse, sigma, fold, slots=3, mod_base=L2, mod_count=L2 + 1, start=11)


T_CELLS = [c for c in INSTANCES if not c[3] and not c[4]]   # the plaintext modulus is transformed in standard order, unfolded (client, encoder)


@pytest.mark.parametrize("cell", T_CELLS, ids=_cell_id)
def test_route_modulus_t(cell):
    """mod_base = M, mod_count = 1: t = 4296540161, far narrower than the chain (33 bits: 4q and 8q lie far below the words' top)"""
    chain, N, inverse, sigma, fold = cell
    _plain(chain, N, inverse, sigma, fold, mod_base=2 * L2 + 1, mod_count=1, slots=3, n=7, start=0)


# ---- lazy inputs -------------------------------------------------------------------------------------------------------------------------
LAZY_FWD = [("default", 8192, 0, 0, 0), ("default", 16384, 0, 0, 1), ("default", 16384, 0, 0, 0), ("default", 32768, 0, 1, 1),
            ("default", 32768, 0, 0, 1), ("default", 4096, 0, 0, 0)]
LAZY_INV = [c for c in CELLS if c[2] and ROUTE[c[:2]][c[2:]][0] != _R2 and c[0] == "default"] + [("barrett_edges", 8192, 1, 0, 0), (B50, 8192, 1, 1, 0)]


@pytest.mark.parametrize("cell", LAZY_FWD, ids=_cell_id)
def test_forward_routes_on_lazy_inputs(cell):
    """the forward cells tests/test_gpu_lazy_inputs.py does not launch, on every representative below 8q: the 32-coefficient kernel in
    standard order (one slice, two folded slices of 2^13 and of 2^14), the 2^14-slice instantiation of the 16-coefficient kernel.  (The
    routes with global stages take canonical words: ntt_global_stage says so.)"""
    chain, N, inverse, sigma, fold = cell
    _plain(chain, N, inverse, sigma, fold, lazy=8, n=6, lazy_out=sigma)


@pytest.mark.parametrize("cell", LAZY_INV, ids=_cell_id)
def test_inverse_routes_on_lazy_inputs(cell):
    """every inverse cell of the register-blocked kernels on every representative below 4q, the range of gs_bfly / bfly<true>"""
    chain, N, inverse, sigma, fold = cell
    _plain(chain, N, inverse, sigma, fold, lazy=4, n=6)


# ---- NttExtra: copy_out / x_lane_in ---------------------------------------------------------------------------------------------------
def _copy_case(chain, N, fold, K, x_lane_in=False, start=0, L=L2):
    """inverse, standard order in, over [nb][K][2][L] with copy_out [nb][4][M][N]"""
    o = _ctx(chain, N, L)
    M, n = o.M, NB * K * 2 * L
    x, mis, want = _crafted(chain, N, L, 1, fold, n, 0, L, start, 0)
    m = _map(N)
    is_x = [(k // (2 * L)) % K == 0 for k in range(n)]
    copy_want = np.full((NB, 4, M, N), FILL, dtype=np.uint64)
    for k in range(n):
        if is_x[k]:
            copy_want[k // (2 * L * K), (k // L) & 1, k % L] = x[k][m]
    inputs, opts = {"data": x}, dict(nlimbs=n, nb=NB, inverse=1, fold=fold, copy=1, copy_K=K)
    if x_lane_in:   # the X limbs are read from the copy array: their places in the data hold a pattern no residue equals
        data = x.copy()
        data[np.array(is_x)] = FILL
        inputs, opts["x_lane_in"] = {"data": data, "copy": copy_want}, 1
    got, plan, _ = _run("ntt", o, inputs, {"data": (n, N), "copy": (NB, 4, M, N)}, **opts)
    _check_plan(chain, N, plan, (1, 0, fold))
    what = "N=%d copy_K=%d%s" % (N, K, " x_lane_in" if x_lane_in else "")
    _check_limbs(o, got["data"], want, mis, 1, 0, fold, 0, what)
    if plan["extra"]:
        _lane(o, plan, got)
        bad = np.argwhere(got["copy"] != copy_want)
        assert not len(bad), "%s: copy array: first of %d at bin %d slot %d limb %d position %d" % ((what, len(bad)) + tuple(bad[0]))
    else:
        assert (got["copy"] == FILL).all(), what + ": the route does not honour NttExtra and the copy array was written"
    return plan


@pytest.mark.parametrize("K", [1, 2, 3])
def test_copy_32_coefficient_kernel(K):
    """N = 4096: ntt_fast_kernel<12, true, false> writes the X limbs of every bin, lane-ordered, into slots 0, 1 of the QP array"""
    _copy_case("default", 4096, 0, K, start=5 * K)


@pytest.mark.parametrize("chain,N,fold", [("default", 8192, 0), ("barrett_edges", 8192, 0), (B50, 8192, 0), ("default", 16384, 1), ("default", 32768, 1)],
                         ids=["8192", "8192-barrett_edges", "8192-50bit", "16384-folded", "32768-folded"])
@pytest.mark.parametrize("K", [1, 2])
def test_copy_16_coefficient_kernel(chain, N, fold, K):
    _copy_case(chain, N, fold, K, start=7 * K)


@pytest.mark.parametrize("chain,N,fold", [("default", 8192, 0), ("barrett_edges", 8192, 0), ("default", 16384, 1), ("default", 32768, 1)],
                         ids=["8192", "8192-barrett_edges", "16384-folded", "32768-folded"])
def test_x_lane_in(chain, N, fold):
    """F_X_LANE_IN: the same data as the copy case (same limbs, K = 2), the copy array read and left as it was"""
    _copy_case(chain, N, fold, 2, x_lane_in=True, start=14)


def test_copy_is_not_honoured_behind_global_stages():
    """N = 65536: NttRoute::extra() is false (xq_reuse off): a copy that is asked for all the same must leave the array alone"""
    plan = _copy_case("default", 65536, 0, 1, start=2)
    assert plan["extra"] == 0


# ---- NttExtra: skip_L --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy_out", [0, 1])
@pytest.mark.parametrize("chain,N", [("default", 4096), ("default", 8192), ("barrett_edges", 8192), (B50, 8192), ("default", 16384), ("default", 32768)],
                         ids=["4096", "8192", "8192-barrett_edges", "8192-50bit", "16384-folded", "32768-folded"])
def test_skip(chain, N, lazy_out):
    """forward, lane order, over [nb][4][M] without the Q limbs of slots 0, 1: those limbs come back as they went in"""
    fold = _lane_rule(N)[0]
    o = _ctx(chain, N, L2)
    M = o.M
    n = NB * 4 * M
    x, mis, want = _crafted(chain, N, L2, 0, fold, n, 0, M, 1, 0)
    keep = {k: x[k] for k in range(n) if (k // M) % 4 < 2 and k % M < L2}
    assert len(keep) == NB * 2 * L2
    got, plan, _ = _run("ntt", o, {"data": x}, {"data": (n, N)}, nlimbs=n - len(keep), nb=NB, sigma=1, fold=fold, skip=1, mod_count=M, lazy_out=lazy_out)
    _check_plan(chain, N, plan, (0, 1, fold))
    _lane(o, plan, got)
    _check_limbs(o, got["data"], want, mis, 0, 1, fold, lazy_out, "N=%d skip" % N, keep=keep)


# ---- key-switch digits -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _digits(chain, N, L):
    """(d2[nb][L][N], the standard-order transforms of its lifts [nb][L][L][N])"""
    o = _ctx(chain, N, L)
    d2 = ti.digit_source(o, NB)
    lifted = ti.lifted(o, d2)
    want = np.stack([np.stack([np.stack([o.ntt(j, lifted[b, i, j]) for j in range(L)]) for i in range(L)]) for b in range(NB)])
    return d2, want


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("chain,N", [("default", 8192), ("barrett_edges", 8192), ("default", 16384), ("default", 32768)],
                         ids=["8192", "8192-barrett_edges", "16384-folded", "32768-folded"])
def test_digits_ride_on_the_forward_launch(chain, N, L):
    """Ntt16Digits: nb L L digit items behind the 2 nb L limbs of d0, d1 (lazy_out, as run() launches them).  lift1 on residues 0,
    floor(q_i / 2), floor(q_i / 2) + 1, q_i - 1 in both members of a folded pair; the XCD transposition with blocks of 8 L 2^s0 items:
    L = 2 has nb L L = 12 < 16 digit limbs (the tail rule alone), L = 3 has 27 = one full block of 24 and a tail of 3.  The digits leave
    canonical whatever lazy_out says"""
    fold = _lane_rule(N)[0]
    o = _ctx(chain, N, L)
    n = NB * 2 * L
    x, mis, want = _crafted(chain, N, L, 0, fold, n, 0, L, 4, 0)
    d2, dig_want = _digits(chain, N, L)
    got, plan, _ = _run("ntt", o, {"data": x, "d2": d2}, {"data": (n, N), "dig": (NB, L, L, N)}, nlimbs=n, nb=NB, sigma=1, fold=fold, digits=1, lazy_out=1)
    assert plan["digits_with_d01"] == 1 and (plan["kernel"], plan["s0"], plan["global_stages"]) == (_B16, fold, 0)
    m = _lane(o, plan, got)
    _check_limbs(o, got["data"], want, mis, 0, 1, fold, 1, "N=%d d0, d1 beside the digits" % N)
    bad = np.argwhere(got["dig"] != dig_want[..., m])
    assert not len(bad), "first of %d: bin %d residue %d into modulus %d, lane position %d" % ((len(bad),) + tuple(bad[0]))


@pytest.mark.parametrize("chain,N,sigma", [("default", 4096, 0), ("default", 4096, 1), ("default", 8192, 0), ("barrett_edges", 8192, 0), (B50, 8192, 0),
                                           ("default", 16384, 0)],
                         ids=["4096-std", "4096-lane", "8192-std", "8192-barrett_edges-std", "8192-50bit-std", "16384-std"])
def test_ntt_digits(chain, N, sigma):
    """launch_ntt_digits: lift_digit in the load phase of ntt_fast_kernel<LOGN, false, SIGMA>, one slice per limb, L = 3"""
    L = 3
    o = _ctx(chain, N, L)
    d2, dig_want = _digits(chain, N, L)
    got, plan, _ = _run("ntt_digits", o, {"d2": d2}, {"dig": (NB, L, L, N)}, nb=NB, sigma=sigma)
    assert (plan["kernel"], plan["s0"], plan["global_stages"]) == (_B32, 0, 0) and plan["digit_lift_std"] == 1 and plan["digit_lift_lane"] == (N == 4096)
    want = dig_want[..., _lane(o, plan, got)] if sigma else dig_want
    bad = np.argwhere(got["dig"] != want)
    assert not len(bad), "first of %d: bin %d residue %d into modulus %d, position %d" % ((len(bad),) + tuple(bad[0]))


def test_what_a_plan_does_not_offer_is_refused():
    """status 2 and no launch: Ntt16Digits and x_lane_in on the 50-bit chain (no digits_with_d01, no x_direct: its lift and its stage A
    are not the column-accumulator ones), launch_ntt_digits in lane order beside a 16-coefficient lane order and on a ring above one
    slice, x_lane_in where the 32-coefficient kernel runs the inverse"""
    z = np.zeros(8, dtype=np.uint64)
    for chain, N, op, opts in [(B50, 8192, "ntt", dict(nlimbs=12, nb=NB, sigma=1, digits=1)),
                               (B50, 8192, "ntt", dict(nlimbs=12, nb=NB, inverse=1, copy=1, copy_K=1, x_lane_in=1)),
                               ("default", 8192, "ntt_digits", dict(nb=NB, sigma=1)),
                               ("default", 32768, "ntt_digits", dict(nb=NB, sigma=0)),
                               ("default", 4096, "ntt", dict(nlimbs=12, nb=NB, inverse=1, copy=1, copy_K=1, x_lane_in=1))]:
        with pytest.raises(AssertionError, match="status 2"):
            _run(op, _ctx(chain, N, L2), {"data": z, "d2": z, "copy": z}, {}, **opts)
    assert not _stopped
