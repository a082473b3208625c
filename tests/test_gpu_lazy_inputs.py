"""The kernels of the product chain at the ends of their lazy input ranges: one launch of one kernel on crafted arrays, against exact
integers (tests/lazy_inputs.py; tests/test_lazy_inputs.py shows on the CPU that the arrays are where claimed).

Inside run() a kernel's operands are made by the transforms: a caller controls their value mod q, never the representative.  Here
tests/lazy_inputs (csrc/build/lazy_inputs_check, a program of its own linked with the library's objects) makes a handle, takes its
constants, plan and lane-order map and calls one piehip::launch_* on files this test writes: [0, 8q) operands for the tensor product,
the own-limb term and the forward transforms, a d01 / d word at every multiple of q below 2^63 and at 2^63 - 1 beside digit and key
words whose 30-bit halves are full, [0, 4q) pairs with the outer stage pending for the folded consumers.

Each case is one child process with a time limit.  It asserts: output == reference (mod q) at every word; bit for bit where the
output is documented canonical; the documented range where it is lazy (< 8q behind lazy_out and fold_store, whose two words also
give back the first operand exactly: y0 + y1 = 2u + 4q, u < 4q; < 4q behind a folded inverse transform); guards and the places a
mode does not write untouched.  No skip and no tolerance: a shape the program refuses fails.  After a status that is neither 0 nor
2, or a time limit, no further case starts the program.

The kernels that reduce a variable x variable column sum outside stage A take the arithmetic kind as a template argument (modarith.h:
ArithKind; kernels.hpp: Arith) and are built at both column-accumulator kinds: barrett, the one-word Barrett block,
and fold, the folded block.  The program takes the kind from the plan or from fd= (fd=0: kind barrett, valid on every context with
column accumulators), so the default chain's inputs and expected outputs serve both.
Every such case names its kind and asserts it: plan["fold_moduli"] is the context's decision, "reduction" on the route line the
kind that ran (_kind_opts, _check_kind).  KIND_POINTS lists the (chain, N, L) they use: tests/test_reduction_kinds.py checks on the
CPU that each chain selects the kind claimed here.

launch_digits with `fold` applies the outer stage on its STORE side only: it lifts canonical coefficients (the centred lift is
defined on the residue, and scale-and-round hands component 2 over canonical), so its case feeds it every value canonical and
checks the fold_store side.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import lazy_inputs as lz
from tests import param_chains as pc
from tests.param_chains import T32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
EXE = os.path.join(CSRC, "build", "lazy_inputs_check")
FILL = np.uint64(lz.FILL)
_stopped = []   # why no further case may start the program: after a fault or a hang nothing more runs on the GPU
_built = []


# ---- the program -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _oracle(chain, N, L):
    from oracle import binding as ob
    if chain == "default":
        return ob.Oracle(N, L, T32)
    q, p = pc.uniform_chain(N, L, chain) if isinstance(chain, int) else pc.chain_by_name(N, L, chain)
    return ob.Oracle(N, L, T32, q, p)


# the kind the plan of each chain of the two-kind cases selects (asserted from the plan line)
PLAN_KIND = {"default": "fold", "fold_edge": "fold", "barrett_edges": "barrett"}


def _kind_opts(chain, kind):
    """the program's option for a case of `kind` on `chain`: none where the plan selects that kind itself, fd=0 for the Barrett
    kernels on a chain whose plan folds"""
    assert kind in ("barrett", "fold") and (kind == PLAN_KIND[chain] or kind == "barrett")
    return {} if kind == PLAN_KIND[chain] else {"fd": 0}


def _kind_id(chain, kind, what):
    """the id of a two-kind case: the plan's kind on the default chain keeps the id the case had when there was one kind; the
    Barrett kernels on the default chain add -barrett, another chain adds its name (its plan's kind: PLAN_KIND)"""
    return what if (chain, kind) == ("default", "fold") else "%s-%s" % (what, "barrett" if chain == "default" else chain)


def _check_kind(plan, chain, kind):
    assert plan["small_moduli"] == 1 and plan["fold_moduli"] == (PLAN_KIND[chain] == "fold"), "the plan's kind on %s" % chain
    assert plan["reduction"] == kind, "the kind that ran"


def _mods(o):
    return [int(v) for v in o.q], [int(v) for v in o.p]


def _run(op, o, inputs, outs, **opts):
    """one child process: `inputs` name -> array go to in_<name>.u64, `outs` name -> shape come back from between their guards.
    Returns (arrays by name -- with "sigma_inv", the handle's lane-order map --, the plan's fields, the program's output)"""
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    if not _built:
        subprocess.check_call(["make", "-j8", "-C", CSRC, "build/lazy_inputs_check"], stdout=subprocess.DEVNULL)
        assert os.path.exists(EXE), "csrc/Makefile did not build " + EXE
        _built.append(True)
    qs, ps = _mods(o)
    with tempfile.TemporaryDirectory(prefix="lazy_inputs_") as tmp:
        for name, arr in inputs.items():
            np.ascontiguousarray(arr, dtype=np.uint64).tofile(os.path.join(tmp, "in_%s.u64" % name))
        cmd = [EXE, op, tmp, str(o.N), str(o.L), str(o.t)] + [str(v) for v in qs + ps] + ["%s=%d" % kv for kv in sorted(opts.items())]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
        except subprocess.TimeoutExpired:
            _stopped.append("lazy_inputs_check %s ran into its time limit" % op)
            raise
        if r.returncode not in (0, 2):
            _stopped.append("lazy_inputs_check %s ended with status %d" % (op, r.returncode))
        assert r.returncode == 0, "status %d\n%s" % (r.returncode, r.stdout[-4000:])
        assert "lazy_inputs_check %s ok" % op in r.stdout
        got = {}
        for name, shape in list(outs.items()) + [("sigma_inv", None)]:
            raw = np.fromfile(os.path.join(tmp, "out_%s.u64" % name), dtype=np.uint64)
            if shape is None:
                got[name] = raw.astype(np.int64)
                continue
            words = int(np.prod(shape))
            assert raw.size == words + 2 * lz.GUARD
            assert (raw[:lz.GUARD] == FILL).all() and (raw[-lz.GUARD:] == FILL).all(), "%s: a guard word was written" % name
            got[name] = raw[lz.GUARD:-lz.GUARD].reshape(shape)
    plan = {}
    for line in r.stdout.splitlines():
        if line.startswith("plan ") or line.startswith("route "):
            plan.update((k, int(v) if v.isdigit() else v) for k, v in (f.split("=") for f in line.split()[1:]))
    return got, plan, r.stdout


def _lane_rule(N):
    """(fold, slice length, kp, T) of the lane order of a ring of N >= 4096 coefficients, written out from the launchers' rule: the
    32-coefficient kernel's at 2^12 (one slice) and 2^16 (four, behind two global stages), the 16-coefficient kernel's between, as two
    folded slices from 2^14 on"""
    fold = 1 if N in (16384, 32768) else 0
    sl = N // 2 if fold else (N // 4 if N == 65536 else N)
    kp, T = (16, sl // 32) if N in (4096, 65536) else (8, sl // 16)
    return fold, sl, kp, T


def _lane(o, plan, got):
    """the lane-order map of a context whose plan has one, written out from the launchers' rule and compared with the handle's"""
    N = o.N
    fold, sl, want_kp, want_T = _lane_rule(N)
    assert plan["lane_order"] == 1 and plan["fold"] == fold and (plan["lane_kp"], plan["lane_T"]) == (want_kp, want_T)
    m = lz.lane_map(N, sl, want_T, want_kp)
    assert (got["sigma_inv"] == m).all()
    return m


def _congruent(got, want, mods, B_of, what):
    """got[..][len(mods)][N] == want (mod m) and got < B_of(m), limb by limb"""
    for a, m in enumerate(mods):
        g = got[..., a, :]
        assert (g < np.uint64(B_of(m))).all(), "%s: limb %d leaves its range" % (what, a)
        assert (g % np.uint64(m) == want[..., a, :]).all(), "%s: limb %d" % (what, a)


def _check_fold_store(o, got, want, first, what, canonical_u):
    """got[n][N]: fold_store outputs of the coefficients want[n][N], limb i under modulus first + i: both words below 8q, the
    coefficients behind them, and the first operand u = (y0 + y1 - 4q) / 2 itself -- below 4q, equal to want where it is canonical"""
    H = o.N // 2
    for i in range(got.shape[0]):
        q, w = lz.fold_w(o, first + i)
        assert (got[i] < np.uint64(8 * q)).all(), "%s: limb %d leaves [0, 8q)" % (what, i)
        assert (lz.unfold_store(got[i], q, w) == want[i]).all(), "%s: limb %d" % (what, i)
        s = lz.obj(got[i, :H]) + lz.obj(got[i, H:]) - 4 * q
        assert (s % 2 == 0).all() and (s >= 0).all() and (s < 8 * q).all(), "%s: limb %d: y0 + y1 is not 2u + 4q with u in [0, 4q)" % (what, i)
        t = lz.obj(got[i, :H]) - s // 2
        assert (t >= 0).all() and (t < 4 * q).all(), "%s: limb %d: the product v psi^(N/2) leaves [0, 4q)" % (what, i)
        if canonical_u:
            assert (lz.u64(s // 2) == want[i, :H]).all(), "%s: limb %d: u is not canonical" % (what, i)


# ---- launch_relin_mac ----------------------------------------------------------------------------------------------------------------
class _MacCase:
    """the operands of one (chain, N, L) for five rows, two keys and five masks, and the rows' sums before the mask as they are asked for"""
    NB, G = 5, 2

    def __init__(self, chain, N, L):
        self.o = o = _oracle(chain, N, L)
        self.qs, self.ps = _mods(o)
        rng = np.random.default_rng(N + 11 * L)
        if chain == 1 << 61:   # every word q - 1
            top = lambda shape: np.broadcast_to(np.array(self.qs, dtype=np.uint64)[:, None] - np.uint64(1), tuple(shape) + (L, N)).copy()  # noqa: E731
            self.ops = {"d01": top((self.NB, 2)), "dig": top((self.NB, L)), "key": top((self.G, L, 2)), "mask": top((self.NB,)), "eqp": None}
        else:
            self.ops = lz.mac_operands(self.qs, self.ps, N, self.NB, self.G, self.NB, rng)
        self.cs = lz.own_limb_consts(self.qs, self.ps, o.t)
        self._rows = {}

    def row(self, r, key, eq):
        if (r, key, eq) not in self._rows:
            p = self.ops
            self._rows[(r, key, eq)] = lz.ref_mac_row(p["d01"][r], p["dig"][r], p["key"][key], self.qs, p["eqp"][r] if eq else None, self.cs)
        return self._rows[(r, key, eq)]


@functools.lru_cache(maxsize=4)
def _mac_case(chain, N, L):
    return _MacCase(chain, N, L)


def _mac(chain, N, L, kp, nb, eq, mask, mask_div=1, key_group=1):
    c = _mac_case(chain, N, L)
    o, p = c.o, c.ops
    LN = L * N
    nmask = (nb + mask_div - 1) // mask_div
    inputs = {"d01": p["d01"][:nb], "dig": p["dig"][:nb]}
    opts = {"nb": nb, "kp": kp, "eq": eq, "mask": mask, "mask_div": mask_div, "key_group": key_group}
    if key_group > 1:   # the keys a stride apart, poison between them
        stride = 2 * L * LN + 2 * N
        gap = np.full(2 * N, FILL, dtype=np.uint64)
        inputs["key"] = np.concatenate([p["key"][0].ravel(), gap, p["key"][1].ravel()])
        opts["key_stride"] = stride
    else:
        inputs["key"] = p["key"][0]
    if eq:
        inputs["eqp"] = p["eqp"][:nb]
    if mask:
        inputs["mask"] = p["mask"][:nmask]
    got, plan, _ = _run("relin_mac", o, inputs, {"out": (nb, 2, L, N)}, **opts)
    want = np.stack([c.row(r, r % key_group, eq) for r in range(nb)])
    if mask:
        want = np.stack([lz.mul_mask(want[r], p["mask"][r // mask_div], c.qs) for r in range(nb)])
    out = got["out"]
    if kp:   # position n of the lane order leaves at its standard position
        out = out[..., _lane(o, plan, got)]
    bad = np.argwhere(out != want)
    assert not len(bad), "first of %d: row %d component %d limb %d lane position %d" % ((len(bad),) + tuple(bad[0]))
    return plan


MAC_POINTS = [(4096, 1), (4096, 0), (8192, 1)]   # (N, out_map): the LDS tile with KP = 16, with KP = 8; no out_map (KP = 0)


@pytest.mark.parametrize("mask,mask_div", [(0, 1), (1, 1), (1, 3)], ids=["nomask", "mask", "maskdiv3"])
@pytest.mark.parametrize("eq", [0, 1])
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("L", [7, 2])
@pytest.mark.parametrize("N,kp", MAC_POINTS, ids=["4096-kp16", "4096-kp0", "8192-kp8"])
@pytest.mark.parametrize("chain", ["default", "barrett_edges"])
def test_relin_mac_column_accumulators(chain, N, kp, L, nb, eq, mask, mask_div):
    """relin_mac_kernel<true, KP, RPT, EQ>: nb = 1 one row per thread, nb = 3 two (the last block without a second row).  Column 0 of
    the positions n = 0 (mod 64) holds L products of full low halves, 2^63 - 1 and the own-limb term's low half -- within 2^60 of
    (L + 8) 2^60 + 2^30 at L = 7; barrett_edges: mu = floor(2^123 / q_0) near 2^64"""
    plan = _mac(chain, N, L, kp, nb, eq, mask, mask_div)
    assert plan["small_moduli"] == 1


@pytest.mark.parametrize("L", [7, 2])
@pytest.mark.parametrize("N,kp", MAC_POINTS, ids=["4096-kp16", "4096-kp0", "8192-kp8"])
def test_relin_mac_key_group(N, kp, L):
    """key_group = 2 with a key_stride: row r takes key r % 2; five rows -- rows (0, 2), (1, 3) share a thread, row 4 has no second row --
    and mask_div = 3 (masks 0 0 0 1 1)"""
    plan = _mac("default", N, L, kp, 5, 1, 1, mask_div=3, key_group=2)
    assert plan["small_moduli"] == 1


@pytest.mark.parametrize("nb", [1, 3])
def test_relin_mac_128_bit_path_at_61_bits(nb):
    """relin_mac_kernel<false, 0>: N = 4096, L = 7, every digit, key, d01 and mask word q - 1 -- 7 (q - 1)^2 + q - 1 near 2^125"""
    plan = _mac(1 << 61, 4096, 7, 0, nb, 0, 1)
    assert plan["small_moduli"] == 0 and plan["lane_order"] == 0


@pytest.mark.parametrize("kp", [1, 0], ids=["kp16", "kp0"])
@pytest.mark.parametrize("mask", [0, 1])
def test_relin_mac_128_bit_path_at_50_bits(kp, mask):
    """relin_mac_kernel<false, KP>: a chain with a lane order and no column accumulators; d01 up to 2^63 - 1, 2^13 multiples of q"""
    plan = _mac(1 << 50, 4096, 7, kp, 3, 0, mask)
    assert plan["small_moduli"] == 0 and plan["lane_order"] == 1


def test_a_shape_the_launcher_refuses_is_status_2():
    """the own-limb term off the column-accumulator path, a folded launch on a ring that is not folded, an input file of another size,
    the folded reduction on a context whose moduli do not take it: the program says so with status 2 and launches nothing (every case of this file fails on such a status)"""
    for chain, op, inputs, opts in [(1 << 61, "relin_mac", {}, {"eq": 1}), ("default", "digits", {}, {"fold": 1}),
                                    ("default", "tensor", {"e": np.zeros(8, dtype=np.uint64)}, {"nb": 1}),
                                    ("barrett_edges", "scale_round", {}, {"fd": 1}), (1 << 50, "expand_both", {}, {"fd": 1})]:
        with pytest.raises(AssertionError, match="status 2"):
            _run(op, _oracle(chain, 4096, 2), inputs, {}, **opts)
    assert not _stopped


# ---- launch_tensor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,mad", [("default", 1), ("barrett_edges", 1), (1 << 50, 0)], ids=["default", "barrett_edges", "below2^50"])
def test_tensor(chain, mad):
    """tensor_kernel<MAD> (two conditional subtractions, column accumulators) and the generic form on a chain with a lane order and no
    column accumulators: all four operands over [0, 8q) at once; the result is canonical"""
    N, L, nb = 4096, 3, 2
    o = _oracle(chain, N, L)
    qs, ps = _mods(o)
    e = lz.lazy_array(qs + ps, lambda q: 8 * q, (nb, 4), N, np.random.default_rng(N + L))
    got, plan, _ = _run("tensor", o, {"e": e}, {"d": (nb, 3, o.M, N)}, nb=nb)
    assert plan["small_moduli"] == mad and plan["lane_order"] == 1
    bad = np.argwhere(got["d"] != lz.ref_tensor(e, qs + ps))
    assert not len(bad), "first of %d: row %d component %d limb %d position %d" % ((len(bad),) + tuple(bad[0]))


# ---- launch_ntt16_tensor ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _fused_tensor_case(chain, N):
    """e[nb][4][M][N] over [0, 8q) in lane order and the COEFFICIENT form of its tensor product, d[nb][3][M][N]"""
    L, nb = 2, 2
    o = _oracle(chain, N, L)
    qs, ps = _mods(o)
    e = lz.lazy_array(qs + ps, lambda q: 8 * q, (nb, 4), N, np.random.default_rng(N + 3))
    sl = N // 2 if N == 16384 else N
    m = lz.lane_map(N, sl, sl // 16, 8)
    t = lz.ref_tensor(e, qs + ps)
    std = np.empty_like(t)
    std[..., m] = t
    d = np.stack([np.stack([np.stack([o.intt(a, std[r, c, a]) for a in range(o.M)]) for c in range(3)]) for r in range(nb)])
    return o, e, d


# (chain, kind, mode): both kinds on the default chain in every mode; d just under the selection bound, and the edges of the one-word
# Barrett (mu near 2^64 and near 2^63) on a chain whose plan selects the Barrett kind itself, with every limb written
TENSOR_CASES = ([("default", kind, mode) for kind in ("barrett", "fold") for mode in ("all", "eval_q_L", "eval_q_d2")]
                + [("fold_edge", "fold", "all"), ("barrett_edges", "barrett", "all")])


@pytest.mark.parametrize("chain,kind,mode", TENSOR_CASES, ids=[_kind_id(c, k, m) for c, k, m in TENSOR_CASES])
@pytest.mark.parametrize("N", [8192, 16384])
def test_ntt16_tensor(N, chain, kind, mode):
    """the TENSOR load phase of ntt16_kernel.h (tensor_load) -- the TENSOR instantiation of ntt16_kernel_t at kind barrett and at kind
    fold --: N = 8192 one slice per limb (canonical coefficients out), N = 16384 folded (pairs in [0, 4q),
    compared after the outer stage).  eval_q_L = L leaves out the Q limbs of d0, d1, eval_q_d2 those of d2 as well: their places
    keep the fill pattern"""
    o, e, d = _fused_tensor_case(chain, N)
    L, M, nb = o.L, o.M, e.shape[0]
    qs, ps = _mods(o)
    opts = {"all": {}, "eval_q_L": {"eval_q_L": L}, "eval_q_d2": {"eval_q_L": L, "eval_q_d2": 1}}[mode]
    opts.update(_kind_opts(chain, kind))
    got, plan, _ = _run("ntt16_tensor", o, {"e": e}, {"d": (nb, 3, M, N)}, nb=nb, **opts)
    _check_kind(plan, chain, kind)
    assert plan["fused_tensor"] == 1 and plan["fold"] == (N == 16384)
    _lane(o, plan, got)
    out = got["d"]
    for c in range(3):
        skipped = L if (mode != "all" and c < 2) or (mode == "eval_q_d2" and c == 2) else 0
        assert (out[:, c, :skipped] == FILL).all(), "component %d: a Q limb this mode leaves out was written" % c
        for r in range(nb):
            for a in range(skipped, M):
                q = (qs + ps)[a]
                if plan["fold"]:
                    assert (out[r, c, a] < np.uint64(4 * q)).all(), "row %d component %d limb %d leaves [0, 4q)" % (r, c, a)
                    assert (lz.fold_load(out[r, c, a], *lz.fold_w(o, a)) == d[r, c, a]).all(), "row %d component %d limb %d" % (r, c, a)
                else:
                    assert (out[r, c, a] == d[r, c, a]).all(), "row %d component %d limb %d" % (r, c, a)


# ---- launch_deg2_finish ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_div", [1, 3])
@pytest.mark.parametrize("L", [2, 7])
def test_deg2_finish(L, mask_div):
    """deg2_finish_kernel<8> at N = 8192, four rows: d over every multiple of q below 2^63 and 2^63 - 1 itself, the QP operands over
    [0, 8q); the rows leave canonical, in standard order"""
    N, nb = 8192, 4
    o = _oracle("default", N, L)
    qs, ps = _mods(o)
    nmask = (nb + mask_div - 1) // mask_div
    p = lz.mac_operands(qs, ps, N, nb, 1, nmask, np.random.default_rng(N + L + mask_div), comps=3)
    got, plan, _ = _run("deg2_finish", o, {"d": p["d01"], "eqp": p["eqp"], "mask": p["mask"]}, {"out": (nb, 3, L, N)}, nb=nb, mask_div=mask_div)
    assert plan["result_eval_q"] == 1
    cs = lz.own_limb_consts(qs, ps, o.t)
    want = np.stack([lz.mul_mask(lz.ref_deg2_row(p["d01"][r], p["eqp"][r], qs, cs), p["mask"][r // mask_div], qs) for r in range(nb)])
    bad = np.argwhere(got["out"][..., _lane(o, plan, got)] != want)
    assert not len(bad), "first of %d: row %d component %d limb %d lane position %d" % ((len(bad),) + tuple(bad[0]))


# ---- fold_load consumers at N = 16384 ------------------------------------------------------------------------------------------------
SR_MODES = {"fold": {}, "fold_comp2": {"fold_comp2": 1}, "p_only01": {"p_only01": 1},
            "p_only012": {"fold_comp2": 1, "p_only01": 1, "p_only2": 1}}


# (chain, kind, L, mode).  L = 2 and 7 (the 128-bit fallback) in every mode, L = 5 (the last lazy output) and L = 6 (the 124-bit form
# of the reduction) in the modes fold and p_only01; both kinds on the default chain, and the folded kind with every d just under
# the selection bound at L = 2 and L = 6
SR_LM = [(L, m) for L in (2, 7) for m in sorted(SR_MODES)] + [(L, m) for L in (5, 6) for m in ("fold", "p_only01")]
SR_CASES = ([("default", kind, L, m) for kind in ("barrett", "fold") for L, m in SR_LM]
            + [("fold_edge", "fold", L, m) for L, m in SR_LM if L in (2, 6)])


@functools.lru_cache(maxsize=None)
def _scale_round_case(chain, L, p01, p2):
    """(o, d, want): d[1][3][M][N] over [0, 4q) with the outer stage pending, poison in the Q limbs a P-only component does not
    read, and the three components scaled and rounded by the oracle.  Shared by the kinds and by the modes that read the same limbs"""
    N = 16384
    o = _oracle(chain, N, L)
    qs, ps = _mods(o)
    d = lz.lazy_array(qs + ps, lambda q: 4 * q, (1, 3), N, np.random.default_rng(N + L))
    want = []
    for c, p_only in enumerate((p01, p01, p2)):
        x = lz.fold_load_poly(o, d[0, c])
        if p_only:
            d[0, c, :L] = FILL
            x[:L] = 0   # the own-limb term is the only place a Q limb enters (tests/test_lazy_inputs.py)
        want.append(o.scale_round_tp(x))
    d.setflags(write=False)
    return o, d, want


@pytest.mark.parametrize("chain,kind,L,mode", SR_CASES, ids=[_kind_id(c, k, "%d-%s" % (L, m)) for c, k, L, m in SR_CASES])
def test_scale_round_folded(chain, kind, L, mode):
    """scale_round_kernel<true, L, kind, P01, P2> at kind barrett and at kind fold.  d[3][M][N] over
    [0, 4q) with the outer stage pending; the Q limbs a P-only component does not read hold a poison pattern.  Components 0, 1 (and
    2 with fold_comp2) leave through fold_store -- their first operand in [0, 4q) (lz: L <= 5, no fold_comp2), canonical otherwise
    --, component 2 canonical without it.  L = 6: colacc_red<FD, true>, the 124-bit form of either block; L = 7: reduce128 under
    both kinds"""
    N = 16384
    opts = SR_MODES[mode]
    o, d, want = _scale_round_case(chain, L, bool(opts.get("p_only01")), bool(opts.get("p_only2")))
    got, plan, _ = _run("scale_round", o, {"d": d}, {"out01": (1, 2, L, N), "out2": (1, L, N)}, nb=1, fold=1, **opts, **_kind_opts(chain, kind))
    _check_kind(plan, chain, kind)
    assert plan["fold"] == 1
    lazy = L <= 5 and not opts.get("fold_comp2")
    for c in range(2):
        _check_fold_store(o, got["out01"][0, c], want[c], 0, "component %d" % c, canonical_u=not lazy)
    if opts.get("fold_comp2"):
        _check_fold_store(o, got["out2"][0], want[2], 0, "component 2", canonical_u=True)
    else:
        assert (got["out2"][0] == want[2]).all(), "component 2"


# (chain, kind, L): L = 6 is the last crt_out on column accumulators (NS = 7 sums); at L = 7 the P -> Q lift of scale_pq takes the 128-bit
# path while the Q -> P sums stay on accumulators
EB_CASES = [("default", kind, L) for kind in ("barrett", "fold") for L in (2, 6, 7)] + [("fold_edge", "fold", L) for L in (2, 6)]


@functools.lru_cache(maxsize=None)
def _expand_both_case(chain, L):
    """(o, x, y, wx, wy): X and Y [1][2][L][N] over [0, 4q) with the outer stage pending and their conversions by the oracle,
    shared by the kinds"""
    N = 16384
    o = _oracle(chain, N, L)
    qs, ps = _mods(o)
    rng = np.random.default_rng(N + L + 1)
    x, y = (lz.lazy_array(qs, lambda q: 4 * q, (1, 2), N, rng) for _ in range(2))
    wx = [o.expand_q_to_qp(lz.fold_load_poly(o, x[0, c])) for c in range(2)]
    wy = [o.scale_pq_expand(lz.fold_load_poly(o, y[0, c])) for c in range(2)]
    for v in [x, y] + wx + wy:
        v.setflags(write=False)
    return o, x, y, wx, wy


@pytest.mark.parametrize("skip_q", [1])   # (a folded context's X always has its Q limbs in place: the only folded form built)
@pytest.mark.parametrize("chain,kind,L", EB_CASES, ids=[_kind_id(c, k, "%d" % L) for c, k, L in EB_CASES])
def test_expand_both_folded(chain, kind, L, skip_q):
    """expand_both_kernel<true, L, kind, true> at kind barrett and at kind fold.  X and Y over [0, 4q)
    with the outer stage pending; every output limb leaves through fold_store; skip_q: the Q limbs of X's slots keep the fill
    pattern"""
    N = 16384
    o, x, y, wx, wy = _expand_both_case(chain, L)
    got, plan, _ = _run("expand_both", o, {"x": x, "y": y}, {"out": (1, 4, o.M, N)}, n_outer=1, fold=1, skip_q=skip_q, **_kind_opts(chain, kind))
    _check_kind(plan, chain, kind)
    assert plan["fold"] == 1
    for c in range(2):
        first = L if skip_q else 0
        assert (got["out"][0, c, :first] == FILL).all(), "X%d: a Q limb was written" % c
        _check_fold_store(o, got["out"][0, c, first:], wx[c][first:], first, "X%d" % c, canonical_u=False)
        _check_fold_store(o, got["out"][0, 2 + c], wy[c], 0, "Y%d" % c, canonical_u=False)


def test_expand_both_folded_without_skip_q_is_refused():
    """fold = 1 with skip_q = 0 is no combination of the library's (plan.fold implies plan.xq_reuse, and every caller passes
    x.q_ready = plan.xq_reuse): launch_expand_pair returns false and launches nothing, and the program reports that with status 2"""
    N, L = 16384, 1
    o = _oracle("default", N, L)
    z = np.zeros((1, 2, L, N), dtype=np.uint64)
    with pytest.raises(AssertionError, match=r"(?s)status 2\b.*refused: expand_both: a combination the launcher is not built for"):
        _run("expand_both", o, {"x": z, "y": z}, {"out": (1, 4, o.M, N)}, n_outer=1, fold=1, skip_q=0)
    assert not _stopped


# every (chain, N, L) of the cases above that name a kind, with the kind its plan selects (tests/test_reduction_kinds.py)
KIND_POINTS = sorted({(c, 16384, L, PLAN_KIND[c]) for c, _, L, _ in SR_CASES} | {(c, 16384, L, PLAN_KIND[c]) for c, _, L in EB_CASES}
                     | {(c, N, 2, PLAN_KIND[c]) for c, _, _ in TENSOR_CASES for N in (8192, 16384)})


def test_digits_folded_at_50_bits():
    """digits_kernel<true> (a chain with folded transforms and no Ntt16Digits): the centred lift of every canonical value of residue i
    into q_j, through fold_store under q_j; the lift itself is canonical"""
    N, L, nb = 16384, 3, 2
    o = _oracle(1 << 50, N, L)
    qs, _ = _mods(o)
    d2 = lz.canon_array(qs, lz.VALUE_NAMES, (nb,), N, np.random.default_rng(N))
    for i, q in enumerate(qs):   # the two residues on either side of the centre
        d2[:, i, 5::64], d2[:, i, 6::64] = np.uint64((q - 1) // 2), np.uint64((q + 1) // 2)
    got, plan, _ = _run("digits", o, {"d2": d2}, {"dig": (nb, L, L, N)}, nb=nb, fold=1)
    assert plan["fold"] == 1 and plan["small_moduli"] == 0
    for b in range(nb):
        for i, qi in enumerate(qs):
            v = lz.obj(d2[b, i])
            centred = np.where(np.array(2 * v >= qi, dtype=bool), v - qi, v)
            want = np.stack([lz.u64(centred % qj) for qj in qs])
            _check_fold_store(o, got["dig"][b, i], want, 0, "row %d residue %d" % (b, i), canonical_u=True)


# ---- forward transforms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy_out", [0, 1])
@pytest.mark.parametrize("N,fold,kernel", [(8192, 0, "blocked16"), (16384, 1, "blocked16"), (4096, 0, "blocked32")],
                         ids=["ntt16-8192", "ntt16-16384-folded", "ntt32-4096"])
def test_forward_transform(N, fold, kernel, lazy_out):
    """the forward transforms in lane order on inputs over [0, 8q): the 16-coefficient kernel one slice per limb and folded (its input
    is then what fold_store leaves: the oracle transforms the coefficients behind it), the 32-coefficient kernel; canonical out, or --
    lazy_out -- below 8q"""
    L = 3
    o = _oracle("default", N, L)
    qs, _ = _mods(o)
    data = lz.lazy_array(qs, lambda q: 8 * q, (2,), N, np.random.default_rng(N + fold))
    got, plan, _ = _run("ntt", o, {"data": data}, {"data": (2, L, N)}, nlimbs=2 * L, sigma=1, fold=fold, lazy_out=lazy_out)
    assert plan["kernel"] == kernel and plan["global_stages"] == 0 and plan["fold"] == fold
    m = _lane(o, plan, got)
    want = np.empty_like(data)
    for r in range(2):
        for i, q in enumerate(qs):
            x = data[r, i] % np.uint64(q)
            if fold:
                x = lz.unfold_store(x, *lz.fold_w(o, i))
            want[r, i] = o.ntt(i, x)[m]
    if lazy_out:
        _congruent(got["data"], want, qs, lambda q: 8 * q, "lazy_out")
    else:
        bad = np.argwhere(got["data"] != want)
        assert not len(bad), "first of %d: polynomial %d limb %d lane position %d" % ((len(bad),) + tuple(bad[0]))
