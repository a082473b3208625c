"""tests/lazy_inputs.py on the CPU: the lazy representatives are where claimed, the crafted operands of the key-switch MAC fill its
column accumulators as far as the proof in relin_mac_kernel allows and no further, and every exact reference agrees with the oracle
on canonical inputs.  Together with tests/test_gpu_lazy_inputs.py: a kernel with one uncounted term fails there and passes the rest
of the suite (uniform operands stay far below the columns' ends).

Two statements about the columns are weaker here than one might write them down from the bound arithmetic, because the exact
integers say so:
  * "one more term reaches 2^64" holds for the BOUND -- (L + 9) 2^60 + 2^30 at L = 7 -- while eight exact products of full halves
    and a 2^63 - 1 word stop 2^34 short of it ((2^30 - 1)^2 = 2^60 - 2^31 + 1); asserted: the bound reaches 2^64, the exact columns
    come within 2^36 of it.  The own-limb term added whole, at the top of its range [0, 4q), does wrap column 0.
  * uniform operands stay below half of column 0's bound and below half the 64-bit word in column 1: column 1's bound is 14 2^60, a
    uniform sum has mean 3.5 2^60 and deviation 0.83 2^60, so 7 2^60 is met by some of 10^5 positions; 2^63 is what the argument needs
    (a further term adds 2 2^60).
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from oracle import exact as ex
from tests import coeff_columns as ccol
from tests import lazy_inputs as lz
from tests import param_chains as pc
from tests.param_chains import T32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
P60, P64 = 1 << 60, 1 << 64


def _chain(name, N, L):
    if name == "default":
        q, p = ob.default_moduli(N, L)
    elif isinstance(name, int):
        q, p = pc.uniform_chain(N, L, name)
    else:
        q, p = pc.named_chain(N, L, name)
    return [int(v) for v in q], [int(v) for v in p]


# ---- the families ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["default", "barrett_edges", 1 << 50])
def test_representatives_are_where_claimed(chain):
    N = 4096
    qs, ps = _chain(chain, N, 3)
    rng = np.random.default_rng(1)
    for q in qs + ps:
        h_lo, h_hi = lz.full_halves(q)
        assert h_lo < q and h_lo & lz.MASK30 == lz.MASK30 and h_lo + (1 << 30) >= q
        assert h_hi < q and h_hi & lz.MASK30 == 0 and h_hi + (1 << 30) > q - 1
        for B in (4 * q, 8 * q, 1 << 63):
            for r in (0, 1, q - 1, h_lo):
                reps = lz.representatives(r, q, B)
                assert all(x % q == r and x < B for x in reps) and reps[-1] + q >= B and len(reps) == len(set(reps))
            words, r, k = lz.lazy_limb(q, B, N, rng, shift=2)
            wo, ro, ko = lz.obj(words), lz.obj(r), lz.obj(k)
            assert (wo == ro + ko * q).all() and (wo % q == ro).all() and (ro < q).all() and (wo < B).all()
            ks = lz.multiples(q, B)
            assert ks[0] == 0 and ks[-1] == (B - 1) // q
            if B != 1 << 63 or chain != 1 << 50:
                assert ks == list(range((B - 1) // q + 1))   # every k there is
            # every k occurs -- with value 0 (the one value whose every multiple fits under 2^63), and in both halves of the limb
            for half in (slice(0, N // 2), slice(N // 2, N)):
                assert set(ko[half][ro[half] == 0]) >= set(ks)
                for val in (1, q - 1, q - 2, h_lo, h_hi):   # the other fixed values: every multiple that fits
                    assert set(ko[half][ro[half] == val]) >= set(kk for kk in ks if val + kk * q < B)
                assert (ro[half] >= q - (1 << 24)).sum() > N // 16 and len(set(ro[half])) > N // 16   # near-q and uniform draws
            # the largest word of the range, and folded pairs that differ
            assert int(words[N // 2 - 1]) == B - 1 and int(words[N - 1]) == B - 1
            assert (k[:N // 2 - 1] != k[N // 2:N - 1]).mean() > 0.5 and (r[:N // 2 - 1] != r[N // 2:N - 1]).mean() > 0.8


def test_lane_map_is_a_permutation_of_pairs():
    for N, sl, T, kp in [(4096, 4096, 128, 16), (8192, 8192, 512, 8), (16384, 8192, 512, 8)]:
        m = lz.lane_map(N, sl, T, kp)
        assert sorted(m) == list(range(N)) and (m[1::2] == m[0::2] + 1).all() and (m // sl == np.arange(N) // sl).all()
        assert m[2 * T] == 2 and m[2] == 2 * kp   # pair 1 of thread 0 sits at T, pair 0 of thread 1 belongs at kp


# ---- the MAC's columns -----------------------------------------------------------------------------------------------------------
def _mac_case(uniform, L=7, N=4096):
    qs, ps = _chain("default", N, L)
    rng = np.random.default_rng(N + L)
    if uniform:
        ops = {"d01": lz.uniform_array(qs, (1, 2), N, rng), "dig": lz.uniform_array(qs, (1, L), N, rng),
               "key": lz.uniform_array(qs, (1, L, 2), N, rng)}
    else:
        ops = lz.mac_operands(qs, ps, N, 1, 1, 1, rng)
    return qs, ops


def test_mac_columns_reach_the_claimed_bounds_and_stop_there():
    """relin_mac_kernel at L = 7 (kernels_keyswitch.hip): column 0 < (L + 8) 2^60 + 2^30 < 2^64, column 1 < 2 L 2^60 + 2^32"""
    L = 7
    qs, ops = _mac_case(False)
    bound0, bound1 = (L + 8) * P60 + (1 << 30), 2 * L * P60 + (1 << 32)
    assert bound0 < P64 and bound1 < P64
    top0 = top1 = whole0 = more0 = more1 = 0
    for j, q in enumerate(qs):
        v = 4 * q - 1   # the own-limb term at the top of its range
        full = lz.split30(lz.full_halves(q)[0])
        for c in range(2):
            c0, c1 = lz.mac_columns(ops["d01"][0], ops["dig"][0], ops["key"][0, :, :, :, :], j, c, v)
            assert c0.max() < bound0 and c1.max() < bound1
            top0, top1 = max(top0, c0.max()), max(top1, c1.max())
            whole0 = max(whole0, lz.mac_columns(ops["d01"][0], ops["dig"][0], ops["key"][0], j, c, v, whole=True)[0].max())
            extra = [0, 0, 0]
            lz.colacc_mac(extra, full, full)   # an eighth term of full halves
            more0, more1 = max(more0, c0.max() + extra[0]), max(more1, c1.max() + extra[1])
    # within one term's worth of the claimed bounds
    assert top0 >= bound0 - P60 and top1 >= bound1 - P60
    # one more term: the bound reaches 2^64, the exact columns leave no room for a word of 2^36
    assert (L + 1 + 8) * P60 + (1 << 30) >= P64
    assert more0 >= P64 - (1 << 36) and more1 >= P64 - (1 << 36)
    # the own-limb term added whole wraps column 0
    assert whole0 >= P64


def test_mac_columns_of_uniform_operands_stay_far_below():
    L = 7
    qs, ops = _mac_case(True)
    bound0 = (L + 8) * P60 + (1 << 30)
    for j, q in enumerate(qs):
        for c in range(2):
            c0, c1 = lz.mac_columns(ops["d01"][0], ops["dig"][0], ops["key"][0], j, c, q - 1)
            assert 2 * c0.max() < bound0 and c1.max() < 1 << 63


# ---- the references against the oracle -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """N = 64, L = 3: a product of two uniform ciphertexts taken apart with the oracle's own pieces"""
    N, L = 64, 3
    o = ob.Oracle(N, L, T32)
    qs, ps = ccol.moduli(o)
    rng = np.random.default_rng(64)
    x = np.stack([ccol.uniform_poly(qs, N, rng) for _ in range(2)])
    y = np.stack([ccol.uniform_poly(qs, N, rng) for _ in range(2)])

    def ntt_qp(poly):
        return np.stack([o.ntt(a, poly[a]) for a in range(o.M)])

    def intt_qp(poly):
        return np.stack([o.intt(a, poly[a]) for a in range(o.M)])
    e = np.stack([ntt_qp(o.expand_q_to_qp(ccol.intt_q(o, x[c]))) for c in range(2)] + [ntt_qp(o.scale_pq_expand(ccol.intt_q(o, y[c]))) for c in range(2)])
    return {"o": o, "qs": qs, "ps": ps, "x": x, "y": y, "e": e, "intt_qp": intt_qp, "want": o.mul_tensor(x, y), "rng": rng}


def test_tensor_reference_agrees_with_the_oracle(small):
    o = small["o"]
    d = lz.ref_tensor(small["e"][None], small["qs"] + small["ps"])[0]
    got = np.stack([ccol.ntt_q(o, o.scale_round_tp(small["intt_qp"](d[c]))) for c in range(3)])
    assert (got == small["want"]).all()


def test_own_limb_term_and_deg2_reference_agree_with_the_oracle(small):
    """scale-and-round is its P-limb part plus [t P^-1]_{q_k} d_k (what p_only01 / p_only2 leave to the MAC and the degree-2 finish):
    the degree-2 finish of the P-limb parts, with the term from the QP operands, is the oracle's tensor product"""
    o, qs, ps = small["o"], small["qs"], small["ps"]
    cs = lz.own_limb_consts(qs, ps, o.t)
    d = lz.ref_tensor(small["e"][None], qs + ps)[0]
    part = []
    for c in range(3):
        dc = small["intt_qp"](d[c])
        full = o.scale_round_tp(dc)
        dc[:o.L] = 0
        p_only = o.scale_round_tp(dc)
        for k, q in enumerate(qs):
            own = lz.obj(small["intt_qp"](d[c])[k]) * cs[k] % q
            assert (lz.obj(full[k]) == (lz.obj(p_only[k]) + own) % q).all()
        part.append(ccol.ntt_q(o, p_only))
    got = lz.ref_deg2_row(np.stack(part), small["e"], qs, cs)
    assert (got == small["want"]).all()
    mask = ccol.uniform_poly(qs, o.N, small["rng"])
    assert (lz.mul_mask(got, mask, qs) == np.stack([ccol.mulmod_rows(got[c], mask, qs) for c in range(3)])).all()


def test_mac_reference_agrees_with_the_oracle(small):
    o, qs, ps = small["o"], small["qs"], small["ps"]
    L, N = o.L, o.N
    d, rng = small["want"], small["rng"]
    evk = np.stack([np.stack([ccol.uniform_poly(qs, N, rng) for _ in range(2)]) for _ in range(L)])
    d2c = ccol.intt_q(o, d[2])
    dig = np.stack([ccol.ntt_q(o, np.stack([np.array([ccol.lift_definition(int(v), qs[i], qs[j]) for v in d2c[i]], dtype=np.uint64) for j in range(L)]))
                    for i in range(L)])
    want = o.relin(d, evk)
    assert (lz.ref_mac_row(d[:2], dig, evk, qs) == want).all()
    # with the own-limb term: d01 without c_j (a (x) b), the term from the QP operands
    cs = lz.own_limb_consts(qs, ps, o.t)
    t = lz.ref_tensor(small["e"][None], qs + ps)[0]
    bare = np.stack([np.stack([lz.u64((lz.obj(d[c, j]) - cs[j] * lz.obj(t[c, j])) % q) for j, q in enumerate(qs)]) for c in range(2)])
    other = np.stack([np.stack([lz.u64((lz.obj(d[c, j]) - lz.obj(t[c, j])) % q) for j, q in enumerate(qs)]) for c in range(2)])
    assert (lz.ref_mac_row(bare, dig, evk, qs, small["e"], cs) == want).all()
    assert not (lz.ref_mac_row(other, dig, evk, qs, small["e"], cs) == want).all()


def test_fold_relations_agree_with_the_oracles_transform(small):
    """position p of the oracle's transform holds a(rho), rho = psi^(2 bitrev(p) + 1); for p < N/2, rho^(N/2) = psi^(N/2), so a(rho) is
    the half-size polynomial u + psi^(N/2) v at rho, and u - psi^(N/2) v in the other half: the store relation.  The load relation
    undoes the last stage of the inverse: (u', v') = ((y0 + y1), (y0 - y1) psi^(-N/2)) / N ... with N^-1 where the half-size inverse
    transforms have left it out"""
    o, rng = small["o"], small["rng"]
    N, H = o.N, o.N // 2
    for a in (0, o.L, o.M - 1):
        q, w = lz.fold_w(o, a)
        x = rng.integers(0, q, N, dtype=np.uint64)
        y = lz.fold_store(x, q, w)
        E = o.ntt(a, x)
        for p in (0, 1, 5, H - 1, H, H + 6, N - 1):
            rho = pow(o.psi(a), 2 * ex.bitrev(p, N.bit_length() - 1) + 1, q)
            half = y[:H] if p < H else y[H:]
            assert int(E[p]) == sum(int(c) * pow(rho, n, q) for n, c in enumerate(half)) % q
        assert (lz.unfold_store(y, q, w) == x).all()
        # a lazy representative of y changes nothing
        assert (lz.unfold_store(lz.u64(lz.obj(y) + 3 * q), q, w) == x).all()
        # load: the pair (u, v) that the folded inverse hands over is N (x0 + x1 psi^(N/2), x0 - x1 psi^(N/2)) / 2 ... undone exactly
        uv = lz.u64(lz.obj(y) * (N // 2) % q)
        assert (lz.fold_load(uv, q, w) == x).all()


def test_lazy_inputs_check_cross_compiles():
    subprocess.check_call(["make", "-j8", "-C", CSRC, "build/lazy_inputs_check"], stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build", "lazy_inputs_check")
    assert os.path.exists(exe)
    # usage errors are status 2, before anything touches a device
    for args in ([], ["tensor", "/nonexistent", "4096", "0", "65537"], ["tensor", "/nonexistent", "4096", "2", "65537", "3", "5"]):
        assert subprocess.run([exe] + args, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 2
