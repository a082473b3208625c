"""The three butterfly blocks for q = 2^60 - d (csrc/ntt16_kernel.h: bfly<INV, SC, H2, ArithKind::fold> -- forward with u = fold(a),
inverse with a' = fold(a + b), inverse without a fold), each in its four forms (twiddle in SGPRs or per lane, 2 sh as an operand or
doubled in the block), on the device against the exact-integer model of tests/fold_bfly_model.py, to the bit.

Operands, per modulus:
  forward   a at 0, 2^60 - 1, 2^60, T - 1, 4q - 1, 4q, 8q - 1, 2^63 - 1, 2^64 - 1 (the fold takes any word; T = 2^60 + 2^31);
            b at 0, q, 4q - 1, 8q - 1, 2^63 - 1
  inverse   a over the same kind of edges below 4q, b at 0, q, 4q - 1; without a fold both legs up to T - 1
  low words at 2^32 - 1 in a, b and w, so that the seeded chain's partial sums pass 2^64 (asserted to happen)
  the directed Shoup family -- low words of the multiplicand and of floor(w 2^63 / q) within 2^8 of 2^32 - 1 -- whose 63-bit
  estimate comes out 3 short (asserted to happen for every block and modulus)
  random operands over the whole contract up to 2^16 cases per block
Moduli: the first and last of the default chain at N = 16384, both ends of fold_edge (d just under 2^27), and the smallest d the
chain generator yields (the first prime = 1 mod 2N below 2^60, at N = 8192).

The operands go through tests/arith_check's device harness in a program of its own, csrc/build/fold_bfly_check (csrc/Makefile builds
it beside arith_check); it runs once, as a child process.
"""
import os
import random
import subprocess

import pytest

from tests import fold_bfly_model as fm
from tests.param_chains import fold_edge, uniform

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
EXE = os.path.join(CSRC, "build", "fold_bfly_check")
FORMS = ("vec,h1", "vec,h2", "sc,h1", "sc,h2")
M32, W64, T = fm.M32, fm.W64, fm.T
PER_BLOCK = 1 << 16


def _moduli():
    default = uniform(16384, 15)
    edge = [int(v) for part in fold_edge(16384, 7) for v in part]
    smallest_d = uniform(8192, 1)[0]
    ms = [default[0], default[-1], edge[0], edge[-1], smallest_d]
    assert all(0 < (1 << 60) - m < (1 << 27) for m in ms) and (1 << 26) < (1 << 60) - edge[0] and (1 << 60) - smallest_d == min((1 << 60) - m for m in ms)
    return sorted(set(ms))


def _cases():
    """[(kind, q, a, b, w)], PER_BLOCK per kind; the scalar forms take one w per launch, so the twiddles are few"""
    out = []
    moduli = _moduli()
    for kind in ("ctf", "gsf", "gsn"):
        mine = []
        for q in moduli:
            low = (((q >> 32) - 1) << 32) | M32            # a twiddle whose low word is all ones
            dws = fm.directed_ws(q, 2)
            ws = [1, q - 1, low] + dws
            if kind == "ctf":
                a_s = fm.forward_a_edges(q) + [(3 << 60) | M32, (7 << 60) | (M32 << 28) | M32, (4 * q - 1) | M32]
                b_s = [0, q, 4 * q - 1, 8 * q - 1, (1 << 63) - 1, (3 << 32) | M32, ((1 << 63) - 1) & ~(1 << 32)]
                lim_a, lim_b = W64, 1 << 63
            elif kind == "gsf":
                a_s = [0, 1, q, T - 1, T, 2 * q, 4 * q - 1, (2 * q) | M32, (3 * q) | M32]
                b_s = [0, q, 4 * q - 1, T, (3 * q) | M32]
                lim_a = lim_b = 4 * q
            else:
                a_s = [0, 1, q, T - 1, (1 << 60) | (M32 >> 2), q | M32, (q >> 1) | M32]
                b_s = [0, q, T - 1, q | M32]
                lim_a = lim_b = T
            mine += [(kind, q, a, b, w) for a in a_s for b in b_s for w in ws]
            # the directed family: multiplicands whose estimate against a directed w is 3 short.  Forward: b itself; inverse: a + 4q - b
            for w in dws:
                found = 0
                for m in fm.directed_bs(q, w, 8 * q):       # (the worst estimates first)
                    if kind == "ctf":
                        fits = [(kind, q, a, m, w) for a in (0, T - 1, 8 * q - 1)]
                    else:                                   # a + 4q - b = m with a, b inside the contract
                        fits = [(kind, q, m - 4 * q + b, b, w) for b in (0, q, lim_b - 1) if 0 <= m - 4 * q + b < lim_a]
                    mine += fits
                    found += bool(fits)
                    if found == 24:
                        break
        rng = random.Random(len(mine))
        per_q = (PER_BLOCK - len(mine)) // len(moduli)
        for q in moduli:
            ws = [1, q - 1] + fm.directed_ws(q, 2)
            lim_a, lim_b = {"ctf": (W64, 1 << 63), "gsf": (4 * q, 4 * q), "gsn": (T, T)}[kind]
            mine += [(kind, q, rng.randrange(lim_a), rng.randrange(lim_b), ws[i % len(ws)]) for i in range(per_q)]
        assert PER_BLOCK - len(moduli) < len(mine) <= PER_BLOCK
        out += mine
    return out


def test_fold_blocks_on_crafted_operands(tmp_path):
    cases = _cases()
    want = [fm.block(*c) for c in cases]
    for kind in ("ctf", "gsf", "gsn"):
        for q in _moduli():
            mult = [(c[3] if kind == "ctf" else c[2] + 4 * q - c[3], c[4]) for c in cases if c[0] == kind and c[1] == q]
            assert any(fm.shoup_error(q, m, w) == 3 for m, w in mult), "no operand of %s under %d whose estimate is 3 short" % (kind, q)
    wraps = [c for c in cases if c[0] == "ctf" and (c[3] & M32) * (c[4] & M32) + fm.fold(c[2], c[1]) >= W64]
    assert {c[1] for c in wraps} == set(_moduli()), "no operand set whose seeded partial sum passes 2^64"

    subprocess.check_call(["make", "-j8", "-C", CSRC, "build/fold_bfly_check"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EXE), "csrc/Makefile did not build " + EXE
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %d %d %d %d\n" % c for c in cases))
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "fold_bfly_check done" in r.stdout, "status %d\n%s" % (r.returncode, r.stdout[-4000:])

    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "r":
            got[(int(f[1]), f[2])] = (int(f[3]), int(f[4]))
    assert len(got) == len(cases) * len(FORMS)
    bad = [(cases[i], form, got[i, form], want[i]) for i in range(len(cases)) for form in FORMS if got[i, form] != want[i]]
    print("%d cases x %d forms, %d with bl wl + u >= 2^64, %d differ" % (len(cases), len(FORMS), len(wraps), len(bad)))
    assert not bad, bad[:8]
