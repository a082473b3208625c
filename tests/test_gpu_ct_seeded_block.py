"""The forward butterfly block of the 16-coefficient transform (csrc/ntt16_kernel.h: bfly<false, SC, H2>, four forms) on crafted lazy
operands against Python integers.

The block seeds the low accumulation chain of the Shoup remainder with u = a mod+ 4q, so that the chain ends as a' = u + v, and forms
b' = (2u + 4q) - a'; everything is arithmetic mod 2^64.  The operands are the ends of its contract -- a in [0, 8q), b below 2^63 --
where the seeded chain carries the most: a at both ends of both halves of [0, 8q), b at 0, q, 8q - 1 and 2^63 - 1, w at 1 and q - 1,
and a set in which the first partial sum bl wl + u itself passes 2^64 (harmless: asserted to happen, and to change nothing).
Moduli: the two largest 60-bit primes of the default chain and the largest 59-bit one.

The expected values are exact: the quotient estimate is restated from the block's comment, qe = 2 bh sh + ((bh sl + bl sh) >> 31)
with s = floor(w 2^63 / q), so v = b w - qe q is known to the bit (and checked to be b w mod q plus at most 3 q).

The operands go through tests/arith_check's device harness (dev.h) in a program of its own, csrc/build/ct_seeded_check, which
csrc/Makefile builds beside arith_check; it runs once, as a child process.
"""
import os
import subprocess

import pytest

from tests.param_chains import uniform

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
EXE = os.path.join(CSRC, "build", "ct_seeded_check")
FORMS = ("vec,h1", "vec,h2", "sc,h1", "sc,h2")
W64 = 1 << 64
M32 = (1 << 32) - 1


def _primes():
    return uniform(16384, 2) + uniform(16384, 1, 1 << 59)


def _expected(q, a, b, w):
    """(a', b', bl wl + u) of the block's contract"""
    s = (w << 63) // q
    bl, bh, sl, sh = b & M32, b >> 32, s & M32, s >> 32
    qe = 2 * bh * sh + ((bh * sl + bl * sh) >> 31)
    v = b * w - qe * q
    assert 0 <= v < 4 * q and v % q == b * w % q and b * w // q - qe <= 3
    u = a - 4 * q if a >= 4 * q else a
    ao, bo = u + v, u + 4 * q - v
    assert 0 <= ao < 8 * q and 0 < bo <= 8 * q and 2 * u + 4 * q < W64
    return ao, bo % W64, bl * (w & M32) + u


def _cases():
    out = []
    for q in _primes():
        for a in (0, 4 * q - 1, 4 * q, 8 * q - 1):
            for b in (0, q, 8 * q - 1, (1 << 63) - 1):
                for w in (1, q - 1):
                    out.append((q, a, b, w))
        # bl wl + u past 2^64: both low words all ones, u at the top of its range
        w = (((q >> 32) - 1) << 32) | M32
        for a in (4 * q - 1, 8 * q - 1):
            for b in ((1 << 63) - 1, (3 << 32) | M32):
                out.append((q, a, b, w))
    return out


def test_forward_block_on_crafted_lazy_operands(tmp_path):
    primes = _primes()
    assert (1 << 59) < primes[1] < primes[0] < (1 << 60) and (1 << 58) < primes[2] < (1 << 59)
    cases = _cases()
    want = {c: _expected(*c) for c in cases}
    wraps = [c for c in cases if want[c][2] >= W64]
    assert {c[0] for c in wraps} == set(primes), "no operand set whose seeded partial sum passes 2^64"

    subprocess.check_call(["make", "-j8", "-C", CSRC, "build/ct_seeded_check"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EXE), "csrc/Makefile did not build " + EXE
    path = tmp_path / "cases.txt"
    path.write_text("".join("%d %d %d %d\n" % c for c in cases))
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "ct_seeded_check done" in r.stdout, "status %d\n%s" % (r.returncode, r.stdout[-4000:])

    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "ct":
            got[(tuple(int(x) for x in f[1:5]), f[5])] = (int(f[6]), int(f[7]))
    assert len(got) == len(cases) * len(FORMS)
    bad = [(c, form, got[c, form], want[c][:2]) for c in cases for form in FORMS if got[c, form] != want[c][:2]]
    print("%d cases x %d forms, %d with bl wl + u >= 2^64, %d differ" % (len(cases), len(FORMS), len(wraps), len(bad)))
    assert not bad, bad[:8]
