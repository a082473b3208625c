"""The folded column reduction (csrc/stage_a_common.h: colacc_fold) as its model tests/fold_reduce.py runs it, on exact integers:
for q = 2^60 - d the lazy result is congruent to z and below 4q, the canonical one equals z mod q, the 32-bit add into t's high word
never carries and every intermediate stays inside its registers -- at z < 2^123 for every d below 2^28 that is checked, at z < 2^124
for every d below 2^27.  Primality plays no part.

  d        1; the nine of the default chain at N = 16384; the largest of the thirteen at N = 32768; the selection bound - 1
           (2^27 - 1, both widths); the 123-bit form's own bound - 1 (2^28 - 1, that width alone)
  columns  fold_reduce.crafted (zero, the bound - 1, all-ones columns, n2_hi at its maximum, u with its low 28 bits set under the
           largest t) and 2000 random triples per (d, width)
and the facts about the default chains that the selection rests on: d < 2^24, 2^20, 2^25 at N = 16384, 8192, 32768.
"""
import pytest

from tests import fold_reduce as fr
from tests.param_chains import uniform


def _ds(N, count):
    return [(1 << 60) - q for q in uniform(N, count)]


@pytest.fixture(scope="module")
def ds():
    return fr.check_ds(_ds(16384, 9), max(_ds(32768, 13)))


def test_default_chains_lie_under_the_selection_bound():
    for N, count, bits in ((16384, 9, 24), (8192, 7, 20), (32768, 13, 25)):
        d = _ds(N, count)
        assert all(0 < v < (1 << bits) for v in d), (N, d)
        assert max(d) < fr.SELECT_MAX_D


def _check(c, d, bits, what):
    q = (1 << 60) - d
    z = fr.value(*c)
    assert z < (1 << bits)
    tr = fr.Trace()
    r = fr.fold_lazy(*c, d, tr)          # (asserts the register widths and the carry-free add itself)
    assert r % q == z % q and r < 4 * q, (what, d, bits, c, tr)
    assert r < 3 * q or d >= fr.MAX_D[124], (what, d, bits, c, tr)   # under the selection bound: the Barrett block's own 3q
    assert fr.fold_canon(*c, d) == z % q, (what, d, bits, c)
    return tr


@pytest.mark.parametrize("bits", [123, 124])
def test_fold_holds_its_contract(ds, bits):
    want = [d for d in ds if d < fr.MAX_D[bits]]
    if bits == 123:
        want.append(fr.MAX_D[123] - 1)
    assert fr.SELECT_MAX_D - 1 in want
    for d in want:
        seen = {}
        for name, c in fr.crafted(d, bits):
            seen[name] = _check(c, d, bits, name)
        # the crafted columns reach what they are named for
        top = ((1 << bits) >> 60) - 1
        assert seen["bound - 1"]["n2"] == top and seen["n2_hi max, rest ones"]["n2"] >> 32 == top >> 32
        assert seen["c0 ones, n1 ones"]["n1"] == fr.M64
        hit = seen["u low 28 ones, t high max"]
        assert hit["um"] == fr.M28 and hit["t"] == fr.M32 * d + fr.M60
        rng = fr.rng_for(d, bits)
        for c in fr.random_columns(rng, bits, 2000):
            _check(c, d, bits, "random")


def test_the_bounds_are_the_largest_the_proof_gives():
    """one power of two further the proof's sum reaches 4 2^60: the worst case it counts, every term at its bound, is not below 4q"""
    for bits, k in ((123, 29), (124, 28)):
        assert (1 << 61) + (1 << (32 + k)) + (1 << (bits - 120 + 2 * k)) >= 1 << 62
        k -= 1
        assert (1 << 61) + (1 << (32 + k)) + (1 << (bits - 120 + 2 * k)) < 4 * ((1 << 60) - (1 << k))
        assert fr.MAX_D[bits] == 1 << k
