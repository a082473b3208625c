"""The folded column reduction of csrc/stage_a_common.h (PIE_COLACC_FOLD_HEAD, colacc_fold) step by step on Python integers
(plain module, imported by the test files; not a conftest).

A column accumulator (c0, c1, c2) holds z = c0 + c1 2^30 + c2 2^60; the modulus is q = 2^60 - d.  The block's contract:
  in    three 64-bit columns whose carry normalisation stays inside 64 bits (n1 = c1 + (c0 >> 30) < 2^64, n2 = c2 + (n1 >> 30) < 2^64:
        what COLACC_MAX_TERMS / COLACC_MAX_TOTAL of madasm.h guarantee), z < 2^123 for d < 2^28 and z < 2^124 for d < 2^27
  out   lazy: a value congruent to z and below 4q;  canonical: z mod q
MAX_D is the bound a context is selected by: the smaller of the two (csrc/kernels.hpp, COLACC_FOLD_MAX_D).
"""
import random

M28, M30, M32, M60, M64 = (1 << 28) - 1, (1 << 30) - 1, (1 << 32) - 1, (1 << 60) - 1, (1 << 64) - 1
MAX_D = {123: 1 << 28, 124: 1 << 27}
SELECT_MAX_D = min(MAX_D.values())


class Trace(dict):
    """every intermediate of one run, by the names of the block's comment"""


def value(c0, c1, c2):
    return c0 + (c1 << 30) + (c2 << 60)


def fold_lazy(c0, c1, c2, d, tr=None):
    """the thirteen instructions; returns r (and fills tr).  Raises AssertionError where a step leaves its register width"""
    tr = tr if tr is not None else Trace()
    n1 = c1 + (c0 >> 30)                      # v_lshrrev_b64, v_lshl_add_u64
    n2 = c2 + (n1 >> 30)                      # v_lshrrev_b64, v_lshl_add_u64
    assert n1 <= M64 and n2 <= M64, "the input contract: the normalisation stays inside 64 bits"
    lo_l = (c0 & M30) | ((n1 << 30) & M32)    # v_and_b32, v_lshl_or_b32
    lo_h = (n1 >> 2) & M28                    # v_bfe_u32
    lo60 = (lo_h << 32) | lo_l
    n2l, n2h = n2 & M32, n2 >> 32
    u = n2h * d                               # v_mad_u64_u32
    t = n2l * d + lo60                        # v_mad_u64_u32
    um = u & M28                              # v_and_b32
    k = u >> 28                               # v_alignbit_b32: the low 32 bits of u >> 28
    th = (t >> 32) + um                       # v_add_u32
    t2 = ((th & M32) << 32) | (t & M32)
    r = t2 + (k & M32) * d                    # v_mad_u64_u32
    tr.update(n1=n1, n2=n2, lo60=lo60, u=u, t=t, um=um, k=k, th=th, t2=t2, r=r)
    assert lo60 == value(c0, c1, c2) & M60
    assert u <= M64 and t <= M64 and r <= M64, "an intermediate left 64 bits"
    assert k <= M32, "u >> 28 left one word"
    assert th <= M32, "the high-word add carried"
    return r


def fold_canon(c0, c1, c2, d, tr=None):
    """... one more fold and one conditional subtraction: z mod q"""
    tr = tr if tr is not None else Trace()
    q = (1 << 60) - d
    r = fold_lazy(c0, c1, c2, d, tr)
    h = r >> 60                               # v_lshrrev_b32 on the high word
    r1 = (r & M60) + h * d                    # v_and_b32 on the high word, v_mad_u64_u32
    assert r1 <= M64 and r1 < 2 * q, "the second fold left [0, 2q)"
    s = r1 - q                                # v_lshl_add_u64 with 2^64 - q, sign mask, two v_bfi_b32
    out = r1 if s < 0 else s
    tr.update(h=h, r1=r1, out=out)
    return out


def columns_of(z):
    """z as carry-normalised columns"""
    return z & M30, (z >> 30) & M30, z >> 60


def crafted(d, bits):
    """the crafted columns for z < 2^bits: a list of (name, (c0, c1, c2))"""
    bound = 1 << bits
    out = [("zero", (0, 0, 0)), ("bound - 1", columns_of(bound - 1))]
    # all-ones columns, as far as the input contract lets them be: c0 all ones with the largest c1 that keeps n1 inside 64 bits (n1 is
    # then all ones), and c1 all ones with the largest c0 that adds nothing to it; c2 the largest that keeps z under the bound
    for name, c0, c1 in (("c0 ones, n1 ones", M64, M64 - (M64 >> 30)), ("c1 ones", M30, M64)):
        c2 = (bound - 1 - c0 - (c1 << 30)) >> 60
        out.append((name, (c0, c1, c2)))
    n2max = (bound >> 60) - 1
    out.append(("n2_hi max, n2_lo 0", (0, 0, n2max & ~M32)))
    out.append(("n2_hi max, rest ones", (M30, M30, n2max)))
    # u = n2_hi d with its low 28 bits all ones (d odd: n2_hi = -d^-1 mod 2^28, raised by multiples of 2^28 to the largest value the
    # bound allows), t's high word at its maximum (n2_lo and lo60 all ones)
    if d & 1:
        n2h = (-pow(d, -1, 1 << 28)) % (1 << 28)
        top = n2max >> 32
        n2h += ((top - n2h) >> 28) << 28
        assert 0 <= n2h <= top and (n2h * d) & M28 == M28
        out.append(("u low 28 ones, t high max", (M30, M30, (n2h << 32) | M32)))
    return out


def random_columns(rng, bits, count):
    """`count` column triples, not normalised, with z < 2^bits and the normalisation inside 64 bits"""
    out = []
    for _ in range(count):
        c0 = rng.getrandbits(64)
        c1 = rng.getrandbits(64) % (M64 - (M64 >> 30))
        c2max = ((1 << bits) - 1 - c0 - (c1 << 30)) >> 60
        c2 = rng.randrange(c2max + 1) if rng.random() < 0.75 else c2max - rng.getrandbits(8) % (c2max + 1)
        out.append((c0, c1, c2))
    return out


def check_ds(c3_ds, c5_max_d):
    """the d values of the checks: 1, the nine of the default chain at N = 16384, the largest at N = 32768, the selection bound - 1"""
    return [1] + list(c3_ds) + [c5_max_d, SELECT_MAX_D - 1]


def rng_for(d, bits):
    return random.Random(d * 1000 + bits)
