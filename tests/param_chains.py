"""Prime chains for the parameter envelope tests (plain module, imported by the test files; not a conftest).

piehip_create accepts any caller-supplied chain of distinct primes below 2^61, = 1 (mod 2N) and above t.  The kernels pick
their arithmetic by the widths of these moduli (the one-word Barrett of the mad paths needs 2^59 < q < 2^60, a modulus
>= 2^60 turns off the lazy-residue transforms, the digit lift needs a Barrett step when q_i >= 2 q_j), so the chains here
are chosen to reach each branch.  Every builder returns (q[L], p[L + 1]) as numpy uint64 arrays.
"""
import numpy as np

from oracle import binding as ob
from oracle import exact as ex

T16 = 65537
T32 = 4296540161
T40 = 1099579260929      # client.PLAINTEXT_MODULI[40]
T48 = 281474981953537    # client.PLAINTEXT_MODULI[48]

NAMED = ("q0_wide", "q_narrow_p_wide", "one_p_61", "barrett_edges")


def q_last_wide(N, L):
    """(q, p): Q = [45-bit, .., 45-bit, 60-bit], P = 55-bit -- the one chain whose DROPPED modulus is far wider than a kept one: the
    limb drop's offset, a multiple of q_i that reaches (q_l - 1)/2, then spans about 2^14 multiples of q_i.  Not in NAMED (other files
    parametrise over it): the tests of the limb drop ask for it by name through chain_by_name"""
    assert L >= 2
    return split(uniform(N, L - 1, 1 << 45) + uniform(N, 1) + uniform(N, L + 1, 1 << 55), L)


FOLD_MAX_D = 1 << 27   # csrc/kernels.hpp: COLACC_FOLD_MAX_D
FOLD_BOUND = (1 << 60) - FOLD_MAX_D


def reduction_kind(q, p):
    """the kind a context of these moduli must select, from the rule itself (piehip.h: piehip_get_reduction): "wide" unless every Q
    and P modulus lies in (2^59, 2^60); then "fold" if every one is 2^60 - d with d < 2^27, "barrett" otherwise"""
    ms = [int(v) for v in q] + [int(v) for v in p]
    if not all((1 << 59) < m < (1 << 60) for m in ms):
        return "wide"
    return "fold" if all((1 << 60) - m < FOLD_MAX_D for m in ms) else "barrett"


def level_chain(q, p, Lc):
    """the moduli of the level context of Lc limbs (piehip_set_chain_schedule: HostParams::init on the parent's q and p with L = Lc):
    q_0 .. q_{Lc-1} and p_0 .. p_Lc -- a prefix of each side, so the level drops q_Lc .. q_{L-1} and p_{Lc+1} .. p_L"""
    return q[:Lc], p[:Lc + 1]


def fold_edge(N, L):
    """(q, p): the 2L + 1 smallest primes = 1 (mod 2N) above 2^60 - 2^27, ascending -- the folded kind with every d just under the
    selection bound (d in (2^26, 2^27) for 15 primes at N = 8192, 16384, 32768)"""
    return split(prime_above(N, FOLD_BOUND, 2 * L + 1), L)


def barrett_60(N, L):
    """(q, p): the 2L + 1 largest such primes below 2^60 - 2^27, descending -- the Barrett kind on a chain otherwise shaped like a
    default one (d in (2^27, 2^28) for 15 primes at those N)"""
    return uniform_chain(N, L, FOLD_BOUND)


def over_at(N, L, where):
    """(q, p): the default chain with ONE modulus replaced by barrett_60's first prime, so the context is of the Barrett kind.  A
    level of Lc limbs keeps q_0 .. q_{Lc-1} and p_0 .. p_Lc (level_chain), hence
      last_q_over  q_{L-1}: every level Lc < L drops it and folds
      last_p_over  p_L:     likewise
      q4_over      q_4 (L >= 6): the level of 5 limbs keeps it and is of the Barrett kind, the levels of 4 and fewer fold"""
    chain = uniform(N, 2 * L + 1)
    over = uniform(N, 1, FOLD_BOUND)[0]
    at = {"last_q_over": L - 1, "last_p_over": 2 * L, "q4_over": 4}[where]
    assert at < 2 * L + 1 and (where != "q4_over" or L >= 6)
    chain[at] = over
    return split(chain, L)


def chain_by_name(N, L, name):
    """named_chain, and under their own names the chains that are not in NAMED: q_last_wide; fold_edge and barrett_60 on either
    side of the folded reduction's selection bound; last_q_over, last_p_over and q4_over (over_at), whose levels differ in kind
    from their parent"""
    if name == "q_last_wide":
        return q_last_wide(N, L)
    if name == "fold_edge":
        return fold_edge(N, L)
    if name == "barrett_60":
        return barrett_60(N, L)
    if name in ("last_q_over", "last_p_over", "q4_over"):
        return over_at(N, L, name)
    if name == "barrett_one_p_61":
        return barrett_one_p_61(N, L)
    return named_chain(N, L, name)


def barrett_one_p_61(N, L):
    """(q, p): barrett_60 with its last P modulus replaced by a 61-bit prime, as one_p_61 is to the default chain: the parent has no
    lazy transforms and does not fold, every level below L drops that prime, folds (N = 16384, 32768) and is of the Barrett kind"""
    return split(uniform(N, 2 * L, FOLD_BOUND) + uniform(N, 1, 1 << 61), L)


def uniform(N, count, below=1 << 60):
    """the `count` largest primes = 1 (mod 2N) below `below`, descending (the oracle's own generator)"""
    return [int(v) for v in ob.gen_primes(N, count, below)]


def prime_above(N, bound, count=1):
    """the `count` smallest primes = 1 (mod 2N) above `bound`, ascending"""
    out = []
    c = bound - bound % (2 * N) + 1
    if c <= bound:
        c += 2 * N
    while len(out) < count:
        if ex.is_prime(c):
            out.append(c)
        c += 2 * N
    return out


def split(chain, L):
    chain = [int(v) for v in chain]
    assert len(chain) == 2 * L + 1 and len(set(chain)) == len(chain)
    return np.array(chain[:L], dtype=np.uint64), np.array(chain[L:], dtype=np.uint64)


def uniform_chain(N, L, below=1 << 60):
    return split(uniform(N, 2 * L + 1, below), L)


def named_chain(N, L, name):
    """(q, p) of one of the mixed-width chains in NAMED:
      q0_wide          Q = [60-bit, 45-bit, 45-bit, ...], P = 55-bit: digit lifts with q_i >= 2 q_j (the barrett128 branch)
      q_narrow_p_wide  Q 36-bit, P 60-bit: every modulus outside (2^59, 2^60) on the Q side
      one_p_61         the default 60-bit chain with its last P modulus replaced by a 61-bit prime
      barrett_edges    Q holds the first prime above 2^59 and the last below 2^60 (mu = floor(2^123 / q) near 2^64 and
                       near 2^63: the edges of the one-word Barrett); the rest are ordinary 60-bit primes
    """
    if name == "q0_wide":
        return split(uniform(N, 1) + uniform(N, L - 1, 1 << 45) + uniform(N, L + 1, 1 << 55), L)
    if name == "q_narrow_p_wide":
        return split(uniform(N, L, 1 << 36) + uniform(N, L + 1), L)
    if name == "one_p_61":
        return split(uniform(N, 2 * L) + uniform(N, 1, 1 << 61), L)
    if name == "barrett_edges":
        assert L >= 2
        top = uniform(N, 2 * L)          # top[0] is the last prime below 2^60
        return split(prime_above(N, 1 << 59) + top, L)
    raise ValueError(name)
