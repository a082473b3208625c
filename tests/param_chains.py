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


def chain_by_name(N, L, name):
    """named_chain, and q_last_wide under its own name"""
    return q_last_wide(N, L) if name == "q_last_wide" else named_chain(N, L, name)


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
