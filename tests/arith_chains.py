"""Moduli and report parsing for the arithmetic-block harness (tests/arith_check): shared by tests/test_arith_host.py and
tests/test_gpu_arith_blocks.py (plain module, not a conftest).

Every chain goes to the programs as "N,L,t,q_0,..,q_{L-1},p_0,..,p_L"; they run it through HostParams::init and test each distinct
modulus of it, the plaintext modulus included.  Between them the chains hold the default 60-bit chain at N = 16384, both
`barrett_edges` primes, a 36-, 45-, 50- and 55-bit prime, the 61-bit prime of `one_p_61` and the plaintext moduli T16, T32, T40, T48.
"""
import re

from tests.param_chains import T16, T32, T40, T48, named_chain, prime_above, uniform, uniform_chain

N = 16384
MIN_COVER = 64

LOW_EDGE = prime_above(N, 1 << 59)[0]   # first prime above 2^59: floor(2^123 / q) just below 2^64
TOP_EDGE = uniform(N, 1)[0]             # last prime below 2^60 (also q_0 of the default chain)


def _spec(L, t, qp):
    q, p = qp
    return ",".join(str(int(v)) for v in [N, L, t] + list(q) + list(p))


def chains():
    return [
        _spec(4, T16, uniform_chain(N, 4)),
        _spec(2, T32, named_chain(N, 2, "barrett_edges")),
        _spec(2, T40, named_chain(N, 2, "q0_wide")),            # 60-, 45- and 55-bit
        _spec(2, T16, named_chain(N, 2, "q_narrow_p_wide")),    # 36-bit
        _spec(2, T48, named_chain(N, 2, "one_p_61")),           # 61-bit
        _spec(1, T40, uniform_chain(N, 1, 1 << 50)),            # 50-bit
    ]


_LINE = re.compile(r"^arith (\S+) q=(\d+) cases=(\d+) fail=(\d+)(.*)$")


def _hist(rest, key):
    m = re.search(key + r"=\[([\d,]+)\]", rest)
    return [int(v) for v in m.group(1).split(",")] if m else None


def parse(stdout):
    """{(block, q): dict(cases, fail, err, need, kdev, kmod, kdiff)} of a program's report lines"""
    out = {}
    for line in stdout.splitlines():
        m = _LINE.match(line)
        if not m or m.group(1) in ("group", "host"):
            continue
        rest = m.group(5)
        need = re.search(r"need=(-?\d+)", rest)
        kdiff = re.search(r"kdiff=(\d+)", rest)
        out[(m.group(1), int(m.group(2)))] = dict(
            cases=int(m.group(3)), fail=int(m.group(4)), err=_hist(rest, "err"), need=int(need.group(1)) if need else None,
            kdev=_hist(rest, "kdev"), kmod=_hist(rest, "kmod"), kdiff=int(kdiff.group(1)) if kdiff else None)
    return out


# Largest error of each quotient estimate, from reasoning and the exact-integer search recorded in DESIGN.md 5b:
#   the 63-bit Shoup estimate 2 bh sh + ((bh sl + bl sh) >> 31) drops bl sl / 2^63 < 2, one floor < 1 and b frac(w 2^63 / q) / 2^63
#   < 1: at most 3 short, and 3 is attained with canonical operands at 60-bit moduli;
#   the one-word Barrett estimate loses frac(z / 2^k) 2^59 / q + floor(z / 2^k) frac(2^123 / q) / 2^64 < 2: at most 2 short; 2 is
#   attained at the first prime above 2^59 and (frac(2^123 / q) < 10^-3 for the primes of the default chain) never at those;
#   barrett128 forms floor(z floor(2^128 / q) / 2^128) exactly: at most 1 short, attained at every multiple of q;
#   the 64-bit Shoup estimate of a canonical operand is at most 1 short, and never short for q < 2^32.
SHOUP63_BLOCKS = ("shoup63_lazy", "shoup63", "divmod63", "shoup4", "ct_bfly", "gs_bfly") + tuple(
    "bfly<%s,%s,%s>" % (d, s, h) for d in ("fwd", "inv") for s in ("vec", "sc") for h in ("h1", "h2"))
SHOUP64_CANONICAL_BLOCKS = ("divmod_shoup", "divmod_shoup_u", "mul_shoup_lazy_u")
BARRETT128_BLOCKS = ("barrett128", "mulmod")
BARRETT_BLOCKS = ("reduce123", "reduce124", "reduce123_u", "colacc_reduce123_lazy", "colacc_reduce<false>", "colacc_reduce<true>",
                  "colacc123_to_4q")


def check_report(rep, must_have):
    """the assertions both tests make on a parsed report; `must_have`: blocks that have to be there for the default modulus"""
    assert rep, "no report lines"
    for b in must_have:
        assert any(k[0] == b for k in rep), "no line for block %s" % b
        if b in BARRETT_BLOCKS:   # the pinned bounds below must not pass for want of the edge primes
            assert (b, LOW_EDGE) in rep and (b, TOP_EDGE) in rep, "no line for block %s at an edge prime" % b
    for (block, q), r in sorted(rep.items()):
        where = "%s q=%d: %r" % (block, q, r)
        assert r["cases"] > 0 and r["fail"] == 0, where
        wide = (1 << 59) < q < (1 << 60)
        if block in SHOUP63_BLOCKS and wide:
            assert r["need"] == 3, where
        if block in BARRETT_BLOCKS and q == LOW_EDGE:
            assert r["need"] == 2, where
        if block in BARRETT_BLOCKS and q == TOP_EDGE:
            assert r["need"] == 1, where
        if block in BARRETT128_BLOCKS:
            assert r["need"] == 1, where
        if block in SHOUP64_CANONICAL_BLOCKS:
            assert r["need"] == (0 if q < (1 << 32) else 1), where
        if r["err"] is not None:    # every histogram printed is also required: no estimate goes unasserted
            assert r["need"] is not None, where
        if r["need"] is not None:
            assert min(r["err"][:r["need"] + 1]) >= MIN_COVER, where
            assert sum(r["err"][r["need"] + 1:]) == 0, where
        if r["kdev"] is not None:   # the multiple of q a lazy form leaves: the device's histogram is the host model's, case for case
            assert r["kdev"] == r["kmod"] and r["kdiff"] == 0, where
