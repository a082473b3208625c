"""Exact-integer model of the butterflies for q = 2^60 - d, d < 2^27 (csrc/ntt16_kernel.h at ArithKind::fold), and the operand families
their tests share (plain module, imported by the test files; not a conftest).

Everything the blocks compute is arithmetic mod 2^64 on values whose true size is known, so the model works on Python integers and
asserts the sizes as it goes: a result that would wrap where the block's derivation says it cannot is an error of the model's
caller, not a value to compare with."""
import random

M32, W64 = (1 << 32) - 1, 1 << 64
P60 = 1 << 60
T = P60 + (1 << 31)     # fold(x) < 2^60 + 15 (2^27 - 1) < T for every 64-bit x


def fold(x, q):
    d = P60 - q
    assert 0 < d < (1 << 27) and 0 <= x < W64
    return (x & (P60 - 1)) + (x >> 60) * d


def shoup(q, b, w):
    """b w - qe q with the 63-bit estimate qe = 2 bh sh + ((bh sl + bl sh) >> 31), s = floor(w 2^63 / q): b w mod q plus at most 3q"""
    assert 0 <= b < (1 << 63) and 0 <= w < q
    s = (w << 63) // q
    bl, bh, sl, sh = b & M32, b >> 32, s & M32, s >> 32
    qe = 2 * bh * sh + ((bh * sl + bl * sh) >> 31)
    v = b * w - qe * q
    assert 0 <= v < 4 * q and v % q == b * w % q
    return v


def shoup_error(q, b, w):
    return shoup(q, b, w) // q


def block(kind, q, a, b, w):
    """(a', b') of one block: "ctf" forward, "gsf" inverse with the fold, "gsn" inverse without"""
    if kind == "ctf":
        u = fold(a, q)
        v = shoup(q, b, w)
        assert 2 * u + 4 * q < W64
        return u + v, u + 4 * q - v
    assert a < 4 * q and b < 4 * q
    dd = a + 4 * q - b
    assert 0 < dd < 8 * q
    if kind == "gsf":
        return fold(a + b, q), shoup(q, dd, w)
    assert kind == "gsn" and a < T and b < T
    return a + b, shoup(q, dd, w)


def forward_a_edges(q):
    """the forward block's first operand: the ends of [0, 8q), of the fold's own pieces, and of 64 bits (the fold takes any word)"""
    return [0, P60 - 1, P60, T - 1, 4 * q - 1, 4 * q, 8 * q - 1, (1 << 63) - 1, W64 - 1]


def directed_ws(q, count, seed=5):
    """twiddles whose floor(w 2^63 / q) has a low word within 2^8 of 2^32 - 1: with a multiplicand of the same shape the dropped
    product bl sl and the two floors leave the estimate 3 short (tests/arith_check/check.h: directed_w)"""
    rng = random.Random(seed * 1000003 + q % 1000003)
    out = []
    while len(out) < count:
        # s = floor(w 2^63 / q) with a chosen low word: w = ceil(s q / 2^63)
        s = (rng.randrange(1 << 30, 1 << 31) << 32) | (M32 - rng.randrange(256))
        w = -((-s * q) >> 63)
        if 0 < w < q and ((w << 63) // q) & M32 >= M32 - 255:
            out.append(w)
    return out


def directed_bs(q, w, lim, tries=4096, seed=9):
    """multiplicands below `lim` with a low word within 2^8 of 2^32 - 1, those first whose estimate against w is 3 short"""
    rng = random.Random(seed * 1000003 + w % 1000003)
    bs = [(rng.randrange(lim >> 32) << 32) | (M32 - rng.randrange(256)) for _ in range(tries)]
    bs = [b for b in bs if b < lim]
    bs.sort(key=lambda b: -shoup_error(q, b, w))
    return bs
