"""Lazy representatives for the hand-offs of the product chain, and exact references of the kernels that take them (plain module,
imported by the test files; not a conftest).

The product chain hands residues from kernel to kernel without normalising them: a consumer documents a range -- [0, 4q) behind a
folded inverse transform, [0, 8q) behind a lazy forward transform, "< 2^63" for the word the key-switch MAC and the degree-2 finish
add into column 0 -- and a caller of the library controls the VALUE mod q of such a word but never which representative arrives.
Here the representatives are chosen: for a value r and a range end B, r + k q for every k with r + k q < B.

  values   0, 1, q - 1, q - 2; the two words below q whose 30-bit halves are full (full_halves); uniform in [q - 2^24, q) as in
           tests/test_gpu_long_sums.py; uniform
  tiling   position i of a limb holds value i % 8 of that list and multiple ks[(i / 8 + shift) % len(ks)], cut down to the largest
           multiple that keeps the word below B; the second half of a limb starts 11 positions further on, so that the members
           (n, n + N/2) of a folded pair hold different values and multiples; the last position of each half is B - 1 itself

Everything the references compute is exact integer arithmetic (Python integers in numpy object arrays); the transforms and the
base conversions are the oracle's.  Nothing is taken from the code under test.
"""
import numpy as np

GUARD = 64                      # words in front of and behind every output array of tests/lazy_inputs/main.cpp
FILL = 0xF1F1F1F1F1F1F1F1       # what those guards, and the places a mode does not write, hold
MASK30 = (1 << 30) - 1
VALUE_NAMES = ("0", "1", "q-1", "q-2", "h_lo", "h_hi", "near", "uni")
# the key-switch MAC's canonical operands: position i % 8 == 0 has full halves in EVERY digit and key word of the sum
DIG_NAMES = ("h_lo", "h_lo", "q-1", "h_hi", "near", "near", "h_lo", "uni")
KEY_NAMES = ("h_lo", "q-1", "h_lo", "h_hi", "near", "h_lo", "near", "uni")


# ---- madasm.h in plain integers ------------------------------------------------------------------------------------------------
def split30(x):
    """Split30 of madasm.h: (x mod 2^30, x >> 30)"""
    return x & MASK30, x >> 30


def colacc_mac(a, x, y):
    """colacc_mac of madasm.h on a = [c0, c1, c2], x and y split30 pairs -- without the wrap of a 64-bit word: the caller looks at the sizes"""
    a[0] += x[0] * y[0]
    a[1] += x[0] * y[1] + x[1] * y[0]
    a[2] += x[1] * y[1]


# ---- values and representatives ------------------------------------------------------------------------------------------------
def full_halves(q):
    """(the largest word below q whose low half is 2^30 - 1, the largest high half with low half 0)"""
    h = q >> 30
    lo_full = (h << 30) | MASK30
    if lo_full >= q:
        lo_full -= 1 << 30
    return lo_full, h << 30


def representatives(r, q, B):
    """r + k q for every k with r + k q < B"""
    return [r + k * q for k in range((B - 1 - r) // q + 1)]


def multiples(q, B):
    """the k that the tiling cycles through: every k up to (B - 1) / q, or -- where those are more than 17 (a narrow chain under
    2^63) -- the ends, the middle and the powers of two"""
    kmax = (B - 1) // q
    if kmax <= 16:
        return list(range(kmax + 1))
    ks = {0, 1, 2, 3, kmax // 2, kmax - 2, kmax - 1, kmax}
    ks.update(1 << s for s in range(2, kmax.bit_length()) if (1 << s) <= kmax)
    return sorted(ks)


def values(q, names, n, rng):
    """n canonical words: position i holds the value names[i % len(names)]"""
    h_lo, h_hi = full_halves(q)
    fixed = {"0": 0, "1": 1, "q-1": q - 1, "q-2": q - 2, "h_lo": h_lo, "h_hi": h_hi}
    out = np.empty(n, dtype=np.uint64)
    for s, name in enumerate(names):
        cnt = len(range(s, n, len(names)))
        if name == "near":
            out[s::len(names)] = np.uint64(q) - rng.integers(1, (1 << 24) + 1, cnt, dtype=np.uint64)
        elif name == "uni":
            out[s::len(names)] = rng.integers(0, q, cnt, dtype=np.uint64)
        else:
            out[s::len(names)] = np.uint64(fixed[name])
    return out


def lazy_limb(q, B, n, rng, shift=0):
    """(words, r, k), each [n]: words = r + k q < B as the module docstring tiles them over one limb of n positions"""
    assert q < B <= 1 << 63 and n % 2 == 0 and n >= 32
    h = n // 2
    ks = np.array(multiples(q, B), dtype=np.uint64)
    pos = np.concatenate([np.arange(h), np.arange(h) + 11])
    # (the values of the second half are drawn 11 positions further on: take n + 16 of them and index)
    r = values(q, VALUE_NAMES, n + 16, rng)[pos]
    k = ks[(pos // 8 + shift) % len(ks)]
    kcap = (np.uint64(B - 1) - r) // np.uint64(q)
    k = np.minimum(k, kcap)
    for last in (h - 1, n - 1):
        r[last], k[last] = (B - 1) % q, (B - 1) // q
    return r + k * np.uint64(q), r, k


def lazy_array(mods, B_of, shape, N, rng):
    """array shape + (len(mods), N): limb a of every polynomial lazy under B_of(q_a), the multiples shifted from polynomial to polynomial"""
    out = np.empty(tuple(shape) + (len(mods), N), dtype=np.uint64)
    for c, idx in enumerate(np.ndindex(*shape)):
        for a, q in enumerate(mods):
            out[idx + (a,)] = lazy_limb(int(q), B_of(int(q)), N, rng, shift=3 * c + a)[0]
    return out


def canon_array(mods, names, shape, N, rng):
    """array shape + (len(mods), N) of canonical words, limb a holding values(q_a, names)"""
    out = np.empty(tuple(shape) + (len(mods), N), dtype=np.uint64)
    for idx in np.ndindex(*shape):
        for a, q in enumerate(mods):
            out[idx + (a,)] = values(int(q), names, N, rng)
    return out


def uniform_array(mods, shape, N, rng):
    return canon_array(mods, ("uni",), shape, N, rng)


def obj(a):
    return np.asarray(a).astype(object)


def u64(a):
    return np.array(a, dtype=np.uint64)


# ---- operands of the key-switch MAC and the degree-2 finish -----------------------------------------------------------------------
TOP63 = (1 << 63) - 1
MASK_NAMES = ("q-1", "h_lo", "near", "uni")


def mac_operands(qs, ps, N, nb, G, nmask, rng, comps=2):
    """dict of the arrays of launch_relin_mac (comps = 2) or launch_deg2_finish (comps = 3) for nb rows:
      d01[nb][comps][L][N]  lazy under 2^63 -- every multiple of q below 8q and the ninth -- and 2^63 - 1 itself at every position
                            n = 0 (mod 64), beside full halves in every digit and key word
      dig[nb][L][L][N], key[G][L][2][L][N]   canonical: DIG_NAMES, KEY_NAMES
      eqp[nb][4][M][N]      lazy under 8q, all four operands
      mask[nmask][L][N]     canonical: MASK_NAMES"""
    qs, ps = [int(q) for q in qs], [int(p) for p in ps]
    L = len(qs)
    ops = {"d01": lazy_array(qs, lambda q: 1 << 63, (nb, comps), N, rng), "eqp": lazy_array(qs + ps, lambda q: 8 * q, (nb, 4), N, rng),
           "mask": canon_array(qs, MASK_NAMES, (nmask,), N, rng)}
    ops["d01"][..., 0::64] = np.uint64(TOP63)
    if comps == 2:
        ops["dig"] = canon_array(qs, DIG_NAMES, (nb, L), N, rng)
        ops["key"] = canon_array(qs, KEY_NAMES, (G, L, 2), N, rng)
    return ops


def mac_columns(d01, dig, key, j, c, v=0, whole=False):
    """the column accumulators of relin_mac_kernel for limb j, component c of one row, position by position, in plain integers:
    (column 0, column 1) as object arrays [N].  v: the own-limb term (an integer or an array), joined as its 30-bit halves as the
    kernel does, or -- whole -- added to column 0 in one piece"""
    L = dig.shape[0]
    a = [obj(d01[c, j]), 0, 0]
    for i in range(L):
        colacc_mac(a, split30(obj(dig[i, j])), split30(obj(key[i, c, j])))
    if whole:
        a[0] = a[0] + v
    else:
        lo, hi = split30(v)
        a[0], a[1] = a[0] + lo, a[1] + hi
    return a[0], a[1]


# ---- lane order ----------------------------------------------------------------------------------------------------------------
def lane_map(N, slice_len, T, kp):
    """lane-order position -> standard position for slices of slice_len coefficients, T threads per slice, kp coefficient pairs per
    thread: pair k of thread tau sits at k T + tau and belongs at kp tau + k (kernels_keyswitch.hip, relin_mac_kernel)"""
    assert 2 * kp * T == slice_len and N % slice_len == 0
    p = np.arange(N)
    pp = (p % slice_len) >> 1
    return ((p // slice_len) * slice_len + 2 * (kp * (pp % T) + pp // T) + (p & 1)).astype(np.int64)


# ---- exact references ------------------------------------------------------------------------------------------------------------
def ref_tensor(e, mods):
    """e[nb][4][M][N] (a0 a1 b0 b1) -> d[nb][3][M][N] = (a0 b0, a0 b1 + a1 b0, a1 b1) mod m, position by position"""
    nb, _, M, N = e.shape
    d = np.empty((nb, 3, M, N), dtype=np.uint64)
    for r in range(nb):
        for a, m in enumerate(mods):
            a0, a1, b0, b1 = (obj(e[r, s, a]) for s in range(4))
            d[r, 0, a], d[r, 1, a], d[r, 2, a] = u64(a0 * b0 % m), u64((a0 * b1 + a1 * b0) % m), u64(a1 * b1 % m)
    return d


def own_limb_consts(qs, ps, t):
    """c_j = [t P^-1]_{q_j}"""
    P = 1
    for p in ps:
        P *= int(p)
    return [int(t) % q * pow(P % q, -1, q) % q for q in qs]


def ref_mac_row(d01, dig, key, qs, eqp=None, cs=None):
    """one row of the key-switch MAC before the mask: (d01[c][j] + sum_i dig[i][j] key[i][c][j] [+ c_j (a (x) b)[c][j]]) mod q_j for
    d01[2][L][N], dig[L][L][N], key[L][2][L][N], eqp[4][M][N] -> [2][L][N]"""
    L, N = len(qs), d01.shape[-1]
    out = np.empty((2, L, N), dtype=np.uint64)
    for j, q in enumerate(qs):
        dg = [obj(dig[i, j]) for i in range(L)]
        if eqp is not None:
            a0, a1, b0, b1 = (obj(eqp[s, j]) for s in range(4))
            own = (a0 * b0, a0 * b1 + a1 * b0)
        for c in range(2):
            s = obj(d01[c, j])
            for i in range(L):
                s = s + dg[i] * obj(key[i, c, j])
            if eqp is not None:
                s = s + cs[j] * own[c]
            out[c, j] = u64(s % q)
    return out


def ref_deg2_row(d, eqp, qs, cs):
    """(d[c][j] + c_j (a (x) b)[c][j]) mod q_j for d[3][L][N], eqp[4][M][N] -> [3][L][N], before the mask"""
    L, N = len(qs), d.shape[-1]
    out = np.empty((3, L, N), dtype=np.uint64)
    for j, q in enumerate(qs):
        a0, a1, b0, b1 = (obj(eqp[s, j]) for s in range(4))
        for c, own in enumerate((a0 * b0, a0 * b1 + a1 * b0, a1 * b1)):
            out[c, j] = u64((obj(d[c, j]) + cs[j] * own) % q)
    return out


def mul_mask(x, mask, qs):
    """x[..][L][N] (.) mask[L][N] mod q_j"""
    out = np.empty_like(x)
    for j, q in enumerate(qs):
        out[..., j, :] = u64(obj(x[..., j, :]) * obj(mask[j]) % q)
    return out


# ---- the outer-stage fold ----------------------------------------------------------------------------------------------------------
def fold_w(o, a):
    """(q, psi^{N/2}) of modulus a of the oracle's chain (Q, then P)"""
    q = int(o.moduli[a])
    return q, pow(o.psi(a), o.N // 2, q)


def fold_load(limb, q, w):
    """what a fold_load consumer makes of limb[N] = (u | v): ((u + v) N^-1 | (u - v) psi^{-N/2} N^-1) mod q -- the coefficients"""
    N = len(limb)
    u, v = obj(limb[:N // 2]), obj(limb[N // 2:])
    ninv = pow(N, -1, q)
    return u64(np.concatenate([(u + v) * ninv % q, (u - v) * (pow(w, -1, q) * ninv % q) % q]))


def fold_store(limb, q, w):
    """what fold_store leaves of the coefficients limb[N] = (u | v): (u + v psi^{N/2} | u - v psi^{N/2}) mod q"""
    N = len(limb)
    u, v = obj(limb[:N // 2]), obj(limb[N // 2:])
    return u64(np.concatenate([(u + v * w) % q, (u - v * w) % q]))


def unfold_store(limb, q, w):
    """the coefficients behind a fold_store output limb[N] = (y0 | y1): ((y0 + y1) / 2 | (y0 - y1) / (2 psi^{N/2})) mod q"""
    N = len(limb)
    y0, y1 = obj(limb[:N // 2]), obj(limb[N // 2:])
    i2 = pow(2, -1, q)
    return u64(np.concatenate([(y0 + y1) * i2 % q, (y0 - y1) * (i2 * pow(w, -1, q) % q) % q]))


def fold_load_poly(o, poly, first=0):
    """fold_load limb by limb for poly[n][N], limb i under modulus first + i"""
    return np.stack([fold_load(poly[i], *fold_w(o, first + i)) for i in range(poly.shape[0])])


def unfold_store_poly(o, poly, first=0):
    return np.stack([unfold_store(poly[i], *fold_w(o, first + i)) for i in range(poly.shape[0])])


def fold_store_poly(o, poly, first=0):
    return np.stack([fold_store(poly[i], *fold_w(o, first + i)) for i in range(poly.shape[0])])
