"""Crafted COEFFICIENT-form columns for the base conversions, the digit lifts and the client's decryption (plain module,
imported by the test files; not a conftest).

A column is the tuple of residues of one coefficient: L of them over Q, or M = 2L + 1 over QP.  The HPS base conversions and the BV
digit lift work on such columns, and they branch and round at places that uniform residues reach with negligible probability:

  digit extremes  the CRT digits y_i = x_i (Q/q_i)^-1 mod q_i at 0, q_i - 1, (q_i - 1)/2 and one-hot: the largest dot products, quotients
                  and rounding counts the conversion kernels can meet
  ties            the exact pre-rounding value sits k units of 2^-60 from a half-integer (the kernels round a sum of truncated 60-bit
                  fractions, (fsum + 2^59) >> 60)
  lift windows    residue limb i at q_j - 1, q_j, q_j + 1, q_i - 1, (q_i +- 1)/2, q_i mod q_j: where the lift of a residue mod q_i into
                  q_j subtracts, wraps and changes sign
  message edges   neighbouring phases x on either side of a step of round(t x/Q): decryption's result changes there, at the messages
                  where it wraps (t -> 0) and where the decoded slot changes sign ((t - 1)/2, (t + 1)/2)
  limb drops      the residue dropped at EVERY step of a drop of several limbs at 0, +-1 and +-(q_l - 1)/2 (the derived residues, not only
                  those given), kept residues at 0 and q_i - 1 in front of a step, and the result of the drop on the level's own edges

and, for the client's encryption, message coefficients m that put [Q m]_t on the branches of the message term.

Everything here is exact integer arithmetic (oracle/exact.py); `o` is an oracle context (oracle.binding.Oracle).
"""
from fractions import Fraction

import numpy as np

from oracle import exact as ex

TIE_KS = (0, 1, -1, 2, -2, 3, -3, 4, -4)   # ... and +-L, +-(2L + 2), +-64, +-2^10: tie_ks(L)


def tie_ks(L):
    """the distances, in units of 2^-60, at which the tie families place a column"""
    ks = list(TIE_KS)
    for k in (L, 2 * L + 2, 64, 1 << 10):
        for s in (k, -k):
            if s not in ks:
                ks.append(s)
    return ks


def moduli(o):
    return [int(v) for v in o.q], [int(v) for v in o.p]


class Families(dict):
    """family name -> list of columns, all over `moduli`"""

    def __init__(self, mods, *args, **kw):
        super().__init__(*args, **kw)
        self.moduli = tuple(int(m) for m in mods)

    def count(self):
        return sum(len(v) for v in self.values())


def reduce_col(x, mods):
    return tuple(int(x % m) for m in mods)


# ---- digit extremes ------------------------------------------------------------------------------------------------------------
def digit_sets(mods):
    """the CRT digit vectors y: all m_i - 1, all 0, one-hot m_i - 1 for every i, all (m_i - 1)/2"""
    n = len(mods)
    ys = [tuple(m - 1 for m in mods), tuple(0 for _ in mods)]
    ys += [tuple(mods[i] - 1 if j == i else 0 for j in range(n)) for i in range(n)]
    ys.append(tuple((m - 1) // 2 for m in mods))
    return ys


def digit_extremes(mods):
    """columns x with x_i = y_i (Mod/m_i) mod m_i, so that x_i (Mod/m_i)^-1 mod m_i = y_i, for the y of digit_sets"""
    Mod = ex.prod(mods)
    return [tuple(y * ((Mod // m) % m) % m for y, m in zip(ys, mods)) for ys in digit_sets(mods)]


def digits_of(col, mods):
    """the CRT digits of a column: y_i = x_i (Mod/m_i)^-1 mod m_i"""
    Mod = ex.prod(mods)
    return tuple(int(x) * pow((Mod // m) % m, -1, m) % m for x, m in zip(col, mods))


# ---- ties ----------------------------------------------------------------------------------------------------------------------
def tie_distance(num, den):
    """distance of num/den from the nearest half-integer, in units of 2^-60 (a Fraction)"""
    f = Fraction(num % den, den)
    return abs(f - Fraction(1, 2)) * (1 << 60)


def tie_unit(M):
    """2^-60 of M in integers: the step between neighbouring tie columns (one, where M itself is below 2^60: a chain of one limb)"""
    return max(1, M >> 60)


def ties_expand(o):
    """{label: x in [0, Q)}: x/Q is k units from 1/2 -- the rounding of the centred lift out of Q (expand) and, through
    round(P x/Q)/P, of the lift out of P (second rounding of scale_pq).  Labels: the integer k, or 'floor', 'floor+1', 'x=0', 'x=1', 'x=-1'"""
    qs, _ = moduli(o)
    Q = ex.prod(qs)
    u = tie_unit(Q)
    out = {"floor": Q // 2, "floor+1": Q // 2 + 1, "x=0": 0, "x=1": 1, "x=-1": Q - 1}
    for k in tie_ks(len(qs)):
        out[k] = (Q // 2 + k * u) % Q
    return out


def ties_scale_first(o):
    """{label: x}: P x mod Q is k units (of Q 2^-60) from Q/2 -- the first rounding of scale_pq, round(P x/Q)"""
    qs, ps = moduli(o)
    Q, P = ex.prod(qs), ex.prod(ps)
    u = tie_unit(Q)
    Pinv = pow(P % Q, -1, Q)
    out = {"floor": (Q - 1) // 2 * Pinv % Q, "floor+1": (Q + 1) // 2 * Pinv % Q}
    for k in tie_ks(len(qs)):
        out[k] = ((Q - 1) // 2 + k * u) * Pinv % Q
    return out


def ties_scale_round(o, rng):
    """{label: d in [0, QP)}: t d mod P is k units (of P 2^-60) from P/2 -- the rounding of round(t d/P); d = x + r P with r uniform"""
    qs, ps = moduli(o)
    Q, P = ex.prod(qs), ex.prod(ps)
    u = tie_unit(P)
    tinv = pow(o.t % P, -1, P)

    def lift(x):
        r = int.from_bytes(rng.bytes((Q.bit_length() + 7) // 8 + 8), "little") % Q
        return x + r * P
    out = {"floor": lift((P - 1) // 2 * tinv % P), "floor+1": lift((P + 1) // 2 * tinv % P), "x=0": 0, "x=1": 1, "x=-1": Q * P - 1}
    for k in tie_ks(len(qs)):
        out[k] = lift(((P - 1) // 2 + k * u) * tinv % P)
    return out


def ties_decrypt(o):
    """{label: x in [0, Q)}: t x mod Q is k units (of Q 2^-60) from Q/2 -- the rounding of decryption, round(t x/Q) mod t.  Labels as in
    ties_expand"""
    qs, _ = moduli(o)
    Q = ex.prod(qs)
    u = tie_unit(Q)
    tinv = pow(o.t % Q, -1, Q)
    out = {"floor": (Q - 1) // 2 * tinv % Q, "floor+1": (Q + 1) // 2 * tinv % Q, "x=0": 0, "x=1": 1, "x=-1": Q - 1}
    for k in tie_ks(len(qs)):
        out[k] = ((Q - 1) // 2 + k * u) * tinv % Q
    return out


def message_edge_values(t):
    """the messages at whose lower edge message_edges places a pair: 1, the two around t/2 where the decoded slot changes sign, t - 1, and
    t itself -- round(t x/Q) = t for x just below Q, which is message 0"""
    return [1, (t - 1) // 2, (t + 1) // 2, t - 1, t]


def message_edges(o):
    """{(m, 'below'): x0 - 1, (m, 'at'): x0} for the m of message_edge_values: x0 = ceil((2m - 1) Q / 2t) is the smallest x with
    round(t x/Q) = m, so the pair rounds to m - 1 and m"""
    qs, _ = moduli(o)
    Q, t = ex.prod(qs), o.t
    out = {}
    for m in message_edge_values(t):
        x0 = -(-(2 * m - 1) * Q // (2 * t))
        out[(m, "below")] = (x0 - 1) % Q
        out[(m, "at")] = x0 % Q
    return out


# ---- lift windows --------------------------------------------------------------------------------------------------------------
def window_values(qs, i):
    """values of residue limb i that sit at the edges of its lifts into the other moduli"""
    qi = qs[i]
    vals = [qi - 1, (qi - 1) // 2, (qi + 1) // 2, 0, 1]
    for j, qj in enumerate(qs):
        if j == i or qj >= qi:
            continue
        vals += [qj - 1, qj, qj + 1, qi % qj]
        if qi >= 2 * qj:   # the Barrett branch of the lift: multiples of q_j below q_i
            for m in (1, 2, qi // qj):
                vals += [m * qj - 1, m * qj, m * qj + 1]
    out = []
    for v in vals:
        if 0 <= v < qi and v not in out:
            out.append(v)
    return out


def lift_windows(qs):
    """columns whose limb i cycles through window_values(qs, i): every column carries a window value in every limb"""
    per = [window_values(qs, i) for i in range(len(qs))]
    n = max(len(v) for v in per)
    return [tuple(per[i][(c + i) % len(per[i])] for i in range(len(qs))) for c in range(n)]


def lift_definition(v, qi, qj):
    """the BV digit of residue v mod q_i in limb j: centred(v, q_i) mod q_j"""
    return ex.centered(v, qi) % qj


# ---- families ------------------------------------------------------------------------------------------------------------------
def q_families(o):
    """all families over Q (inputs of expand and scale_pq, and residue columns for the digit lifts)"""
    qs, _ = moduli(o)
    f = Families(qs)
    f["digits"] = digit_extremes(qs)
    f["ties_expand"] = [reduce_col(x, qs) for x in ties_expand(o).values()]
    f["ties_scale_first"] = [reduce_col(x, qs) for x in ties_scale_first(o).values()]
    f["windows"] = lift_windows(qs)
    return f


def qp_families(o, rng):
    """all families over QP (inputs of scale-and-round)"""
    qs, ps = moduli(o)
    mods = qs + ps
    f = Families(mods)
    f["digits"] = digit_extremes(mods)
    f["ties_scale_round"] = [reduce_col(x, mods) for x in ties_scale_round(o, rng).values()]
    return f


def window_families(o):
    qs, _ = moduli(o)
    f = Families(qs)
    f["windows"] = lift_windows(qs)
    f["digits"] = digit_extremes(qs)
    return f


def decrypt_families(o):
    """all families over Q for the rounding of decryption: phases, COEFFICIENT columns of c0 + c1 s (+ c2 s^2)"""
    qs, _ = moduli(o)
    f = Families(qs)
    f["digits"] = digit_extremes(qs)
    f["windows"] = lift_windows(qs)
    f["ties_decrypt"] = [reduce_col(x, qs) for x in ties_decrypt(o).values()]
    f["message_edges"] = [reduce_col(x, qs) for x in message_edges(o).values()]
    return f


# ---- the limb drop ---------------------------------------------------------------------------------------------------------------
# The drop of limb l (tests/test_result_limbs.py) takes r = c mod q_l centred and leaves (c - r) / q_l, a number modulo q_0 .. q_{l-1}.
# It branches on c_l > (q_l - 1)/2, and its kernels form c_i - r as one unsigned word whose ends are met only when c_i is 0 or
# q_i - 1 while c_l sits at the branch.  The columns below are built backwards from what the drop is to meet at every step.
def undrop(y, l_from, qs, rs):
    """the column over qs of the c with  c <- (c q_l + r_l) mod (q_0 .. q_l)  for l = l_from .. L - 1, from c = y, an integer modulo
    q_0 .. q_{l_from - 1}; rs[l] is a centred residue, |rs[l]| <= (q_l - 1)/2 (a list of length L, or a dict, indexed by l).
    Dropping the limbs L - 1 .. l_from from the column by the definition gives back y, and the residue dropped at step l is
    rs[l] mod q_l"""
    qs = [int(q) for q in qs]
    c = int(y) % ex.prod(qs[:l_from])
    for l in range(l_from, len(qs)):
        r = int(rs[l])
        assert 2 * abs(r) <= qs[l] - 1
        c = (c * qs[l] + r) % ex.prod(qs[:l + 1])
    return reduce_col(c, qs)


def drop_patterns(qs, Lc):
    """the patterns of dropped residues r (dicts l -> r_l over the dropped limbs Lc .. L - 1) that drop_families cycles through: every
    dropped limb at the same element of {0, 1, -1, half, -half}; each limb alone at +-half or +-1, the others at 0; the two
    alternations of +half / -half (half = (q_l - 1)/2: +half is the largest residue that counts as positive, -half = (q_l + 1)/2 mod
    q_l the smallest that counts as negative)"""
    qs = [int(q) for q in qs]
    D = list(range(Lc, len(qs)))
    half = {l: (qs[l] - 1) // 2 for l in D}
    pats = [{l: 0 for l in D}, {l: 1 for l in D}, {l: -1 for l in D}, {l: half[l] for l in D}, {l: -half[l] for l in D}]
    for l in D:
        for v in (half[l], -half[l], 1, -1):
            pats.append({j: v if j == l else 0 for j in D})
    for first in (1, -1):
        pats.append({l: first * (-1) ** (l - Lc) * half[l] for l in D})
    out = []
    for p in pats:
        if p not in out:
            out.append(p)
    return out


def drop_families(o, ol, Lc):
    """Families over the parent's q for the drop of the limbs L - 1 .. Lc (ol: the level oracle of the first Lc limbs):

      final  y undropped with one pattern of drop_patterns, cycling; y runs over the CRT values of every column of q_families(ol) --
             digit extremes, ties and windows of the LEVEL, so that the level's expand / scale_pq meet their own edges behind the drop --
             and 0, 1, Q_Lc - 1.  As many columns as the longer of the two lists
      kept   for every dropped limb l the state just before its drop -- residues i < l all 0 or all q_i - 1, limb l at 0, (q_l - 1)/2,
             (q_l + 1)/2, q_l - 1 -- undropped through the limbs above l with r = 0 and with r = (q_j - 1)/2

    .claims[family][k] says what column k was built from: (y, pattern) for final; (l, state, pattern) for kept, state the residues
    0 .. l in front of step l"""
    qs, _ = moduli(o)
    L = len(qs)
    assert 1 <= Lc < L and [int(v) for v in ol.q] == qs[:Lc]
    QLc = ex.prod(qs[:Lc])
    lvl = q_families(ol)
    ys = [ex.crt(col, qs[:Lc]) for cols in lvl.values() for col in cols] + [0, 1, QLc - 1]
    pats = drop_patterns(qs, Lc)
    f = Families(qs)
    f.claims = {"final": [], "kept": []}
    f["final"], f["kept"] = [], []
    for k in range(max(len(ys), len(pats))):
        y, pat = ys[k % len(ys)], pats[k % len(pats)]
        f["final"].append(undrop(y, Lc, qs, pat))
        f.claims["final"].append((y, pat))
    for l in range(Lc, L):
        ql = qs[l]
        for low in (0, 1):
            for vl in (0, (ql - 1) // 2, (ql + 1) // 2, ql - 1):
                state = tuple(0 if low == 0 else qs[i] - 1 for i in range(l)) + (vl,)
                x = ex.crt(state, qs[:l + 1])
                for top in ((0, 1) if l + 1 < L else (0,)):
                    pat = {j: top * ((qs[j] - 1) // 2) for j in range(l + 1, L)}
                    f["kept"].append(undrop(x, l + 1, qs, pat))
                    f.claims["kept"].append((l, state, pat))
    return f


# ---- placing columns in a polynomial ---------------------------------------------------------------------------------------------
def tile_map(fam, N):
    """{coefficient index: (family, column)}: the columns, families interleaved, at n = 0, 1, 2, .. and again -- from another family --
    at N/2 + n, so that the two members (n, n + N/2) of a folded pair hold different families; the last two coefficients of each
    half (N/2 - 2, N/2 - 1, N - 2, N - 1) are crafted as well"""
    lists = [[(name, c) for c in cols] for name, cols in fam.items() if cols]
    entries = []
    for r in range(max(len(v) for v in lists)):
        entries += [v[r] for v in lists if r < len(v)]
    C, h = len(entries), N // 2
    if C + 2 > h:
        raise ValueError("%d columns do not fit a half of %d coefficients" % (C, h))
    out = {}
    for n in list(range(C)) + [h - 2, h - 1]:
        e = n if n < C else n - (h - 2)
        out[n] = entries[e]
        s = 1
        while s < C and entries[(e + s) % C][0] == entries[e][0]:
            s += 1
        out[n + h] = entries[(e + s) % C]
    return out


def uniform_poly(mods, N, rng):
    return np.stack([rng.integers(0, m, N, dtype=np.uint64) for m in mods])


def tile(fam, N, rng):
    """polynomial [len(moduli)][N]: the columns of `fam` where tile_map puts them, uniform residues elsewhere"""
    poly = uniform_poly(fam.moduli, N, rng)
    for n, (_, col) in tile_map(fam, N).items():
        poly[:, n] = np.array(col, dtype=np.uint64)
    return poly


def columns_poly(cols, mods, N):
    """polynomial [len(mods)][N] with the columns at n = 0, 1, .. and zeros behind them (len(cols) <= N)"""
    poly = np.zeros((len(mods), N), dtype=np.uint64)
    for n, col in enumerate(cols):
        poly[:, n] = np.array(col, dtype=np.uint64)
    return poly


def cols_of(arr):
    return [tuple(int(v) for v in arr[:, n]) for n in range(arr.shape[1])]


def sigma(poly, g, mods):
    """a(X) -> a(X^g) mod X^N + 1, limb by limb, for poly [len(mods)][N]"""
    N = poly.shape[1]
    k = np.arange(N, dtype=np.int64) * int(g) % (2 * N)
    dst, neg = k % N, k >= N
    out = np.empty_like(poly)
    for l, m in enumerate(mods):
        v = poly[l]
        out[l, dst] = np.where(neg & (v != 0), np.uint64(m) - v, v)
    return out


def ntt_q(o, poly):
    return np.stack([o.ntt(i, poly[i]) for i in range(poly.shape[0])])


def intt_q(o, poly):
    return np.stack([o.intt(i, poly[i]) for i in range(poly.shape[0])])


# ---- crafted messages and ciphertexts of a given phase ---------------------------------------------------------------------------
def message_rrs(t):
    """the values of rr = [Q m]_t that enc_message_coeffs cycles through: encryption adds -rr/t or (t - rr)/t according to rr <= t/2,
    and nothing at all for rr = 0"""
    h = (t - 1) // 2
    return [0, 1, 2, h - 1, h, h + 1, h + 2, t - 2, t - 1]


def enc_message_coeffs(o, n):
    """n message coefficients m_i = rr_i (Q mod t)^-1 mod t, rr_i cycling through message_rrs(t): [Q m_i]_t = rr_i"""
    qs, _ = moduli(o)
    t = o.t
    Qinv = pow(ex.prod(qs) % t, -1, t)
    rrs = message_rrs(t)
    return np.array([rrs[i % len(rrs)] * Qinv % t for i in range(n)], dtype=np.uint64)


def mulmod_rows(a, b, mods):
    """a b limb by limb for [len(mods)][N] arrays, with Python integers"""
    return np.stack([np.array([int(x) * int(y) % int(m) for x, y in zip(ra, rb)], dtype=np.uint64) for ra, rb, m in zip(a, b, mods)])


def phase_ct(o, X, sk=None, c1=None, c2=None):
    """the ciphertext [2 or 3][L][N] (EVALUATION) whose phase c0 + c1 s + c2 s^2 is the COEFFICIENT polynomial X [L][N]: c0 = NTT(X) -
    c1 s - c2 s^2, from c1 (and c2) in EVALUATION form and the key sk.  Without c1 the phase is X under any key"""
    qs, _ = moduli(o)
    c0 = ntt_q(o, np.ascontiguousarray(X, dtype=np.uint64))
    if c1 is None:
        assert c2 is None
        return np.stack([c0, np.zeros_like(c0)])
    comps = [c1] if c2 is None else [c1, c2]
    spow = sk
    for c in comps:
        cs = mulmod_rows(c, spow, qs)
        c0 = np.stack([np.array([(int(x) - int(y)) % q for x, y in zip(c0[i], cs[i])], dtype=np.uint64) for i, q in enumerate(qs)])
        spow = mulmod_rows(spow, sk, qs)
    return np.stack([c0] + [np.ascontiguousarray(c, dtype=np.uint64) for c in comps])


def columns_polys(cols, mods, N):
    """the columns in as many polynomials [len(mods)][N] as they need: [ceil(len(cols) / N)][len(mods)][N], zeros behind the last"""
    return np.stack([columns_poly(cols[s:s + N], mods, N) for s in range(0, len(cols), N)])


# ---- steering d2 of a product --------------------------------------------------------------------------------------------------
def d2_constant(o):
    """c = floor(Q/t): with a1 the constant polynomial c, d2 = a1 (x) b1 is coefficient-wise in b1"""
    qs, _ = moduli(o)
    return ex.prod(qs) // o.t


def exact_d2(o, b):
    """coefficient of d2 = round(t c round(P b/Q) / P) mod Q for the centred coefficient b of b1 and a1 = c"""
    qs, ps = moduli(o)
    Q, P = ex.prod(qs), ex.prod(ps)
    return ex.rnd_div(o.t * d2_constant(o) * ex.rnd_div(P * b, Q), P) % Q


def solve_d2(o, targets, reach=8):
    """for every target column (L residues) a centred coefficient b with exact_d2(o, b) = CRT(target), or None where the search over
    round(D Q/(t c)) +- reach finds none"""
    qs, _ = moduli(o)
    Q = ex.prod(qs)
    tc = o.t * d2_constant(o)
    out = []
    for col in targets:
        D = ex.crt(col, qs)
        b0 = ex.rnd_div(ex.centered(D, Q) * Q, tc)
        hit = None
        for d in sorted(range(-reach, reach + 1), key=abs):
            b = b0 + d
            if 2 * abs(b) < Q and exact_d2(o, b) == D:
                hit = b
                break
        out.append(hit)
    return out


def d2_operands(o, targets, rng):
    """EVALUATION ciphertexts (a, b), each [2][L][N], whose tensor product has the target columns as coefficients 0, 1, .. of d2,
    cycled over all N coefficients: a1 = c, b1 from solve_d2, a0 and b0 uniform"""
    qs, _ = moduli(o)
    N = o.N
    bs = solve_d2(o, targets)
    assert None not in bs, "solve_d2 missed %d of %d targets" % (bs.count(None), len(bs))
    c = d2_constant(o)
    a1 = np.zeros((len(qs), N), dtype=np.uint64)
    b1 = np.zeros((len(qs), N), dtype=np.uint64)
    for i, q in enumerate(qs):
        a1[i, 0] = c % q
        b1[i] = np.array([bs[n % len(bs)] % q for n in range(N)], dtype=np.uint64)
    a = np.stack([ntt_q(o, uniform_poly(qs, N, rng)), ntt_q(o, a1)])
    b = np.stack([ntt_q(o, uniform_poly(qs, N, rng)), ntt_q(o, b1)])
    return a, b
