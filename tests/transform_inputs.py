"""Crafted inputs for the transform launches themselves (plain module, imported by the test files; not a conftest).

tests/lazy_inputs.py chooses the REPRESENTATIVE a kernel is handed; this module chooses the VALUES a transform is handed, so that its
butterflies meet operand coincidences that uniform data produces with negligible probability.  Every family is canonical, one limb
of N words, written in the order the transform's first stage reads: COEFFICIENT natural order for a forward transform, EVALUATION
standard (bit-reversed) order for an inverse one (a lane-ordered launch gets the same limb permuted by the handle's map).

  const c      every word c, c in {1, (q - 1)/2, q - 1}, plus a small tag per (limb, half): the Gentleman-Sande butterflies of the
               first inverse stage (distance 1) all meet a = b, i.e. a - b + 4q = 4q exactly
  delta v p    zeros and one word v in {1, q - 1} at p in {0, 1, N/2 - 1, N/2, N - 1}
  alt s        IN FRONT OF THE STAGE WHOSE BUTTERFLIES ARE s APART the residues are 0 and q - 1 in runs of s, the second half of the
               limb with the runs swapped: that stage meets the pairs (0, q - 1) and (q - 1, 0).  For the first stage of a direction
               (s = N/2 forward, s = 1 inverse) the limb itself is that pattern; for every other s the pattern is carried back through the
               stages in front (plain runs of 0 and q - 1 in the INPUT do not survive one stage: tests/test_transform_inputs.py shows what
               they turn into, and that this family is where it claims).  s = N/2 has one pair per limb: two limbs, alt N/2 and alt N/2 swapped
  max          every word q - 1: the sum path of the inverse doubles it stage by stage, 2^s (q - 1), across the 4q threshold of its
               mod+ block and then a few units below 8q in front of every later one
  near         distinct words, uniform in [q - 2^24, q)
  rand         uniform

The stage networks below are the textbook ones with the oracle's twiddle tables (o.twiddles), canonical residues throughout:
forward Cooley-Tukey, stage with m groups and distance t = N/(2m): (a, b) -> (a + w b, a - w b), w = tw[m + group]; inverse
Gentleman-Sande, stage with h groups and distance t = N/(2h): (a, b) -> (a + b, (a - b) w), w = itw[h + group], N^-1 at the end.
tests/test_transform_inputs.py pins them to the oracle's ntt / intt.  Two arithmetics: Python integers (`exact=True`: what the CPU
test argues with) and uint64 words with a long-double quotient estimate and two corrections (what the GPU test crafts its arrays with
in milliseconds; the CPU test holds it against the first).  No reference is computed here: those are the oracle's transforms.
"""
import functools

import numpy as np

from tests import lazy_inputs as lz

_LD_OK = np.finfo(np.longdouble).nmant >= 63   # an x87 extended double: the quotient estimate is off by at most one


# ---- a b mod q on arrays ---------------------------------------------------------------------------------------------------------
def mulmod(a, b, q, exact=False):
    """a b mod q for uint64 arrays below q < 2^61"""
    if exact or not _LD_OK:
        return lz.u64(lz.obj(a) * lz.obj(b) % int(q))
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    qe = np.floor(a.astype(np.longdouble) * b.astype(np.longdouble) / np.longdouble(q)).astype(np.uint64)
    with np.errstate(over="ignore"):
        r = (a * b - qe * np.uint64(q)).astype(np.int64)   # mod 2^64: the true remainder lies in (-q, 2q)
    r = np.where(r < 0, r + np.int64(q), r)
    r = np.where(r >= np.int64(q), r - np.int64(q), r)
    return r.astype(np.uint64)


def addmod(a, b, q):
    s = np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)
    return np.where(s >= np.uint64(q), s - np.uint64(q), s)


def submod(a, b, q):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return np.where(a >= b, a - b, a + np.uint64(q) - b)


# ---- the stage networks ------------------------------------------------------------------------------------------------------------
class Stages:
    """the two networks of one modulus of an oracle context"""

    def __init__(self, o, mi, exact=False):
        self.N, self.q, self.exact = o.N, int(o.moduli[mi]), exact
        self.tw, self.itw = o.twiddles(mi)
        q = self.q
        self.tw_inv = lz.u64([pow(int(w), -1, q) for w in self.tw[1:]])      # (index 0 of the tables is not a twiddle)
        self.itw_inv = lz.u64([pow(int(w), -1, q) for w in self.itw[1:]])
        self.inv2, self.n_inv = pow(2, -1, q), pow(o.N, -1, q)

    def _mul(self, a, b):
        return mulmod(a, b, self.q, self.exact)

    def distances(self, inverse):
        """the butterfly distance of every stage, in the order the direction runs them"""
        logN = self.N.bit_length() - 1
        return [1 << k for k in range(logN)] if inverse else [self.N >> (k + 1) for k in range(logN)]

    def stage(self, x, t, inverse, back=False):
        """one stage with distance t on x[N] (a new array); back: the stage undone"""
        N, q = self.N, self.q
        g = N // (2 * t)
        X = np.asarray(x, dtype=np.uint64).reshape(g, 2, t)
        a, b = X[:, 0, :], X[:, 1, :]
        out = np.empty_like(X)
        if not inverse:
            if not back:
                v = self._mul(b, self.tw[g:2 * g, None])
                out[:, 0, :], out[:, 1, :] = addmod(a, v, q), submod(a, v, q)
            else:   # a = (a' + b') / 2, b = (a' - b') / (2 w)
                out[:, 0, :] = self._mul(addmod(a, b, q), np.uint64(self.inv2))
                out[:, 1, :] = self._mul(self._mul(submod(a, b, q), np.uint64(self.inv2)), self.tw_inv[g - 1:2 * g - 1, None])
        else:
            if not back:
                out[:, 0, :], out[:, 1, :] = addmod(a, b, q), self._mul(submod(a, b, q), self.itw[g:2 * g, None])
            else:   # d = b' / w: a = (a' + d) / 2, b = (a' - d) / 2
                d = self._mul(b, self.itw_inv[g - 1:2 * g - 1, None])
                out[:, 0, :] = self._mul(addmod(a, d, q), np.uint64(self.inv2))
                out[:, 1, :] = self._mul(submod(a, d, q), np.uint64(self.inv2))
        return out.reshape(N)

    def run(self, x, inverse, until=None, first=0):
        """the network from its stage number `first` on, up to (not including) the stage with distance `until`; all of it, and the
        inverse's N^-1, where until is None"""
        x = np.asarray(x, dtype=np.uint64)
        for t in self.distances(inverse)[first:]:
            if t == until:
                return x
            x = self.stage(x, t, inverse)
        assert until is None
        return self._mul(x, np.uint64(self.n_inv)) if inverse else x

    def carry_back(self, y, inverse, s, first=0):
        """the input whose residues in front of the stage with distance s are y (the network entered at stage number `first`)"""
        ds = self.distances(inverse)[first:]
        x = np.asarray(y, dtype=np.uint64)
        for t in reversed(ds[:ds.index(s)]):
            x = self.stage(x, t, inverse, back=True)
        return x


# ---- the families ------------------------------------------------------------------------------------------------------------------
def alt_pattern(q, N, s, swapped=False):
    """0 and q - 1 in runs of s, the runs swapped in the second half of the limb (s < N/2), or everywhere (swapped)"""
    j = np.arange(N)
    odd = (j // s) & 1
    if s < N // 2:
        odd = odd ^ (j >= N // 2)
    if swapped:
        odd = odd ^ 1
    return np.where(odd == 1, np.uint64(q - 1), np.uint64(0))


def specs(N, inverse, first=0):
    """the families of one direction, in the order the limbs of a launch take them; first: leading stages the launch does not run
    (a folded forward transform enters at stage 1: no alt N/2)"""
    out = [("max",), ("const", "q-1"), ("const", "1"), ("const", "half")]
    ds = [1 << k for k in range(N.bit_length() - 1)]
    if not inverse:
        ds = ds[:len(ds) - first][::-1]
    alts = [("alt", s, False) for s in ds]
    if N // 2 in ds:
        alts.append(("alt", N // 2, True))
    deltas = [("delta", v, p) for v in ("1", "q-1") for p in (0, 1, N // 2 - 1, N // 2, N - 1)]
    out += alts[:2] + [("near",), ("rand",)] + deltas[:2] + alts[2:] + deltas[2:]
    return out


def tag_of(k, half):
    return 2 * (k % 61) + half


def limb(spec, stages, inverse, k, rng, first=0):
    """limb number k of a launch: family `spec` under the modulus of `stages`"""
    q, N = stages.q, stages.N
    name = spec[0]
    if name == "max":
        return np.full(N, q - 1, dtype=np.uint64)
    if name == "const":
        c = {"q-1": q - 1, "1": 1, "half": (q - 1) // 2}[spec[1]]
        out = np.empty(N, dtype=np.uint64)
        for h in range(2):
            t = tag_of(k, h)
            out[h * (N // 2):(h + 1) * (N // 2)] = c - t if spec[1] == "q-1" else c + t
        return out
    if name == "delta":
        out = np.zeros(N, dtype=np.uint64)
        out[spec[2]] = q - 1 if spec[1] == "q-1" else 1
        return out
    if name == "alt":
        return stages.carry_back(alt_pattern(q, N, spec[1], spec[2]), inverse, spec[1], first)
    if name == "near":
        v = np.uint64(q) - (rng.permutation(1 << 24)[:N].astype(np.uint64) + np.uint64(1))
        return v
    if name == "rand":
        return rng.integers(0, q, N, dtype=np.uint64)
    raise ValueError(spec)


@functools.lru_cache(maxsize=128)
def _stages(o, mi):
    return Stages(o, mi)


def limbs(o, inverse, n, mod_base, mod_count, start=0, first=0, seed=0):
    """(x[n][N], the spec of every limb): limb k of a launch under modulus mod_base + k % mod_count takes family start + k"""
    sp = specs(o.N, inverse, first)
    rng = np.random.default_rng(1000003 * o.N + 101 * start + seed)
    took = [sp[(start + k) % len(sp)] for k in range(n)]
    x = np.stack([limb(took[k], _stages(o, mod_base + k % mod_count), inverse, start + k, rng, first) for k in range(n)])
    return x, took


# ---- key-switch digit sources ------------------------------------------------------------------------------------------------------
def digit_source(o, nb, seed=0):
    """d2[nb][L][N] COEFFICIENT: the lift-window columns of tests/coeff_columns.py (residue limb i at 0, floor(q_i / 2), floor(q_i / 2)
    + 1, q_i - 1 and the edges of its lifts into the other moduli) at n = 0, 1, .. and, one column further on, at N/2 + n -- both
    members of a folded pair, with different columns --, and at the last word of each half; uniform residues elsewhere"""
    from tests import coeff_columns as ccol
    rng = np.random.default_rng(77 * o.N + seed)
    qs = [int(v) for v in o.q]
    cols = ccol.lift_windows(qs)
    C, h = len(cols), o.N // 2
    out = []
    for b in range(nb):
        poly = ccol.uniform_poly(qs, o.N, rng)
        for n in range(C):
            poly[:, n] = np.array(cols[(n + b) % C], dtype=np.uint64)
            poly[:, h + n] = np.array(cols[(n + b + 1) % C], dtype=np.uint64)
        poly[:, h - 1], poly[:, o.N - 1] = np.array(cols[0], dtype=np.uint64), np.array(cols[1 % C], dtype=np.uint64)
        out.append(poly)
    return np.stack(out)


def lifted(o, d2):
    """[nb][L(i)][L(j)][N]: the centred lift of residue limb i of every polynomial into q_j (COEFFICIENT: before the transform)"""
    qs = [int(v) for v in o.q]
    out = np.empty((d2.shape[0], len(qs), len(qs), o.N), dtype=np.uint64)
    for b in range(d2.shape[0]):
        for i, qi in enumerate(qs):
            v = lz.obj(d2[b, i])
            centred = np.where(np.array(2 * v > qi, dtype=bool), v - qi, v)
            for j, qj in enumerate(qs):
                out[b, i, j] = lz.u64(centred % qj)
    return out


# ---- the lazy butterflies' sum path in plain integers ----------------------------------------------------------------------------------
def max_sum_path(q, logN):
    """the word at position 0 of an all-(q - 1) limb through the inverse stages, as gs_bfly forms it: s = a + b, then s mod+ 4q.
    Returns [(s, fired)] per stage: the sum in front of the block and whether its conditional subtraction fired"""
    a, out = q - 1, []
    for _ in range(logN):
        s = 2 * a            # the partner at distance t went through the same sums
        fired = s >= 4 * q
        out.append((s, fired))
        a = s - 4 * q if fired else s
    return out
