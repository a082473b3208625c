"""The butterflies for q = 2^60 - d (csrc/ntt16_kernel.h at ArithKind::fold), without a GPU: the arithmetic in exact integers, the
blocks of csrc/ntt16_bfly.inc executed instruction by instruction against it, the static table of the inverse butterflies that need
no fold, and the worst-case ranges pushed through every stage of both slice lengths.

    fold(x) = (x mod 2^60) + (x >> 60) d   is congruent to x mod q and below T = 2^60 + 2^31 < 2q for every 64-bit x
    forward   u = fold(a):  a' = u + v, b' = u + 4q - v            (v = b w - qe q in [0, 4q), qe the 63-bit Shoup estimate)
    inverse   a' = fold(a + b)  or, where a and b are both known to be below T, a' = a + b < 2T < 4q;  b' = (a + 4q - b) w - qe q

tests/fold_bfly_model.py holds the model (the GPU tests of the block and of the transforms compare with the same one); the
instruction lists are the generator's own (tools/gen_ntt16_bfly.py), run here by a dozen-mnemonic interpreter on 32-bit registers, so
a block that names a wrong register, reads VCC too early or wraps where the model does not shows up on any machine.
"""
import os
import re
import subprocess
import sys

import pytest

from tests import fold_bfly_model as fm
from tests.param_chains import fold_edge, uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ntt16_bfly as gen   # noqa: E402

M32, W64 = (1 << 32) - 1, 1 << 64
D_MAX = (1 << 27) - 1
# d = 1 and d = 2^27 - 1 are the ends of the rule (no primes: the bounds do not ask for one), between them the default chain's moduli
MODULI = [(1 << 60) - 1, (1 << 60) - D_MAX] + uniform(8192, 15) + uniform(16384, 15) + [int(v) for part in fold_edge(32768, 7) for v in part]


def test_fold_is_a_reduction_below_T():
    for q in MODULI:
        d = (1 << 60) - q
        assert 0 < d <= D_MAX and fm.T < 2 * q and 2 * fm.T < 4 * q and fm.T + 4 * q < 8 * q < (1 << 63)
        for x in (0, 1, q - 1, q, (1 << 60) - 1, 1 << 60, fm.T - 1, fm.T, 4 * q - 1, 4 * q, 8 * q - 1, (1 << 63) - 1, 1 << 63, W64 - 1,
                  (15 << 60) | ((1 << 60) - 1), 15 << 60):
            f = fm.fold(x, q)
            assert f % q == x % q and 0 <= f < fm.T and f == (x & ((1 << 60) - 1)) + (x >> 60) * d
        assert fm.fold(W64 - 1, q) == (1 << 60) - 1 + 15 * d      # the largest value a fold can leave
        # the canonical store: fold, then one conditional subtraction
        for x in (0, q - 1, q, 2 * q - 1, 4 * q, 6 * q - 1, 8 * q - 1):
            f = fm.fold(x, q)
            assert (f - q if f >= q else f) == x % q


# ---- the generated blocks, executed --------------------------------------------------------------------------------------------------
class Machine:
    """32-bit registers by name; operands as the generator writes them: vN, v[N:N+1], %[name], literals"""
    def __init__(self, ops64, ops32):
        self.r = {}
        self.vcc = None
        self.vcc_age = 99        # VALU instructions since VCC was written
        for k, v in ops64.items():
            self.set64("%[" + k + "]", v)
        for k, v in ops32.items():
            self.r["%[" + k + "]"] = v
        self.alias = {}

    def tie(self, pair_name, lo_name, hi_name):
        """al / ah are the halves of the tied operand a (the contract the listing check verifies)"""
        self.alias["%[" + lo_name + "]"] = ("%[" + pair_name + "]", 0)
        self.alias["%[" + hi_name + "]"] = ("%[" + pair_name + "]", 1)

    def _half(self, name):
        m = re.match(r"v\[(\d+):(\d+)\]$", name)
        if m:
            return ("v%s" % m.group(1), "v%s" % m.group(2))
        return (name + ".lo", name + ".hi")

    def get32(self, name):
        if re.match(r"(0x[0-9a-f]+|\d+)$", name):
            return int(name, 0)
        if name in self.alias:
            p, h = self.alias[name]
            return self.r[self._half(p)[h]]
        return self.r[name]

    def set32(self, name, v):
        if name in self.alias:
            p, h = self.alias[name]
            self.r[self._half(p)[h]] = v & M32
        else:
            self.r[name] = v & M32

    def get64(self, name):
        if name == "0":
            return 0
        lo, hi = self._half(name)
        return self.r[lo] | (self.r[hi] << 32)

    def set64(self, name, v):
        lo, hi = self._half(name)
        self.r[lo], self.r[hi] = v & M32, (v >> 32) & M32

    def run(self, lines):
        for ln in lines:
            op, rest = ln.split(None, 1)
            a = [x.strip() for x in re.split(r",\s*(?![^\[]*\])", rest)]
            reads_vcc = op == "v_subb_co_u32"
            if reads_vcc:
                assert self.vcc is not None and self.vcc_age >= 2, "VCC read %d instructions after its write: %s" % (self.vcc_age, ln)
            self.vcc_age += 1
            if op == "v_mad_u64_u32":       # d64, carry-out, s0, s1, addend64
                v = self.get32(a[2]) * self.get32(a[3]) + self.get64(a[4])
                self.set64(a[0], v)
                if a[1] == "vcc":
                    self.vcc, self.vcc_age = None, 0     # a discarded carry-out: whoever reads VCC next reads rubbish
            elif op == "v_lshl_add_u64":    # d64, s64, shift, addend64
                self.set64(a[0], (self.get64(a[1]) << int(a[2])) + self.get64(a[3]))
            elif op == "v_lshrrev_b64":
                self.set64(a[0], self.get64(a[2]) >> int(a[1]))
            elif op == "v_lshrrev_b32":
                self.set32(a[0], self.get32(a[2]) >> int(a[1]))
            elif op == "v_lshlrev_b32":
                self.set32(a[0], self.get32(a[2]) << int(a[1]))
            elif op == "v_and_b32":
                self.set32(a[0], self.get32(a[1]) & self.get32(a[2]))
            elif op == "v_ashrrev_i32":
                self.set32(a[0], M32 if self.get32(a[2]) >> 31 else 0)
            elif op == "v_bfi_b32":
                m = self.get32(a[1])
                self.set32(a[0], (m & self.get32(a[2])) | (~m & M32 & self.get32(a[3])))
            elif op == "v_add_u32":
                self.set32(a[0], self.get32(a[1]) + self.get32(a[2]))
            elif op == "v_sub_co_u32":      # d, vcc, s0, s1
                v = self.get32(a[2]) - self.get32(a[3])
                self.set32(a[0], v)
                self.vcc, self.vcc_age = int(v < 0), 0
            elif op == "v_subb_co_u32":     # d, vcc, s0, s1, vcc
                v = self.get32(a[2]) - self.get32(a[3]) - self.vcc
                self.set32(a[0], v)
                self.vcc, self.vcc_age = int(v < 0), 0
            else:
                raise AssertionError("unknown instruction: " + ln)


def _run_block(kind, h2, q, a, b, w):
    s = (w << 63) // q
    nq = W64 - q
    c64 = {"q4": 4 * q, "nq4": W64 - 4 * q}
    c32 = {"nql": nq & M32, "nqh": nq >> 32, "wl0": w & M32, "wh0": w >> 32, "sl0": s & M32, "sh0": s >> 32, "sh20": (2 * (s >> 32)) & M32,
           "bl0": b & M32, "bh0": b >> 32}
    c64["a0"] = a
    if kind == "ctf":
        m = Machine(c64, c32)
        m.tie("a0", "al0", "ah0")
        m.run([ln.replace("%%", "%") for ln in gen.ctf_stream(0, h2)])
        return m.get64("%[a0]"), m.get32("%[bol0]") | (m.get32("%[boh0]") << 32)
    c64["b0"] = b
    m = Machine(c64, c32)
    m.run([ln.replace("%%", "%") for ln in (gen.gsf_stream if kind == "gsf" else gen.gsn_stream)(0, h2)])
    return m.get64("%[ao0]"), m.get64("%[bo0]")


def _operands(kind, q):
    ws = [1, q - 1, (((q >> 32) - 1) << 32) | M32] + fm.directed_ws(q, 2)
    if kind == "ctf":
        a_s = fm.forward_a_edges(q) + [(3 << 60) | M32, (7 << 60) | (M32 << 28) | M32]
        b_s = [0, q, 4 * q - 1, 8 * q - 1, (1 << 63) - 1, (3 << 32) | M32]
    elif kind == "gsf":
        a_s = [0, 1, q, fm.T - 1, fm.T, 2 * q, 4 * q - 1, (2 * q) | M32]
        b_s = [0, q, 4 * q - 1, fm.T, (3 * q) | M32]
    else:
        a_s = [0, 1, q, fm.T - 1, (1 << 60) | (M32 >> 2), q | M32]
        b_s = [0, q, fm.T - 1, q | M32]
    return [(a, b, w) for a in a_s for b in b_s for w in ws]


@pytest.mark.parametrize("kind", ["ctf", "gsf", "gsn"])
def test_generated_block_is_the_model(kind):
    n = 0
    for q in MODULI[:2] + MODULI[2:4] + MODULI[-2:]:
        for a, b, w in _operands(kind, q):
            want = fm.block(kind, q, a, b, w)
            for h2 in (False, True):
                assert _run_block(kind, h2, q, a, b, w) == want, (kind, h2, q, a, b, w)
            n += 1
    assert n > 500


def test_model_reaches_estimate_error_3():
    """the directed family (low words of the multiplicand and of floor(w 2^63 / q) near 2^32 - 1) makes the 63-bit estimate 3 short"""
    for q in (MODULI[2], MODULI[-1]):
        errs = {fm.shoup_error(q, b, w) for w in fm.directed_ws(q, 4) for b in fm.directed_bs(q, w, 8 * q)}
        assert 3 in errs, errs


# ---- the static range table ----------------------------------------------------------------------------------------------------------
def _table_from_the_rule(stages, d0):
    """restated, not imported: registers carry 'below T' or 'below 4q'; a pass starts at 'below 4q' everywhere; a butterfly on two
    'below T' registers adds without a fold and leaves its sum only 'below 4q'; every other one folds its sum to 'below T'; the
    product leg is 'below 4q' always"""
    state = ["4q"] * 16
    out = []
    for s in range(stages):
        d = d0 << s
        nf = []
        for k in range(16):
            if k & d:
                continue
            if state[k] == state[k + d] == "T":
                nf.append(k)
                state[k] = "4q"
            else:
                state[k] = "T"
            state[k + d] = "4q"
        out.append(nf)
    return out


def test_range_table_is_the_generators():
    for logns, passes in ((13, ((2, 1), (4, 1), (4, 1), (3, 2))), (14, ((2, 1), (4, 1), (4, 1), (4, 1)))):
        assert gen.PASSES[logns] == passes
        for st, d0 in passes:
            assert _table_from_the_rule(st, d0) == gen.nofold_table(st, d0)
    assert [sum(map(len, gen.nofold_table(st))) for st in (2, 3, 4)] == [4, 6, 9]
    assert gen.nofold_count(13) == (28, 104) and gen.nofold_count(14) == (31, 112)
    # a stage whose registers sit 2 apart from the start (pass 1' of the 2^13 slice: two columns per thread) has the same counts
    assert [len(nf) for nf in gen.nofold_table(3, 2)] == [0, 4, 2] and [len(nf) for nf in gen.nofold_table(4)] == [0, 4, 2, 3]


# ---- worst-case ranges through every stage -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logns", [13, 14])
def test_worst_case_ranges_through_all_stages(logns):
    """exclusive upper bounds per register, carried ACROSS the hand-offs (as the largest bound of any register: the hand-offs permute)
    while the kernel's state is reset there: no word at or above 4q in front of an inverse butterfly, none at or above 8q in front of
    a forward one, and no 64-bit wrap of a + b, a + 4q - b or 2u + 4q"""
    for q in MODULI:
        d = (1 << 60) - q
        fold_max = (1 << 60) + 15 * d           # exclusive bound of a fold of any 64-bit word
        assert fold_max <= fm.T
        # inverse: canonical, lazy [0, 4q) loads and the tensor load phase's [0, 3q) all enter below 4q
        bound = [4 * q] * 16
        for st, d0 in gen.PASSES[logns]:
            bound = [max(bound)] * 16
            table = gen.nofold_table(st, d0)
            for s in range(st):
                dd = d0 << s
                for k in range(16):
                    if k & dd:
                        continue
                    a, b = bound[k], bound[k + dd]
                    assert a <= 4 * q and b <= 4 * q, "a word at or above 4q in front of an inverse butterfly"
                    assert a + b < W64 and a + 4 * q < W64 and a + 4 * q < (1 << 63), "64-bit wrap"
                    if k in table[s]:
                        assert a <= fm.T and b <= fm.T
                        bound[k] = a + b - 1            # a' = a + b, both exclusive bounds
                        assert bound[k] <= 2 * fm.T < 4 * q
                    else:
                        bound[k] = min(fold_max, a + b)
                    bound[k + dd] = 4 * q               # the product: b w mod q + at most 3q
        assert max(bound) <= 4 * q                      # what the inverse hands over ([0, 4q))
        # forward: [0, 8q) in (the lazy contract of every producer), stage after stage
        bound = 8 * q
        for _ in range(logns + 1):                      # (+ 1: the outermost stage of a folded slice in the digit lift's load phase)
            assert bound <= 8 * q, "a word at or above 8q in front of a forward butterfly"
            u = min(fold_max, bound)
            assert 2 * u + 4 * q < W64
            bound = u + 4 * q                           # a' = u + v < u + 4q; b' = u + 4q - v <= u + 4q - 1 + ... both below u + 4q
        assert bound <= fm.T + 4 * q < 6 * q            # what the lazy store leaves: inside [0, 8q)


def test_committed_blocks_are_the_generators(tmp_path):
    out = tmp_path / "ntt16_bfly.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ntt16_bfly.py")], env=dict(os.environ, NTT16_BFLY_OUT=str(out)),
                          stdout=subprocess.DEVNULL)
    txt = out.read_text()
    assert txt == open(os.path.join(ROOT, "nested_hashing_psi_amd", "csrc", "ntt16_bfly.inc")).read()
    for name in ("NTT16_CTF1", "NTT16_CTF1H", "NTT16_GSF1", "NTT16_GSF1H", "NTT16_GSN1", "NTT16_GSN1H"):
        body = re.search(r"#define %s\(TWC\).*?\n        :" % name, txt, re.S).group(0)
        assert not re.search(r"v_mov|s_nop|v_nop|nq4", body), name
    sizes = {name: len(re.findall(r'\\n\\t"', re.search(r"#define %s\(TWC\).*?\n        :" % name, txt, re.S).group(0)))
             for name in ("NTT16_CTS1H", "NTT16_CTF1H", "NTT16_CTF1", "NTT16_GS1H", "NTT16_GSF1H", "NTT16_GSN1H", "NTT16_GS1", "NTT16_GSF1", "NTT16_GSN1")}
    assert (sizes["NTT16_CTF1H"], sizes["NTT16_CTF1"]) == (17, 18) and sizes["NTT16_CTS1H"] == 18
    assert sizes["NTT16_GSF1H"] == sizes["NTT16_GS1H"] - 1 == 18 and sizes["NTT16_GSF1"] == sizes["NTT16_GS1"] - 1
    assert sizes["NTT16_GSN1H"] == sizes["NTT16_GS1H"] - 4 == 15 and sizes["NTT16_GSN1"] == sizes["NTT16_GS1"] - 4
