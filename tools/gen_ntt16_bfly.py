#!/usr/bin/env python3
"""Generates nested_hashing_psi_amd/csrc/ntt16_bfly.inc: the 60-bit lazy NTT butterflies of ntt16_kernel.h as hand-scheduled
gfx950 instruction blocks (the generator can interleave NB independent butterflies per block; NB = 1 is what ships).

Issue costs on gfx950 (tools/microbench_ops.hip, cycles per wave64 instruction per SIMD with 2+ waves): every VOP3 instruction --
v_mad_u64_u32, v_lshl_add_u64, v_lshrrev_b64, v_bfi_b32, v_mul_lo/hi_u32 alike -- 4.1-4.3; 32-bit VOP1/VOP2 2.0-2.5; a wave
alone on its SIMD 4+ for everything; a 2-cycle instruction that follows a 4-cycle one costs 4 itself (tools/microbench_operands.hip), so
the VOP1/VOP2 instructions are grouped.  Both blocks are 20 instructions, 19 where 2 sh is an operand (the inverse's last product is
written straight to the output; 64-bit differences are borrow chains through VCC, see ct_stream).  The seeded forward block
(cts_stream, what the kernels use; ct_stream is kept for -DNTT16_CT_SEEDED=0 builds) is 19 / 18: its remainder chain starts at u
and ends as a'.  Contexts whose moduli are all 2^60 - d, d < 2^27, reduce by folding with d instead of the select: ctf_stream
(forward, 18 / 17), gsf_stream (inverse, 19 / 18) and gsn_stream (inverse between two operands that are known to be small: no
reduction, 16 / 15); nofold_table says which butterflies of a pass take the last.

    python tools/gen_ntt16_bfly.py          (rewrites the .inc; the output is committed)

Register use of stream i: 11 fixed VGPRs v[128 - 11 (i + 1) .. 128 - 11 i) (an asm operand cannot name the halves of a 64-bit pair, so every
temporary whose halves are needed lives in a named register; all are in the clobber list); 9 in the seeded forward block.
"""
import os

OUT = os.environ.get("NTT16_BFLY_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nested_hashing_psi_amd", "csrc", "ntt16_bfly.inc")


NREG = {False: 11, True: 11}  # fixed VGPRs per stream: forward (CT), inverse (GS)


class Regs:
    """Fixed registers of stream i.  Lifetimes allow these overlays (see the instruction lists):
    CT:   u over t (the select writes in place); the sign mask in QE's low register until qe is written; u + 4q over QE (after
          the last use of qe)
    GS:   a + 4q over QE (dead once d exists); s = a + b over ACC and t = s - 4q over C (both dead after the select, before
          the first product); the sign mask in X until 2 dh is written"""
    def __init__(self, i, gs):
        n = NREG[gs]
        self.n = n
        self.base = 128 - n * (i + 1) - int(os.environ.get('NTT16_BASE_SHIFT', '0'))
        b = self.base
        self.X = b           # 2 bh (CT) / sign mask, then 2 dh (GS)
        self.T = b + 1       # CT: t = a - 4q, then u in place
        self.U = self.T
        self.D = b + 1       # GS: d = a - b + 4q
        self.CR = b + 3      # m1 / cr / cr >> 31
        self.QE = b + 5
        self.T6 = self.QE    # CT: u + 4q (after the last use of qe); GS: a + 4q (before qe)
        self.ACC = b + 7     # acc, then v
        self.C = b + 9

    def all(self):
        return range(self.base, self.base + self.n)


def p(r):
    return "v[%d:%d]" % (r, r + 1)


def v(r):
    return "v%d" % r


# A 64-bit difference is v_sub_co_u32 + v_subb_co_u32 through VCC (gfx950 has no 64-bit vector subtraction; the alternative,
# x + ~y + 1, is two v_not_b32 and a v_lshl_add_u64).  A VALU instruction that reads VCC needs two wait states after the VALU
# write of VCC: two independent instructions that leave VCC alone sit between the halves (the multiplier instructions discard
# their carry-out into VCC, so none of them may).  The halves of an asm operand cannot be named, so a result that is produced
# in halves is two 32-bit outputs (the register coalescer makes them a pair).
def ct_stream(i, h2=False):
    r = Regs(i, False)
    o = lambda name: "%%[%s%d]" % (name, i)
    bl, bh = o("bl"), o("bh")
    m = r.QE  # the sign mask lives in qe's low register until qe is written (the selects consume it before that)
    return [
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.CR), bl, o("sh")),                  # m1 = bl sh
        "v_lshl_add_u64 %s, %s, 0, %%[nq4]" % (p(r.T), o("a")),                       # t = a - 4q
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.CR), bh, o("sl"), p(r.CR)),        # cr = bh sl + m1
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.ACC), bl, o("wl")),                 # acc = bl wl
        # the 2-cycle instructions sit next to each other: one that follows a 4-cycle instruction costs 4 itself
        # (profiles/r03/microbench_operands.txt, "mad + v_not alternating")
    ] + ([] if h2 else [
        "v_lshlrev_b32 %s, 1, %s" % (v(r.X), bh),                                     # 2 bh
    ]) + [
        "v_ashrrev_i32 %s, 31, %s" % (v(m), v(r.T + 1)),                              # all ones iff t < 0
        "v_bfi_b32 %s, %s, %s, %s" % (v(r.U), v(m), o("al"), v(r.T)),                 # u = t < 0 ? a : t   (in place)
        "v_bfi_b32 %s, %s, %s, %s" % (v(r.U + 1), v(m), o("ah"), v(r.T + 1)),
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.C), bl, o("wh")),                   # c = bl wh
        "v_lshrrev_b64 %s, 31, %s" % (p(r.CR), p(r.CR)),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.C), bh, o("wl"), p(r.C)),          # c += bh wl
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), bh, o("sh2"), p(r.CR))) if h2 else     # qe = bh (2 sh) + (cr >> 31)
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), v(r.X), o("sh"), p(r.CR))),  # qe = 2 bh sh + (cr >> 31)
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (p(r.ACC), v(r.QE), p(r.ACC)),     # acc += qe_lo nq_lo
        "v_mad_u64_u32 %s, vcc, %s, %%[nqh], %s" % (p(r.C), v(r.QE), p(r.C)),         # c += qe_lo nq_hi
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (p(r.C), v(r.QE + 1), p(r.C)),     # c += qe_hi nq_lo: the last read of an input
        "v_lshl_add_u64 %s, %s, 0, %%[q4]" % (p(r.T6), p(r.U)),                       # u + 4q   (over qe)
        "v_sub_co_u32 %s, vcc, %s, %s" % (o("bol"), v(r.T6), v(r.ACC)),               # b' = u + 4q - v, low half
        "v_add_u32 %s, %s, %s" % (v(r.ACC + 1), v(r.ACC + 1), v(r.C)),                # v = acc + (c << 32)
        "v_lshl_add_u64 %s, %s, 0, %s" % (o("ao"), p(r.U), p(r.ACC)),                 # a' = u + v
        "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (o("boh"), v(r.T6 + 1), v(r.ACC + 1)), # b', high half
    ]


class RegsS:
    """Fixed registers of stream i of the seeded forward block: 9.  The remainder's low chain accumulates in a's own registers
    (a is dead once u exists), so the block has no acc pair; 2u + 4q is formed over u in place; the sign mask lives in qe's low
    register until qe is written."""
    n = 9

    def __init__(self, i):
        self.base = 128 - self.n * (i + 1) - int(os.environ.get('NTT16_BASE_SHIFT', '0'))
        b = self.base
        self.X = b           # 2 bh
        self.T = b + 1       # t = a - 4q, then u in place, then 2u + 4q in place
        self.U = self.T
        self.CR = b + 3      # m1 / cr / cr >> 31
        self.QE = b + 5
        self.C = b + 7

    def all(self):
        return range(self.base, self.base + self.n)


# The seeded forward block: a' = u + v and v = b w + qe (2^64 - q) are all arithmetic mod 2^64 on values whose true results lie
# below 8q < 2^63, so the low chain of the remainder starts at bl wl + u instead of bl wl + 0 and ends as a' -- the parent's
# a' = u + v (one v_lshl_add_u64) is gone.  b' = u + 4q - v = (2u + 4q) - a': 2u + 4q < 12q < 2^64 is one v_lshl_add_u64 with
# shift 1, and the difference is the same borrow chain against a'.  A wrap in a partial sum of the chain is harmless mod 2^64.
#
# a is a tied operand (%[a]: read as a, written as a'); %[al] / %[ah] are (u32)a and (u32)(a >> 32) of the same variable, which
# the register allocator keeps in the two halves of that pair -- an asm operand cannot name the halves of a pair, and the
# borrow chain and the high-word add need them.  That allocation is checked in every instantiation's listing, not assumed:
# tools/ct_seeded_listing.py.  The low chain writes %[a] (twice) only after the last read of a, al and ah as *inputs* (the
# selects); from then on %[al] / %[ah] name the halves of the accumulating a'.
#
# The VCC wait states: v_sub_co needs a' low word, which needs qe, and every VCC-free instruction of the block but the
# high-word add is an ancestor of qe or of the subtraction's minuend -- inside one block there is one VCC-free filler, not two.
# The second is the last product of the high chain, which needs only qe: it discards its carry-out into an SGPR pair of its own
# (%[cs], an output nobody reads) instead of VCC.  Tried first: the whole product in the low chain, `last mad (writes a') ->
# v_sub_co -> v_subb_co`.  That tail has no filler at all (the minuend 2u + 4q must precede v_sub_co) and pays an s_nop 1; ending
# the low chain early and patching the high word of a' through %[ah] between the halves of the difference pays none.
def cts_stream(i, h2=False):
    r = RegsS(i)
    o = lambda name: "%%[%s%d]" % (name, i)
    bl, bh = o("bl"), o("bh")
    m = r.QE
    return [
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.CR), bl, o("sh")),                  # m1 = bl sh
        "v_lshl_add_u64 %s, %s, 0, %%[nq4]" % (p(r.T), o("a")),                       # t = a - 4q
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.CR), bh, o("sl"), p(r.CR)),        # cr = bh sl + m1
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.C), bl, o("wh")),                   # c = bl wh
    ] + ([] if h2 else [
        "v_lshlrev_b32 %s, 1, %s" % (v(r.X), bh),                                     # 2 bh
    ]) + [
        "v_ashrrev_i32 %s, 31, %s" % (v(m), v(r.T + 1)),                              # all ones iff t < 0
        "v_bfi_b32 %s, %s, %s, %s" % (v(r.U), v(m), o("al"), v(r.T)),                 # u = t < 0 ? a : t   (in place)
        "v_bfi_b32 %s, %s, %s, %s" % (v(r.U + 1), v(m), o("ah"), v(r.T + 1)),         # the last read of a
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (o("a"), bl, o("wl"), p(r.U)),          # a' = bl wl + u: the chain is seeded
        "v_lshrrev_b64 %s, 31, %s" % (p(r.CR), p(r.CR)),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.C), bh, o("wl"), p(r.C)),          # c += bh wl
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), bh, o("sh2"), p(r.CR))) if h2 else     # qe = bh (2 sh) + (cr >> 31)
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), v(r.X), o("sh"), p(r.CR))),  # the last read of b and of the twiddle
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (o("a"), v(r.QE), o("a")),         # a' += qe_lo nq_lo: its low word is final
        "v_mad_u64_u32 %s, vcc, %s, %%[nqh], %s" % (p(r.C), v(r.QE), p(r.C)),         # c += qe_lo nq_hi
        "v_lshl_add_u64 %s, %s, 1, %%[q4]" % (p(r.U), p(r.U)),                        # 2u + 4q   (in place)
        "v_sub_co_u32 %s, vcc, %s, %s" % (o("bol"), v(r.U), o("al")),                 # b' = 2u + 4q - a', low half
        "v_mad_u64_u32 %s, %%[cs], %s, %%[nql], %s" % (p(r.C), v(r.QE + 1), p(r.C)),  # c += qe_hi nq_lo   (carry-out not into VCC)
        "v_add_u32 %s, %s, %s" % (o("ah"), o("ah"), v(r.C)),                          # a' += c << 32
        "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (o("boh"), v(r.U + 1), o("ah")),       # b', high half
    ]


def gs_stream(i, h2=False):
    """h2: 2 sh is an operand of its own (wave-uniform twiddles: the doubling is a scalar instruction)"""
    r = Regs(i, True)
    o = lambda name: "%%[%s%d]" % (name, i)
    dl, dh = v(r.D), v(r.D + 1)
    s, t, m = r.ACC, r.C, r.X
    return [
        "v_lshl_add_u64 %s, %s, 0, %%[q4]" % (p(r.T6), o("a")),                       # a + 4q   (over qe)
        "v_lshl_add_u64 %s, %s, 0, %s" % (p(s), o("a"), o("b")),                      # s = a + b   (over acc)
        "v_sub_co_u32 %s, vcc, %s, %s" % (dl, v(r.T6), o("bl")),                      # d = a + 4q - b, low half
        "v_lshl_add_u64 %s, %s, 0, %%[nq4]" % (p(t), p(s)),                           # t = s - 4q   (over c)
        "v_ashrrev_i32 %s, 31, %s" % (v(m), v(t + 1)),                                # all ones iff t < 0
        "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (dh, v(r.T6 + 1), o("bh")),            # d, high half
        "v_bfi_b32 %s, %s, %s, %s" % (o("aol"), v(m), v(s), v(t)),                    # a' = t < 0 ? s : t   (early-clobber outputs:
        "v_bfi_b32 %s, %s, %s, %s" % (o("aoh"), v(m), v(s + 1), v(t + 1)),            #  the twiddles are read below)
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.ACC), dl, o("wl")),
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.C), dl, o("wh")),
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.CR), dl, o("sh")),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.CR), dh, o("sl"), p(r.CR)),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.C), dh, o("wl"), p(r.C)),
    ] + ([] if h2 else [
        "v_lshlrev_b32 %s, 1, %s" % (v(r.X), dh),
    ]) + [
        "v_lshrrev_b64 %s, 31, %s" % (p(r.CR), p(r.CR)),
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), dh, o("sh2"), p(r.CR))) if h2 else
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), v(r.X), o("sh"), p(r.CR))),  # the last read of a per-lane twiddle
        "v_mad_u64_u32 %s, vcc, %s, %%[nqh], %s" % (p(r.C), v(r.QE), p(r.C)),
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (p(r.C), v(r.QE + 1), p(r.C)),
        "v_add_u32 %s, %s, %s" % (v(r.ACC + 1), v(r.ACC + 1), v(r.C)),                # dl wl + (c << 32)
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (o("bo"), v(r.QE), p(r.ACC)),      # b' = d w: the last product lands in the output
    ]


# ---- q = 2^60 - d (contexts with NttPlan::fold_moduli: every modulus has d < 2^27) ---------------------------------------------------
# fold(x) = (x mod 2^60) + (x >> 60) d is congruent to x and below T = 2^60 + 2^31 < 2q for every 64-bit x: three instructions
# (v_lshrrev_b32 and v_and_b32 on the high word, one v_mad_u64_u32 onto the masked pair; d is the low word of 2^64 - q, nql) where the
# conditional subtraction of 4q takes four, and a tighter range than [0, 4q).
FOLD_MASK = "0xfffffff"   # the high word of 2^60 - 1


# The seeded forward block with u = fold(a) in a's own registers: the mask is written through %[ah] (the same reliance on the
# allocation of al / ah as the seeded block's tail, checked by the same tool), the fold and both products of the low chain
# accumulate in %[a], and 2u + 4q is taken from u before the chain goes on.  a' = u + v < T + 4q < 6q, b' = u + 4q - v in (0, 6q).
# 17 instructions with 2 sh as an operand, 18 without; nq4 is not read.  The three 32-bit instructions open the block: they follow
# the v_subb_co_u32 that closes the block before (a 2-cycle instruction behind a 4-cycle one costs 4).
def ctf_stream(i, h2=False):
    r = RegsS(i)
    o = lambda name: "%%[%s%d]" % (name, i)
    bl, bh = o("bl"), o("bh")
    m = r.QE  # a >> 60 lives in qe's low register until qe is written
    return [
        "v_lshrrev_b32 %s, 28, %s" % (v(m), o("ah")),                                 # a >> 60
        "v_and_b32 %s, %s, %s" % (o("ah"), FOLD_MASK, o("ah")),                       # a mod 2^60   (in place)
    ] + ([] if h2 else [
        "v_lshlrev_b32 %s, 1, %s" % (v(r.X), bh),                                     # 2 bh
    ]) + [
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.CR), bl, o("sh")),                  # m1 = bl sh
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (o("a"), v(m), o("a")),            # u = fold(a)   (in place)
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.CR), bh, o("sl"), p(r.CR)),        # cr = bh sl + m1
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.C), bl, o("wh")),                   # c = bl wh
        "v_lshl_add_u64 %s, %s, 1, %%[q4]" % (p(r.U), o("a")),                        # 2u + 4q
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (o("a"), bl, o("wl"), o("a")),          # a' = bl wl + u: the chain is seeded
        "v_lshrrev_b64 %s, 31, %s" % (p(r.CR), p(r.CR)),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.C), bh, o("wl"), p(r.C)),          # c += bh wl
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), bh, o("sh2"), p(r.CR))) if h2 else     # qe = bh (2 sh) + (cr >> 31)
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), v(r.X), o("sh"), p(r.CR))),  # the last read of b and of the twiddle
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (o("a"), v(r.QE), o("a")),         # a' += qe_lo nq_lo: its low word is final
        "v_mad_u64_u32 %s, vcc, %s, %%[nqh], %s" % (p(r.C), v(r.QE), p(r.C)),         # c += qe_lo nq_hi
        "v_sub_co_u32 %s, vcc, %s, %s" % (o("bol"), v(r.U), o("al")),                 # b' = 2u + 4q - a', low half
        "v_mad_u64_u32 %s, %%[cs], %s, %%[nql], %s" % (p(r.C), v(r.QE + 1), p(r.C)),  # c += qe_hi nq_lo   (carry-out not into VCC)
        "v_add_u32 %s, %s, %s" % (o("ah"), o("ah"), v(r.C)),                          # a' += c << 32
        "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (o("boh"), v(r.U + 1), o("ah")),       # b', high half
    ]


def gs_product(r, o, h2, first=None):
    """b' = d w of the inverse blocks: d in r.D, the result in %[bo].  first: the instruction that opens the low chain, where the
    caller has placed it already"""
    dl, dh = v(r.D), v(r.D + 1)
    return ([] if first else [
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.ACC), dl, o("wl")),
    ]) + [
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.C), dl, o("wh")),
        "v_mad_u64_u32 %s, vcc, %s, %s, 0" % (p(r.CR), dl, o("sh")),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.CR), dh, o("sl"), p(r.CR)),
        "v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.C), dh, o("wl"), p(r.C)),
    ] + ([] if h2 else [
        "v_lshlrev_b32 %s, 1, %s" % (v(r.X), dh),
    ]) + [
        "v_lshrrev_b64 %s, 31, %s" % (p(r.CR), p(r.CR)),
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), dh, o("sh2"), p(r.CR))) if h2 else
        ("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (p(r.QE), v(r.X), o("sh"), p(r.CR))),  # the last read of a per-lane twiddle
        "v_mad_u64_u32 %s, vcc, %s, %%[nqh], %s" % (p(r.C), v(r.QE), p(r.C)),
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (p(r.C), v(r.QE + 1), p(r.C)),
        "v_add_u32 %s, %s, %s" % (v(r.ACC + 1), v(r.ACC + 1), v(r.C)),                # dl wl + (c << 32)
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (o("bo"), v(r.QE), p(r.ACC)),      # b' = d w: the last product lands in the output
    ]


# The folding inverse block: a' = fold(a + b) < T (a + b < 8q < 2^63).  The shift and the mask fill the wait states between the
# halves of d; the fold's multiply-add discards its carry-out into VCC and therefore follows the high half.  One instruction
# fewer than NTT16_GS1 / NTT16_GS1H: 19 / 18.  a' is one 64-bit early-clobber output (the twiddles are read after it is written).
def gsf_stream(i, h2=False):
    r = Regs(i, True)
    o = lambda name: "%%[%s%d]" % (name, i)
    s, m = r.ACC, r.X
    return [
        "v_lshl_add_u64 %s, %s, 0, %%[q4]" % (p(r.T6), o("a")),                       # a + 4q   (over qe)
        "v_lshl_add_u64 %s, %s, 0, %s" % (p(s), o("a"), o("b")),                      # s = a + b   (over acc)
        "v_sub_co_u32 %s, vcc, %s, %s" % (v(r.D), v(r.T6), o("bl")),                  # d = a + 4q - b, low half
        "v_lshrrev_b32 %s, 28, %s" % (v(m), v(s + 1)),                                # s >> 60
        "v_and_b32 %s, %s, %s" % (v(s + 1), FOLD_MASK, v(s + 1)),                     # s mod 2^60
        "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(r.D + 1), v(r.T6 + 1), o("bh")),    # d, high half
        "v_mad_u64_u32 %s, vcc, %s, %%[nql], %s" % (o("ao"), v(m), p(s)),             # a' = fold(s)
    ] + gs_product(r, o, h2)


# The non-folding inverse block, for a and b both below T: a' = a + b < 2T = 2^61 + 2^32 < 4q as it stands.  Four instructions
# fewer than NTT16_GS1 / NTT16_GS1H: 16 / 15.  The select that filled the wait states between the halves of d is gone; the sum is
# one filler, the product that opens the low chain the other (it needs the low half of d only, and discards its carry-out into an
# SGPR pair of its own -- cs, early-clobber: it is written before the twiddles are read -- instead of VCC).
def gsn_stream(i, h2=False):
    r = Regs(i, True)
    o = lambda name: "%%[%s%d]" % (name, i)
    first = "v_mad_u64_u32 %s, %%[cs], %s, %s, 0" % (p(r.ACC), v(r.D), o("wl"))
    return [
        "v_lshl_add_u64 %s, %s, 0, %%[q4]" % (p(r.T6), o("a")),                       # a + 4q   (over qe)
        "v_sub_co_u32 %s, vcc, %s, %s" % (v(r.D), v(r.T6), o("bl")),                  # d = a + 4q - b, low half
        "v_lshl_add_u64 %s, %s, 0, %s" % (o("ao"), o("a"), o("b")),                   # a' = a + b
        first,                                                                        # dl wl   (carry-out not into VCC)
        "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(r.D + 1), v(r.T6 + 1), o("bh")),    # d, high half
    ] + gs_product(r, o, h2, first)


# Which inverse butterflies take the non-folding block is static.  In the Gentleman-Sande network a butterfly of one stage pairs two
# sum legs or two product legs of the stage before; a sum leg is below T after a fold (below 2T < 4q without one), a product leg
# below 4q.  Every pass starts from "below 4q" on all 16 registers (the loads and the LDS hand-offs promise no more) and runs its
# stages on register distances d0, 2 d0, ...: csrc/ntt16_kernel.h keeps this state in GsRanges, here it is as a table.
PASSES = {13: ((2, 1), (4, 1), (4, 1), (3, 2)), 14: ((2, 1), (4, 1), (4, 1), (4, 1))}   # slice length -> (stages, d0) of passes 4', 3', 2', 1'


def nofold_table(stages, d0=1):
    """-> per stage of one pass, the low registers k of the butterflies (x[k], x[k + d]) that need no fold"""
    below_t, out = 0, []
    for s in range(stages):
        d = d0 << s
        lows = [k for k in range(16) if not k & d]
        nf = [k for k in lows if below_t >> k & below_t >> (k + d) & 1]
        out.append(nf)
        below_t = sum(1 << k for k in lows if k not in nf)
    return out


def nofold_count(logns):
    """-> (non-folding butterflies, butterflies) per thread of one slice of 2^logns coefficients"""
    return sum(len(nf) for st, d0 in PASSES[logns] for nf in nofold_table(st, d0)), 8 * sum(st for st, _ in PASSES[logns])


def interleave(streams):
    out = []
    for k in range(max(len(s) for s in streams)):
        for s in streams:
            if k < len(s):
                out.append(s[k])
    return out


def emit(name, gs, nb, h2=False, seeded=False, fold=None):
    """h2: the twiddle's doubled high Shoup word is an operand (t.sh2); seeded: the forward block whose chain starts at u;
    fold: one of the blocks for q = 2^60 - d -- "ctf" (forward, seeded), "gsf" (inverse, folding), "gsn" (inverse, non-folding)"""
    assert not (gs and seeded) and fold in (None, "ctf", "gsf", "gsn") and (not fold or (gs, seeded) == (fold != "ctf", fold == "ctf"))
    stream = {None: gs_stream if gs else cts_stream if seeded else ct_stream, "ctf": ctf_stream, "gsf": gsf_stream, "gsn": gsn_stream}[fold]
    lines = interleave([stream(i, h2) for i in range(nb)])
    body = " \\\n".join('        "%s\\n\\t"' % ln for ln in lines)
    # forward: no early-clobber -- every input is read before the first output is written (checked below), so outputs may reuse
    # input registers.  inverse: a' is written before the twiddles are read -> its two halves are early-clobber outputs.
    # seeded forward: a' grows in the tied operand a, whose registers no other input can share; al / ah name its halves (see
    # cts_stream), read as a before the first write of a and as a' after the last, never in between.
    late = ("bo",) if gs else ("bol", "boh", "cs") if seeded else ("ao", "bol", "boh")
    first_out = min(k for k, ln in enumerate(lines) if any("%%[%s" % nm in ln for nm in late))
    vgpr_inputs = ["%%[%s%d]" % (nm, i) for nm in (("b", "bl", "bh", "wl", "wh", "sl", "sh", "sh2") if seeded else
                                                   ("a", "b", "al", "ah", "bl", "bh", "wl", "wh", "sl", "sh", "sh2")) for i in range(nb)]
    for ln in lines[first_out + 1:]:
        assert not any(op + "," in ln + "," or ln.endswith(op) for op in vgpr_inputs), "input read after an output was written: " + ln
    if seeded:
        for i in range(nb):
            wr = [k for k, ln in enumerate(lines) if ln.split()[1] == "%%[a%d]," % i]
            # (the fold block's chain has one more link, u = fold(a), behind the mask written through ah)
            assert len(wr) == (3 if fold else 2) and wr[-1] < first_out, "the low chain ends before the difference starts"
            if fold:
                assert [ln.split()[0] for ln in lines if "%%[ah%d]" % i in ln][:2] == ["v_lshrrev_b32", "v_and_b32"], "shift, then mask"
                assert not any("%%[a%s%d]" % (hl, i) in ln for ln in lines[2:wr[0]] for hl in "lh"), "half of a touched between mask and fold"
            assert not any("%%[a%s%d]" % (hl, i) in ln for ln in lines[wr[0]:wr[-1] + 1] for hl in "lh"), "half of a read inside the low chain"
            assert not any("%%[a%d]" % i in ln for ln in lines[wr[-1] + 1:]), "a' touched as a pair after its low chain"
    # VCC: written by the low half of a difference, read by its high half two or more instructions later, untouched in between
    for k, ln in enumerate(lines):
        if ln.startswith("v_sub_co_u32"):
            j = next(j for j in range(k + 1, len(lines)) if lines[j].startswith("v_subb_co_u32"))
            assert j - k - 1 >= 2 and not any("vcc" in x for x in lines[k + 1:j]), "VCC hazard: " + ln
    if fold in ("gsf", "gsn"):
        outs = ", ".join('[ao%d] "=&v"(ao%d), [bo%d] "=v"(bo%d)' % ((i,) * 4) for i in range(nb)) + (', [cs] "=&s"(cs)' if fold == "gsn" else "")
    elif gs:
        outs = ", ".join('[aol%d] "=&v"(aol%d), [aoh%d] "=&v"(aoh%d), [bo%d] "=v"(bo%d)' % ((i,) * 6) for i in range(nb))
    elif seeded:
        outs = ", ".join('[a%d] "+v"(a%d), [bol%d] "=v"(bol%d), [boh%d] "=v"(boh%d)' % ((i,) * 6) for i in range(nb)) + ', [cs] "=s"(cs)'
    else:
        outs = ", ".join('[ao%d] "=v"(ao%d), [bol%d] "=v"(bol%d), [boh%d] "=v"(boh%d)' % ((i,) * 6) for i in range(nb))
    twc = "TWC"
    ins = []
    for i in range(nb):
        if gs:
            ins.append('[a%d] "v"(a%d), [b%d] "v"(b%d), [bl%d] "v"((u32)b%d), [bh%d] "v"((u32)(b%d >> 32))' % ((i,) * 8))
        elif seeded:
            ins.append('[al%d] "v"((u32)a%d), [ah%d] "v"((u32)(a%d >> 32)), [bl%d] "v"((u32)b%d), [bh%d] "v"((u32)(b%d >> 32))' % ((i,) * 8))
        else:
            ins.append('[a%d] "v"(a%d), [al%d] "v"((u32)a%d), [ah%d] "v"((u32)(a%d >> 32)), [bl%d] "v"((u32)b%d), [bh%d] "v"((u32)(b%d >> 32))'
                       % ((i,) * 10))
        ins.append('[wl%d] %s(t%d.wl), [wh%d] %s(t%d.wh), [sl%d] %s(t%d.sl), [sh%d] %s(t%d.sh)' % (i, twc, i, i, twc, i, i, twc, i, i, twc, i))
        if h2:
            ins.append('[sh2%d] %s(t%d.sh2)' % (i, twc, i))
    ins.append('[nql] "s"(m.nql), [nqh] "s"(m.nqh), [q4] "s"(m.q4)' if fold else '[nql] "s"(m.nql), [nqh] "s"(m.nqh), [nq4] "s"(m.nq4), [q4] "s"(m.q4)')
    clob = ['"vcc"'] + ['"v%d"' % x for i in range(nb) for x in (RegsS(i) if seeded else Regs(i, gs)).all()]
    return ("#define %s(TWC) \\\n    asm( \\\n%s \\\n        : %s \\\n        : %s \\\n        : %s)\n"
            % (name, body, outs, ", \\\n          ".join(ins), ", ".join(clob)))


def main():
    text = ("// ntt16_bfly.inc -- GENERATED by tools/gen_ntt16_bfly.py; do not edit.  See that script and ntt16_kernel.h.\n"
            "// NTT16_CT1(TWC): one forward butterfly on (a0, b0, t0) -> (ao0, {bol0, boh0}); NTT16_GS1(TWC): one inverse butterfly\n"
            "// -> ({aol0, aoh0}, bo0).  TWC = NTT16_S (wave-uniform twiddles, SGPR operands) or NTT16_V (per-lane twiddles); m = ModC.\n"
            "// NTT16_CT1H(TWC) / NTT16_GS1H(TWC): 2 sh is an operand of its own (t0.sh2) -- one instruction fewer.\n"
            "// NTT16_CTS1(TWC) / NTT16_CTS1H(TWC): the seeded forward butterfly, one instruction fewer again: (a0 tied, b0, t0) ->\n"
            "// (a0, {bol0, boh0}); cs is an SGPR pair that takes one discarded carry-out.\n"
            "// q = 2^60 - d, d < 2^27 (m.nql = d): NTT16_CTF1(TWC) / NTT16_CTF1H(TWC), the seeded forward butterfly with u = fold(a), same\n"
            "// operands; NTT16_GSF1(TWC) / NTT16_GSF1H(TWC): the inverse butterfly with a' = fold(a + b), -> (ao0, bo0); NTT16_GSN1(TWC) /\n"
            "// NTT16_GSN1H(TWC): a' = a + b for a, b below 2^60 + 2^31, -> (ao0, bo0), cs as above.  None of them reads m.nq4.\n")
    # one butterfly per block: measured, a wave issues at most every other VALU slot whatever its instruction-level parallelism
    # (interleaving two butterflies per block changed nothing but the register count), so parallelism comes from waves
    text += emit("NTT16_CT1", False, 1) + emit("NTT16_GS1", True, 1) + emit("NTT16_CT1H", False, 1, True) + emit("NTT16_GS1H", True, 1, True)
    text += emit("NTT16_CTS1", False, 1, seeded=True) + emit("NTT16_CTS1H", False, 1, True, seeded=True)
    text += emit("NTT16_CTF1", False, 1, seeded=True, fold="ctf") + emit("NTT16_CTF1H", False, 1, True, seeded=True, fold="ctf")
    text += emit("NTT16_GSF1", True, 1, fold="gsf") + emit("NTT16_GSF1H", True, 1, True, fold="gsf")
    text += emit("NTT16_GSN1", True, 1, fold="gsn") + emit("NTT16_GSN1H", True, 1, True, fold="gsn")
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT)
    for logns in sorted(PASSES):
        print("2^%d slice, inverse at the fold kind: %d of %d butterflies per thread without a fold (passes of %s stages: %s)" % (
            (logns,) + nofold_count(logns) + (", ".join(str(st) for st, _ in PASSES[logns]),
                                              " + ".join(str(sum(len(nf) for nf in nofold_table(st, d0))) for st, d0 in PASSES[logns]))))


if __name__ == "__main__":
    main()
