"""the seeded forward butterfly (NTT16_CTS1 / NTT16_CTS1H of csrc/ntt16_bfly.inc) in a hipcc -S listing of kernels_ntt16.hip:
python tools/ct_seeded_listing.py file.s

The block's contract (csrc/ntt16_kernel.h) rests on one thing no operand constraint can state: that the inputs al / ah, the halves
of the tied operand a, sit in the two registers of a's pair.  This asserts it for every forward block of every kernel of the
listing, from the registers the compiler substituted:
  the two v_mad_u64_u32 of the low chain write one pair v[L:L+1], the second accumulating onto it;
  the selects before them read vL, v(L+1) as the halves of a;
  v_sub_co_u32 subtracts vL, v_add_u32 updates v(L+1) in place, v_subb_co_u32 subtracts v(L+1);
  the pair is none of the block's fixed registers and none of b's;
and reports per kernel: forward blocks, instructions per block (18 with 2 sh as an operand, 19 without), v_mov / s_nop inside a block
(none allowed), VGPRs, spills and scratch (128, 0, 0 required of every ntt16_kernel_t).  Exit status 1 when anything fails.
A listing built with -DNTT16_CT_SEEDED=0 has no seeded blocks; that is reported, and is an error unless --unseeded is given.

The kernels at ArithKind::fold (q = 2^60 - d) use the folding blocks.  Their forward block (NTT16_CTF1 / NTT16_CTF1H, 18 / 17) is the
seeded block with u = fold(a) formed in a's own registers: it is held to the same aliasing checks (the shift reads, and the mask
reads and writes, v(L+1); the fold and both products of the low chain accumulate in v[L:L+1]).  For the inverse kernels a second
table counts the blocks per form -- select (NTT16_GS1 / GS1H, 20 / 19), folding (NTT16_GSF1 / GSF1H, 19 / 18), non-folding
(NTT16_GSN1 / GSN1H, 16 / 15) -- with their sizes; a fold-kind kernel must hold the non-folding blocks of the static range table
(28 of 104 in a 2^13 slice, 31 of 112 in a 2^14 slice: tools/gen_ntt16_bfly.py) and no select block, a Barrett-kind kernel select
blocks only.  The rows of the fold-kind transforms (not the tensor launch's, which was a fold-kind kernel before its butterflies
were) are printed under the heading "fold" and begin with "fold:"."""
import re
import subprocess
import sys

FIXED = set(range(119, 128))   # RegsS of tools/gen_ntt16_bfly.py, stream 0


def kernels(txt):
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end', txt, re.S | re.M):
        out[m.group(1)] = {'body': m.group(2)}
    for m in re.finditer(r'- \.agpr_count:.*?\.wavefront_size:\s+\d+', txt, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)
        if g('name') in out:
            out[g('name')]['regs'] = tuple(int(g(k)) for k in ('vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size'))
    return out


def short(name):
    d = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
    if d.endswith(')'):   # cut the parameter list: the parenthesis that matches the last one (an enum template argument has its own)
        depth, i = 0, len(d)
        while True:
            i -= 1
            depth += (d[i] == ')') - (d[i] == '(')
            if not depth:
                break
        d = d[:i]
    return re.sub(r'^void ', '', d).replace('piehip::', '')


def asm_blocks(body):
    for m in re.finditer(r';;#ASMSTART\n(.*?);;#ASMEND', body, re.S):
        yield [ln.strip() for ln in m.group(1).split('\n') if ln.strip()]


def ops(ln):
    return [o.strip() for o in ln.split(None, 1)[1].split(',')]


def pair(o):
    m = re.match(r'v\[(\d+):(\d+)\]$', o)
    return (int(m.group(1)), int(m.group(2))) if m else None


def is_forward(blk):
    # both forward blocks open with m1 = bl sh and t = a - 4q; the inverse opens with two v_lshl_add_u64
    return len(blk) >= 18 and blk[0].startswith('v_mad_u64_u32') and blk[1].startswith('v_lshl_add_u64') and any(
        ln.startswith('v_subb_co_u32') for ln in blk)


def is_forward_fold(blk):
    # the fold block opens with the shift and the mask of a's high word and has the seeded tail
    return (len(blk) >= 17 and blk[0].startswith('v_lshrrev_b32') and blk[1].startswith('v_and_b32') and ops(blk[1])[1] == '0xfffffff'
            and any(ln.startswith('v_subb_co_u32') for ln in blk))


def is_seeded(blk):
    return any(ln.startswith('v_lshl_add_u64') and ops(ln)[2] == '1' for ln in blk)


GS_SIZES = {'select': (19, 20), 'folding': (18, 19), 'non-folding': (15, 16)}


def inverse_form(blk):
    """-> 'select' | 'folding' | 'non-folding' for an inverse butterfly block, None for anything else"""
    if len(blk) < 15 or not blk[0].startswith('v_lshl_add_u64') or not any(ln.startswith('v_subb_co_u32') for ln in blk):
        return None
    if any(ln.startswith('v_bfi_b32') for ln in blk):
        return 'select'
    return 'folding' if any(ln.startswith('v_and_b32') for ln in blk) else 'non-folding'


def check_inverse(blk, form):
    bad = []
    if len(blk) not in GS_SIZES[form]:
        bad.append("%s block of %d instructions" % (form, len(blk)))
    for ln in blk:
        if ln.startswith(('v_mov', 's_nop', 'v_nop')):
            bad.append("has " + ln)
    i, j = (next(k for k, ln in enumerate(blk) if ln.startswith(p)) for p in ('v_sub_co_u32', 'v_subb_co_u32'))
    if j - i - 1 < 2 or any('vcc' in ln for ln in blk[i + 1:j]):
        bad.append("VCC wait states between the halves of the difference")
    return bad


# non-folding blocks of an inverse kernel at ArithKind::fold, by slice length (passes of 2, 4, 4, 3 and of 2, 4, 4, 4 stages)
NOFOLD = {104: 28, 112: 31}


def check_block(blk, fold=False):
    """-> list of complaints about one seeded forward block (fold: the block with u = fold(a) in a's registers)"""
    bad = []
    if len(blk) not in ((17, 18) if fold else (18, 19)):
        bad.append("%d instructions" % len(blk))
    for ln in blk:
        if ln.startswith(('v_mov', 's_nop', 'v_nop')):
            bad.append("has " + ln)
    mads = [ops(ln) for ln in blk if ln.startswith('v_mad_u64_u32')]
    low = [o for o in mads if pair(o[0]) and pair(o[0])[0] not in FIXED]
    if fold:
        if len(mads) != 10 or len(low) != 3 or len({o[0] for o in low}) != 1 or any(o[4] != o[0] for o in low):
            return bad + ["low chain not found: %r" % low]
    elif len(mads) != 9 or len(low) != 2 or low[0][0] != low[1][0] or low[1][4] != low[1][0]:
        return bad + ["low chain not found: %r" % low]
    lo, hi = pair(low[0][0])
    if hi != lo + 1 or {lo, hi} & FIXED:
        bad.append("a' in v[%d:%d]" % (lo, hi))
    if fold:   # bl, bh as the products name them: every multiplicand outside the fixed registers
        b_regs = {o[2] for o in mads if re.match(r'v\d+$', o[2]) and int(o[2][1:]) not in FIXED}
    else:
        b_regs = {low[0][2]} | {o[2] for o in mads[:3]}
    if {'v%d' % lo, 'v%d' % hi} & b_regs:
        bad.append("a' shares a register with b")
    sel = [ops(ln) for ln in blk if ln.startswith('v_bfi_b32')]
    sub = [ops(ln) for ln in blk if ln.startswith('v_sub_co_u32')]
    sbb = [ops(ln) for ln in blk if ln.startswith('v_subb_co_u32')]
    add = [ops(ln) for ln in blk if ln.startswith('v_add_u32')]
    if fold:
        shift, mask = ops(blk[0]), ops(blk[1])
        dbl = [ops(ln) for ln in blk if ln.startswith('v_lshl_add_u64') and ops(ln)[2] == '1']
        if sel or shift[2] != 'v%d' % hi or mask[0] != 'v%d' % hi or mask[2] != 'v%d' % hi:
            bad.append("shift and mask touch %r, a' is v[%d:%d]" % ([shift[2], mask[0], mask[2]], lo, hi))
        if len(dbl) != 1 or pair(dbl[0][1]) != (lo, hi):
            bad.append("2u + 4q reads %r, a' is v[%d:%d]" % ([d[1] for d in dbl], lo, hi))
    elif len(sel) != 2 or [s[2] for s in sel] != ['v%d' % lo, 'v%d' % hi]:
        bad.append("selects read %r, a' is v[%d:%d]" % ([s[2] for s in sel], lo, hi))
    if len(sub) != 1 or sub[0][3] != 'v%d' % lo:
        bad.append("v_sub_co_u32 reads %r, a' low is v%d" % ([s[3] for s in sub], lo))
    if len(add) != 1 or add[0][0] != 'v%d' % hi or add[0][1] != 'v%d' % hi:
        bad.append("v_add_u32 updates %r, a' high is v%d" % ([s[:2] for s in add], hi))
    if len(sbb) != 1 or sbb[0][3] != 'v%d' % hi:
        bad.append("v_subb_co_u32 reads %r, a' high is v%d" % ([s[3] for s in sbb], hi))
    if len(sub) == 1 and len(sbb) == 1:
        i, j = (next(k for k, ln in enumerate(blk) if ln.startswith(p)) for p in ('v_sub_co_u32', 'v_subb_co_u32'))
        if j - i - 1 < 2 or any('vcc' in ln for ln in blk[i + 1:j]):
            bad.append("VCC wait states between the halves of the difference")
    return bad


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    unseeded_ok = '--unseeded' in sys.argv
    ks = kernels(open(args[0]).read())
    ok = True
    print("%-62s %7s %8s %8s %9s %5s %5s %7s  %s" % ("kernel", "forward", "seeded", "aliased", "instr", "vgpr", "spill", "scratch", "verdict"))
    fold_rows, inv_rows = [], []
    for name, k in ks.items():
        blocks = list(asm_blocks(k['body']))
        fwd = [b for b in blocks if is_forward(b) or is_forward_fold(b)]
        seeded = [b for b in fwd if is_seeded(b)]
        complaints = [(i, c) for i, b in enumerate(seeded) for c in check_block(b, is_forward_fold(b))]
        is_fold = any(is_forward_fold(b) or inverse_form(b) in ('folding', 'non-folding') for b in blocks)
        transform = 'ntt16_kernel_t' in name   # (a harness kernel holds one block of whatever kind it was written for)
        if transform and is_fold and 'ArithKindE2' not in name:
            complaints.append((0, "folding blocks in a Barrett-kind kernel"))
        inv = [(b, inverse_form(b)) for b in blocks if inverse_form(b)]
        inv_bad = [c for b, f in inv for c in check_inverse(b, f)]
        if inv:
            n = {f: sum(1 for _, g in inv if g == f) for f in GS_SIZES}
            if transform and is_fold and (n['select'] or n['non-folding'] != NOFOLD.get(len(inv))):
                inv_bad.append("%d select and %d non-folding blocks of %d at the fold kind" % (n['select'], n['non-folding'], len(inv)))
            inv_rows.append((name, n, {f: "/".join(map(str, sorted({len(b) for b, g in inv if g == f}))) or "-" for f in GS_SIZES}, inv_bad))
        if transform and fwd and is_fold != all(is_forward_fold(b) for b in fwd):
            complaints.append((0, "forward blocks of the other kind"))
        aliased = len(seeded) - len({i for i, _ in complaints})
        sizes = sorted({len(b) for b in fwd})
        v, sp, sc = k['regs']
        verdict = []
        if 'ntt16_kernel_t' in name and (v != 128 or sp or sc):
            verdict.append("registers")
        if complaints:
            verdict.append("blocks")
        if inv_bad:
            verdict.append("inverse")
        if fwd and len(seeded) != len(fwd) and not (unseeded_ok and not seeded):
            verdict.append("%d unseeded" % (len(fwd) - len(seeded)))
        ok &= not verdict
        to_fold = is_fold and 'Lb1ELb0ELb1E' not in name   # a transform at the fold kind (the tensor launch's kernels stay in the first table)
        row = ["%-62s %7d %8d %8d %9s %5d %5d %7d  %s" % (("fold: " + short(name).replace('ntt16::', '', 1) if to_fold else short(name))[:62], len(fwd), len(seeded), aliased, "/".join(map(str, sizes)) or "-", v, sp, sc,
                                                          ", ".join(verdict) or "ok")]
        row += ["    block %d: %s" % (i, c) for i, c in complaints[:8]] + ["    inverse: %s" % c for c in inv_bad[:8]]
        if to_fold:
            fold_rows += row
        else:
            print("\n".join(row))
    if fold_rows:
        print("fold")
        print("\n".join(fold_rows))
    if inv_rows:
        print("inverse blocks")
        print("%-68s %7s %12s %12s %12s" % ("kernel", "blocks", "select", "folding", "non-folding"))
        for name, n, sz, _ in inv_rows:
            print("inv:  %-62s %7d %12s %12s %12s" % (short(name)[:62], sum(n.values()), *("%d x %s" % (n[f], sz[f]) if n[f] else "-" for f in GS_SIZES)))
    tot = sum(1 for k in ks.values() for b in asm_blocks(k['body']) if is_forward(b) or is_forward_fold(b))
    print("%d kernels, %d forward blocks: %s" % (len(ks), tot, "ok" if ok else "FAILED"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
