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
A listing built with -DNTT16_CT_SEEDED=0 has no seeded blocks; that is reported, and is an error unless --unseeded is given."""
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


def is_seeded(blk):
    return any(ln.startswith('v_lshl_add_u64') and ops(ln)[2] == '1' for ln in blk)


def check_block(blk):
    """-> list of complaints about one seeded forward block"""
    bad = []
    if len(blk) not in (18, 19):
        bad.append("%d instructions" % len(blk))
    for ln in blk:
        if ln.startswith(('v_mov', 's_nop', 'v_nop')):
            bad.append("has " + ln)
    mads = [ops(ln) for ln in blk if ln.startswith('v_mad_u64_u32')]
    low = [o for o in mads if pair(o[0]) and pair(o[0])[0] not in FIXED]
    if len(mads) != 9 or len(low) != 2 or low[0][0] != low[1][0] or low[1][4] != low[1][0]:
        return bad + ["low chain not found: %r" % low]
    lo, hi = pair(low[0][0])
    if hi != lo + 1 or {lo, hi} & FIXED:
        bad.append("a' in v[%d:%d]" % (lo, hi))
    b_regs = {low[0][2]} | {o[2] for o in mads[:3]}   # bl, bh as the products name them
    if {'v%d' % lo, 'v%d' % hi} & b_regs:
        bad.append("a' shares a register with b")
    sel = [ops(ln) for ln in blk if ln.startswith('v_bfi_b32')]
    sub = [ops(ln) for ln in blk if ln.startswith('v_sub_co_u32')]
    sbb = [ops(ln) for ln in blk if ln.startswith('v_subb_co_u32')]
    add = [ops(ln) for ln in blk if ln.startswith('v_add_u32')]
    if len(sel) != 2 or [s[2] for s in sel] != ['v%d' % lo, 'v%d' % hi]:
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
    for name, k in ks.items():
        fwd = [b for b in asm_blocks(k['body']) if is_forward(b)]
        seeded = [b for b in fwd if is_seeded(b)]
        complaints = [(i, c) for i, b in enumerate(seeded) for c in check_block(b)]
        aliased = len(seeded) - len({i for i, _ in complaints})
        sizes = sorted({len(b) for b in fwd})
        v, sp, sc = k['regs']
        verdict = []
        if 'ntt16_kernel_t' in name and (v != 128 or sp or sc):
            verdict.append("registers")
        if complaints:
            verdict.append("blocks")
        if fwd and len(seeded) != len(fwd) and not (unseeded_ok and not seeded):
            verdict.append("%d unseeded" % (len(fwd) - len(seeded)))
        ok &= not verdict
        print("%-62s %7d %8d %8d %9s %5d %5d %7d  %s" % (short(name)[:62], len(fwd), len(seeded), aliased, "/".join(map(str, sizes)) or "-", v, sp, sc,
                                                        ", ".join(verdict) or "ok"))
        for i, c in complaints[:8]:
            print("    block %d: %s" % (i, c))
    tot = sum(1 for k in ks.values() for b in asm_blocks(k['body']) if is_forward(b))
    print("%d kernels, %d forward blocks: %s" % (len(ks), tot, "ok" if ok else "FAILED"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
