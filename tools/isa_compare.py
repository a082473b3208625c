"""per-kernel comparison of two hipcc -S listings of one file (before and after a change): python tools/isa_compare.py before.s after.s
Kernels that only the second listing has are listed with their figures; one that only the first has is an error.  A kernel counts as identical when its instructions, its kernel descriptor and its metadata entry are (the compilation-unit id,
__hip_cuid_<hash>, neutralised); for the others: tools/isa_regs.py's columns, waves per SIMD, instruction totals and the counts of the
memory and multiplier instructions, each as before->after where it changed."""
import collections
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    txt = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', txt)
    out = collections.OrderedDict()
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end', txt, re.S | re.M):
        out[m.group(1)] = {'body': m.group(2)}
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', txt, re.S | re.M):
        out[m.group(1)]['desc'] = m.group(2)
    for m in re.finditer(r'- \.agpr_count:.*?\.wavefront_size:\s+\d+', txt, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)
        out[g('name')]['meta'] = blk
        out[g('name')]['regs'] = tuple(int(g(k)) for k in ('vgpr_count', 'vgpr_spill_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size'))
    return out, txt


def mix(body):
    c = collections.Counter()
    for ln in body.split('\n'):
        ln = ln.strip()
        if not ln or ln[0] in '.;/' or ln.endswith(':'):
            continue
        c[ln.split()[0]] += 1
    return c


def fam(c, prefix):
    return sum(v for k, v in c.items() if k.startswith(prefix))


FAMS = ('global_load_', 'global_store_', 'v_mad_u64_u32', 'v_mul_hi_u32', 'v_mul_lo_u32', 'v_lshl_add_u64')


def short(name):
    d = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
    m = re.match(r'void piehip::(\w+(<[^(]*>)?)\(', d)
    return m.group(1) if m else d.split('(')[0].replace('piehip::', '')


def waves(v):
    return min(8, 512 // ((v + 7) // 8 * 8))


pa, pt = kernels(sys.argv[1])
he, ht = kernels(sys.argv[2])
gone = [k for k in pa if k not in he]
new = [k for k in he if k not in pa]
assert not gone, "kernels of the first listing missing from the second: %s" % gone
same = [k for k in pa if pa[k] == he[k]]
diff = [k for k in pa if pa[k] != he[k]]
print("%d kernels, %d with identical listing (instructions, kernel descriptor, metadata), %d differ" % (len(pa), len(same), len(diff)))
print("whole listing identical" if pt == ht else "whole listing differs")
if new:   # kernels only the second listing has: their register figures and instruction totals
    print()
    print("%d kernels only in the second listing:" % len(new))
    for k in new:
        r, c = he[k]['regs'], mix(he[k]['body'])
        print("  %-52s vgpr %3d spill %d sgpr %3d scratch %3d waves %d instructions %5d  v_cndmask_b32 %d" % (
            short(k), r[0], r[1], r[2], r[3], waves(r[0]), sum(c.values()), c['v_cndmask_b32']))
print()
print("identical, by kernel template: " + ", ".join("%s x %d" % kv for kv in collections.Counter(re.sub(r'<.*', '', short(k)) for k in same).items()))
print()
print("kernels whose listing differs (parent -> this tree):")
print("%-46s %-11s %-5s %-9s %-7s %-5s %-15s %-9s %-9s %-11s %-9s %-9s %-9s %s" % (
    "kernel", "vgpr", "spill", "sgpr", "scratch", "waves", "instructions", "g_load", "g_store", "mad_u64_u32", "mul_hi", "mul_lo", "lshl_add", "other mnemonics that differ"))
ok = True
for k in diff:
    a, b = pa[k], he[k]
    ca, cb = mix(a['body']), mix(b['body'])
    ta, tb = sum(ca.values()), sum(cb.values())
    cols = ["%d->%d" % (fam(ca, f), fam(cb, f)) if fam(ca, f) != fam(cb, f) else "%d" % fam(ca, f) for f in FAMS]
    others = sorted(m for m in set(ca) | set(cb) if ca[m] != cb[m] and not m.startswith(FAMS))
    ra, rb = a['regs'], b['regs']
    pr = lambda i: ("%d->%d" % (ra[i], rb[i])) if ra[i] != rb[i] else "%d" % ra[i]
    wa, wb = waves(ra[0]), waves(rb[0])
    print("%-46s %-11s %-5s %-9s %-7s %-5s %-15s %-9s %-9s %-11s %-9s %-9s %-9s %s" % (
        short(k), pr(0), pr(1), pr(2), pr(3), ("%d->%d" % (wa, wb)) if wa != wb else "%d" % wa,
        "%d->%d (%+.2f%%)" % (ta, tb, 100.0 * (tb - ta) / ta), *cols, " ".join("%s %+d" % (m, cb[m] - ca[m]) for m in others)))
