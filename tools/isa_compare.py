"""per-kernel comparison of two hipcc -S listings of one file (before and after a change):
    python tools/isa_compare.py [--removed FILE] [--renamed FILE] [--neutral-ordinals] before.s after.s [after2.s ...]
Several "after" listings: the file was cut into these (each kernel in exactly one of them); they are read as one listing.
Kernels that only the second listing has are listed with their figures; one that only the first has is an error.  A kernel counts as
identical when its instructions, its kernel descriptor and its metadata entry are (the compilation-unit id, __hip_cuid_<hash>,
neutralised); for the others: tools/isa_regs.py's columns, waves per SIMD, instruction totals and the counts of the memory and
multiplier instructions, each as before->after where it changed.
--removed FILE: the kernels the change removes on purpose, one per line, as this tool prints them (e.g. expand_kernel<true, true, 3u,
false, false>) or mangled.  They may be missing from the second listing and are listed by name; any OTHER kernel missing there, and a
named one that is still there, stays an error.
--renamed FILE: the kernels the change renames, one pair per line, old<TAB>new, each as this tool prints kernel names or mangled (a
change of a template's parameter list renames every instantiation).  A pair is compared as ONE kernel: each side's own mangled name is
replaced by a fixed word in its body, its descriptor and its metadata entry first.  The pairs are listed as renamed, not as removed and
new; a pair whose old name the first listing lacks, or whose new name the second lacks, is an error.
--neutral-ordinals: the compiler numbers the functions of a listing and puts that ordinal into local labels (.LBB<f>_<n>, and BB<f>_<n>
inside comments), so taking out or reordering one kernel renames the labels of every kernel behind it.  With this option the ordinal
is replaced by a fixed letter in both listings before anything is compared, and the padding between a label and the comment behind it
(which depends on the label's length) by one blank; the label's own number <n> stays."""
import argparse
import collections
import re
import subprocess
import sys


def kernels(path, neutral_ordinals):
    txt = open(path).read()
    txt = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', txt)
    if neutral_ordinals:
        txt = re.sub(r'\bL?BB\d+_(\d+)', r'BBf_\1', txt)
        txt = re.sub(r'^(\.BBf_\d+:)[ \t]+', r'\1 ', txt, flags=re.M)   # (the comment behind a label starts at a fixed column)
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


SHORT = {}


def short(name):
    """the demangled name without return type, parameter list and piehip:: (template arguments may hold parentheses: enum values)"""
    if name not in SHORT:
        d = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
        if d.endswith(')'):   # cut the parameter list: the parenthesis that matches the last one
            depth, i = 0, len(d)
            while True:
                i -= 1
                depth += (d[i] == ')') - (d[i] == '(')
                if not depth:
                    break
            d = d[:i]
        SHORT[name] = re.sub(r'^void ', '', d).replace('piehip::', '')
    return SHORT[name]


def find(listing, name, which):
    """the mangled name of `name` (mangled, or as short() prints it) in a listing"""
    hits = [k for k in listing if k == name or short(k) == re.sub(r'^void ', '', name)]
    assert len(hits) == 1, "--renamed: %s is not a kernel of the %s listing" % (name, which)
    return hits[0]


def unnamed(entry, own):
    return {k: v.replace(own, 'KERNEL') if isinstance(v, str) else v for k, v in entry.items()}


def waves(v):
    return min(8, 512 // ((v + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--removed", default=None)
    ap.add_argument("--renamed", default=None)
    ap.add_argument("--neutral-ordinals", action="store_true")
    ap.add_argument("before")
    ap.add_argument("after", nargs="+")
    args = ap.parse_args()
    pa, pt = kernels(args.before, args.neutral_ordinals)
    he, ht = collections.OrderedDict(), ""
    for path in args.after:
        part, txt = kernels(path, args.neutral_ordinals)
        twice = [short(k) for k in part if k in he]
        assert not twice, "kernels that more than one of the second listings has: %s" % twice
        he.update(part)
        ht += txt
        if len(args.after) > 1:
            print("second listing, part: %s (%d kernels)" % (path, len(part)))
    renamed = []
    if args.renamed:
        for ln in open(args.renamed):
            if ln.strip():
                old, new = ln.rstrip('\n').split('\t')
                renamed.append((find(pa, old.strip(), "first"), find(he, new.strip(), "second")))
        assert len(set(o for o, n in renamed)) == len(renamed) == len(set(n for o, n in renamed)), "--renamed: a name occurs twice"
        # from here on a pair is one kernel under its old name
        moved = {o: unnamed(he[n], n) for o, n in renamed}
        for o, n in renamed:
            del he[n]
        clash = [short(o) for o in moved if o in he]
        assert not clash, "--renamed: old names the second listing still has: %s" % clash
        for o, n in renamed:
            pa[o] = unnamed(pa[o], o)
        he.update(moved)
    removed = set(ln.strip() for ln in open(args.removed) if ln.strip()) if args.removed else set()
    gone = [k for k in pa if k not in he]
    new = [k for k in he if k not in pa]
    named = [k for k in pa if k in removed or short(k) in removed]
    unexpected = [short(k) for k in gone if k not in named]
    assert not unexpected, "kernels of the first listing missing from the second: %s" % unexpected
    assert not [k for k in named if k in he], "kernels named as removed that the second listing still has: %s" % [short(k) for k in named if k in he]
    assert len(named) == len(removed), "names in --removed that the first listing does not have"
    if gone:
        print("%d kernels removed on purpose (--removed), missing from the second listing:" % len(gone))
        for k in gone:
            print("  " + short(k))
        print()
        for k in gone:
            del pa[k]
    if renamed:
        print("%d kernels renamed (--renamed), each pair compared as one kernel, its own name neutralised:" % len(renamed))
        for o, n in renamed:
            print("  %s -> %s%s" % (short(o), short(n), "" if pa[o] == he[o] else "   DIFFERS"))
        print()
    if args.neutral_ordinals:
        print("(function ordinals in local labels neutralised)")
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


if __name__ == "__main__":
    main()
