"""Which compiled kernels does a traced run launch?
    python tools/instantiation_coverage.py [--listings DIR] [--no-make] [--unlaunched FILE] [--all-namespaces] TRACE_DIR [TRACE_DIR ...]
Built set: the kernel symbols of the device listings (csrc/build/<file>.s, `make listings` of csrc/Makefile) of every .hip file the
Makefile's SRCS names, parsed by kernels() of tools/isa_compare.py.  Launched set: the kernel names of every *_kernel_stats.csv and
*_kernel_trace.csv found under the TRACE_DIRs (rocprofv3 --output-format csv --kernel-trace --stats), whichever process wrote them.
Only names are read: no instruction text, no durations.

Matching: on MANGLED names where the traces hold them (rocprofv3 -M / --mangled-kernels; the ".kd" the profiler appends is cut).
Traces with demangled names are matched on the demangled text instead: the listing's names go through llvm-cxxfilt and both sides
lose their blanks.  The first line of the output says which was used.

Output: one row per source file and template family (built, launched, not launched), then the unlaunched kernels, one per line, as
tools/isa_compare.py prints kernel names (--unlaunched FILE writes that list, sorted, to a file as well).

The list names this library's kernels (namespace piehip).  Kernels that a library header instantiates into a listing (rocprim's,
behind hipcub::DeviceRadixSort in kernels_hash.hip: names of a kilobyte each, most of them for other target architectures) have
their rows in the table and one closing count; --all-namespaces lists them by name as well."""
import argparse
import collections
import csv
import glob
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_compare   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")


def makefile_hip_files(makefile=os.path.join(CSRC, "Makefile")):
    """the .hip files of the Makefile's SRCS, without the extension"""
    m = re.search(r'^SRCS\s*=\s*(.*)$', open(makefile).read(), re.M)
    return [os.path.splitext(w)[0] for w in m.group(1).split() if w.endswith(".hip")]


def built_kernels(listing):
    """the mangled names of the kernels (functions with a kernel descriptor) of one device listing"""
    ks, _ = isa_compare.kernels(listing, False)
    return [k for k, v in ks.items() if 'desc' in v]


def launched_names(dirs):
    """(names, number of csv files read): the kernel-name column of every stats and trace csv under the directories"""
    names, nfiles = set(), 0
    for d in dirs:
        for pat in ("*_kernel_stats.csv", "*_kernel_trace.csv"):
            for p in glob.glob(os.path.join(d, "**", pat), recursive=True):
                nfiles += 1
                with open(p, newline="") as f:
                    rd = csv.DictReader(f)
                    col = "Kernel_Name" if "Kernel_Name" in (rd.fieldnames or ()) else "Name"
                    for row in rd:
                        if row.get(col):
                            names.add(row[col])
    return names, nfiles


def strip_kd(n):
    return n[:-3] if n.endswith(".kd") else n


def squeeze(s):
    return re.sub(r'\s+', '', s)


def cxxfilt():
    """llvm-cxxfilt: on the PATH, or beside ROCm's compiler"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path=os.path.join(rocm, "llvm", "bin")) or "c++filt"


def demangle_all(names):
    out = subprocess.run([cxxfilt()] + list(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, out))


def match(built, launched):
    """(the built names that were launched, 'mangled' or 'demangled').  built: mangled names; launched: as the traces spell them"""
    launched = set(strip_kd(n) for n in launched)
    mangled = [n for n in launched if n.startswith("_Z")]
    if mangled or not launched:
        return set(b for b in built if b in launched), "mangled"
    dem = demangle_all(sorted(built))
    want = set(squeeze(n) for n in launched)
    return set(b for b in built if squeeze(dem[b]) in want), "demangled"


def family(mangled):
    return re.sub(r'<.*', '', isa_compare.short(mangled))


OWN = "_ZN6piehip"   # the library's kernels: namespace piehip (and the namespaces inside it)


def coverage(built_by_file, launched, all_namespaces=False):
    """rows (file, family, built, launched, not launched), the sorted unlaunched names as isa_compare prints them -- the library's own,
    or all --, the mode, and the number of unlaunched kernels of other namespaces that the list leaves out"""
    every = [k for ks in built_by_file.values() for k in ks]
    hit, mode = match(every, launched)
    rows = []
    for f, ks in built_by_file.items():
        fams = collections.OrderedDict()
        for k in ks:
            fams.setdefault(family(k), []).append(k)
        for fam, members in fams.items():
            n = sum(k in hit for k in members)
            rows.append((f, fam, len(members), n, len(members) - n))
    miss = set(k for k in every if k not in hit)
    listed = set(k for k in miss if all_namespaces or k.startswith(OWN))
    return rows, sorted(set(isa_compare.short(k) for k in listed)), mode, len(miss - listed)


def report(rows, unlaunched, mode, nfiles, others=0):
    out = ["names matched: %s (%d csv files read)" % (mode, nfiles), "",
           "%-22s %-34s %6s %9s %13s" % ("file", "family", "built", "launched", "not launched")]
    for f, fam, b, l, u in rows:
        out.append("%-22s %-34s %6d %9d %13d" % (f, fam, b, l, u))
    out.append("%-22s %-34s %6d %9d %13d" % ("all", "", sum(r[2] for r in rows), sum(r[3] for r in rows), sum(r[4] for r in rows)))
    out += ["", "not launched:"] + unlaunched
    if others:
        out += ["", "and %d kernels of other namespaces (--all-namespaces lists them)" % others]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--listings", default=os.path.join(CSRC, "build"))
    ap.add_argument("--no-make", action="store_true", help="read the listings as they are, do not bring them up to date")
    ap.add_argument("--unlaunched", default=None)
    ap.add_argument("--all-namespaces", action="store_true", help="list the unlaunched kernels of library headers (rocprim) too")
    ap.add_argument("traces", nargs="+")
    args = ap.parse_args()
    files = makefile_hip_files()
    if not args.no_make:
        subprocess.check_call(["make", "-C", CSRC, "listings"], stdout=subprocess.DEVNULL)
    built = collections.OrderedDict((f + ".hip", built_kernels(os.path.join(args.listings, f + ".s"))) for f in files)
    launched, nfiles = launched_names(args.traces)
    assert nfiles, "no *_kernel_stats.csv or *_kernel_trace.csv under %s" % args.traces
    rows, unlaunched, mode, others = coverage(built, launched, args.all_namespaces)
    sys.stdout.write(report(rows, unlaunched, mode, nfiles, others))
    if args.unlaunched:
        open(args.unlaunched, "w").write("".join(n + "\n" for n in unlaunched))


if __name__ == "__main__":
    main()
