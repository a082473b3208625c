"""tools/instantiation_coverage.py: the parsing and the set arithmetic on a small listing and two trace files written here (no GPU, no
build), and the committed record of profiles/instantiation_coverage: every kernel the traced suite still does not launch is listed as
unreachable, with the host condition that excludes it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import instantiation_coverage as ic   # noqa: E402

REC = os.path.join(ROOT, "profiles", "instantiation_coverage")

# five kernels of the library in three families, and one device function that is no kernel
K_E1 = "_ZN6piehip13expand_kernelILb0ELb0ELj1ELNS_9ArithKindE0ELb0EEEvPKNS_9DevConstsEjPKmmmPmjj"
K_E2 = "_ZN6piehip13expand_kernelILb1ELb0ELj2ELNS_9ArithKindE2ELb0EEEvPKNS_9DevConstsEjPKmmmPmjj"
K_D1 = "_ZN6piehip16limb_drop_kernelILi2ELi1EEEvPKNS_9DevConstsEjjPKmPm"
K_D2 = "_ZN6piehip16limb_drop_kernelILi3ELi1EEEvPKNS_9DevConstsEjjPKmPm"
K_P = "_ZN6piehip14permute_kernelEjPKmPKjPm"
DEVFN = "_ZN6piehip9barrett64Em"
K_LIB = "_ZN7rocprim6detail17trampoline_kernelILi950EEEvPj"      # a library header's kernel in our listing


def listing(names, devfns=()):
    txt = "\t.text\n"
    for n in list(names) + list(devfns):
        txt += "%s:                                  ; @%s\n\ts_endpgm\n.Lfunc_end0:\n" % (n, n)
    for n in names:
        txt += "\t.amdhsa_kernel %s\n\t\t.amdhsa_next_free_vgpr 8\n\t.end_amdhsa_kernel\n" % n
    txt += "amdhsa.kernels:\n"
    for n in names:
        txt += ("  - .agpr_count:     0\n    .group_segment_fixed_size: 0\n    .name:           %s\n    .private_segment_fixed_size: 0\n"
                "    .sgpr_count:     10\n    .symbol:         %s.kd\n    .vgpr_count:     8\n    .vgpr_spill_count: 0\n"
                "    .wavefront_size: 64\n") % (n, n)
    return txt


@pytest.fixture()
def built(tmp_path):
    (tmp_path / "a.s").write_text(listing([K_E1, K_E2, K_D1], [DEVFN]))
    (tmp_path / "b.s").write_text(listing([K_D2, K_P, K_LIB]))
    return {"a.hip": ic.built_kernels(str(tmp_path / "a.s")), "b.hip": ic.built_kernels(str(tmp_path / "b.s"))}


def test_listing_kernels_only(built):
    assert built == {"a.hip": [K_E1, K_E2, K_D1], "b.hip": [K_D2, K_P, K_LIB]}


def test_mangled_traces_of_several_processes(built, tmp_path):
    d1, d2 = tmp_path / "t1" / "sub", tmp_path / "t2"
    d1.mkdir(parents=True)
    d2.mkdir()
    (d1 / "11_kernel_stats.csv").write_text('"Name","Calls","TotalDurationNs"\n"%s.kd",3,100\n"__amd_rocclr_copyBuffer.kd",1,5\n' % K_E2)
    (d1 / "12_kernel_stats.csv").write_text('"Name","Calls","TotalDurationNs"\n"%s.kd",1,7\n' % K_P)
    (d2 / "9_kernel_trace.csv").write_text('"Kind","Agent_Id","Kernel_Name","Start_Timestamp"\n"KERNEL_DISPATCH",1,"%s.kd",1\n' % K_D1)
    (d2 / "9_agent_info.csv").write_text('"Name"\n"%s"\n' % K_D2)      # not a kernel file: not read
    names, nfiles = ic.launched_names([str(tmp_path / "t1"), str(d2)])
    assert nfiles == 3 and names == {K_E2 + ".kd", K_P + ".kd", K_D1 + ".kd", "__amd_rocclr_copyBuffer.kd"}
    rows, unlaunched, mode, others = ic.coverage(built, names)
    assert mode == "mangled" and others == 1
    assert rows == [("a.hip", "expand_kernel", 2, 1, 1), ("a.hip", "limb_drop_kernel", 1, 1, 0),
                    ("b.hip", "limb_drop_kernel", 1, 0, 1), ("b.hip", "permute_kernel", 1, 1, 0),
                    ("b.hip", "rocprim::detail::trampoline_kernel", 1, 0, 1)]
    assert unlaunched == ["expand_kernel<false, false, 1u, (ArithKind)0, false>", "limb_drop_kernel<3, 1>"]
    rep = ic.report(rows, unlaunched, mode, nfiles, others)
    assert rep.startswith("names matched: mangled (3 csv files read)")
    assert rep.endswith("not launched:\nexpand_kernel<false, false, 1u, (ArithKind)0, false>\nlimb_drop_kernel<3, 1>\n\n"
                        "and 1 kernels of other namespaces (--all-namespaces lists them)\n")
    assert ic.coverage(built, names, all_namespaces=True)[1:] == (unlaunched + ["rocprim::detail::trampoline_kernel<950>"], mode, 0)
    # a second trace directory only ever adds
    (d2 / "10_kernel_stats.csv").write_text('"Name","Calls"\n"%s.kd",1\n' % K_D2)
    names2, _ = ic.launched_names([str(tmp_path / "t1"), str(d2)])
    assert ic.coverage(built, names2)[1] == ["expand_kernel<false, false, 1u, (ArithKind)0, false>"]


def test_demangled_traces_match_the_same_kernels(built):
    names = {"void piehip::expand_kernel<true, false, 2u, (piehip::ArithKind)2, false>(piehip::DevConsts const*, unsigned int, "
             "unsigned long const*, unsigned long, unsigned long, unsigned long*, unsigned int, unsigned int)",
             "piehip::permute_kernel(unsigned int, unsigned long const*, unsigned int const*, unsigned long*)"}
    rows, unlaunched, mode, _ = ic.coverage(built, names)
    assert mode == "demangled"
    assert unlaunched == ["expand_kernel<false, false, 1u, (ArithKind)0, false>", "limb_drop_kernel<2, 1>", "limb_drop_kernel<3, 1>"]


def test_nothing_launched(built):
    rows, unlaunched, mode, others = ic.coverage(built, set())
    assert [r[3] for r in rows] == [0, 0, 0, 0, 0] and len(unlaunched) == 5 and others == 1


def test_makefile_files():
    files = ic.makefile_hip_files()
    assert {"kernels_pie", "kernels_stage_a", "kernels_convert", "kernels_chain_drop", "kernels_keyswitch", "kernels_slice", "kernels_ntt16",
            "kernels_ntt_fast"} <= set(files)
    assert all(os.path.exists(os.path.join(ic.CSRC, f + ".hip")) for f in files)


def _lines(name):
    return [ln.rstrip("\n") for ln in open(os.path.join(REC, name)) if ln.strip()]


def _reasons():
    reasons = {}
    for ln in _lines("unreachable.txt"):
        name, _, reason = ln.partition("\t")
        assert len(reason.strip()) >= 20, "no reason: %r" % ln
        assert name not in reasons, "listed twice: %s" % name
        reasons[name] = reason
    return reasons


def test_what_is_still_unlaunched_is_listed_as_unreachable_with_a_reason():
    before, after = _lines("before_unlaunched.txt"), _lines("after_unlaunched.txt")
    reasons = _reasons()
    assert set(after) <= set(before), "the new cases only add launches"
    missing = [n for n in after if n not in reasons]
    assert not missing, "unlaunched and not listed as unreachable: %s" % missing


def test_the_unreachable_kernels_are_not_built():
    """removed.txt: the 19 kernels of unreachable.txt and the six expand_both_kernel<true, L, K, false> that only tests/lazy_inputs
    selected.  The device listings of this checkout (no GPU: hipcc cross-compiles) hold none of them, and exactly the rest of the
    two families"""
    import subprocess
    import isa_compare
    removed = set(_lines("removed.txt"))
    assert len(removed) == 25 and set(_reasons()) <= removed
    subprocess.check_call(["make", "-j2", "-C", ic.CSRC, "build/kernels_convert.s", "build/kernels_ntt_fast.s"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    names = [isa_compare.short(k) for f in ("kernels_convert", "kernels_ntt_fast") for k in ic.built_kernels(os.path.join(ic.CSRC, "build", f + ".s"))]
    assert not removed & set(names)
    count = lambda fam: sum(n.startswith(fam + "<") for n in names)
    assert count("expand_both_kernel") == 63 and count("ntt_fast_kernel") == 11


def test_every_kernel_the_suite_did_not_launch_has_a_case_or_a_reason():
    """tests/test_gpu_instantiations.py names one instantiation per case: together with unreachable.txt its rows are exactly the
    kernels of before_unlaunched.txt, none twice, and each row says which dispatcher selects it"""
    from tests import test_gpu_instantiations as gi
    before, reasons = _lines("before_unlaunched.txt"), _reasons()
    rows = [r[0] for r in gi.ROWS]
    assert len(set(rows)) == len(rows) and not set(rows) & set(reasons)
    assert set(rows) | set(reasons) == set(before)
    for name, driver, _, why in gi.ROWS:
        assert driver in gi.DRIVERS and len(why) >= 20, name
