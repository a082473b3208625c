"""The folding butterflies in the compiler's output (beside tests/test_ct_seeded_listing.py, which keeps its ten rows): on the device
listing of kernels_ntt16.hip of this checkout (no GPU: hipcc cross-compiles), tools/ct_seeded_listing.py must find

  every forward block of the fold-kind transforms seeded and aliased, at 17 / 18 instructions (the block masks a's high word
  through the input ah and accumulates u = fold(a) in a's pair: right only while ah sits in the pair's high register);
  the inverse blocks of every kernel in exactly the two sizes of their form -- select 19 / 20, folding 18 / 19, non-folding 15 / 16;
  per fold-kind inverse kernel, the non-folding blocks of the static range table (tools/gen_ntt16_bfly.py: nofold_count) times the
  one instantiation of each pass the kernel holds, and no select block;
  128 VGPRs, no spill, no scratch in all sixteen instantiations;

and must refuse a copy in which one fold block's v_subb_co_u32 reads another register than the high half of a'.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "ct_seeded_listing.py")
LISTING = os.path.join(CSRC, "build", "kernels_ntt16.s")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ntt16_bfly as gen   # noqa: E402


def _check(path):
    return subprocess.run([sys.executable, TOOL, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)


def test_fold_blocks_of_the_listing(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "build/kernels_ntt16.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = _check(LISTING)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()

    # forward, seeded, aliased, instr, vgpr, spill, scratch, verdict -- of every instantiation, and of the fold-kind transforms
    rows = [ln.split() for ln in lines if ln.startswith(("ntt16::ntt16_kernel_t", "fold: "))]
    assert len(rows) == 16 and all(row[-4:] == ["128", "0", "0", "ok"] for row in rows), rows
    fold = [ln.split() for ln in lines if ln.startswith("fold: ")]
    assert len(fold) == 6 and all("(ArithKind)2>" in " ".join(row) for row in fold)
    fwd = [row for row in fold if int(row[-8]) > 0]
    assert sorted(int(row[-8]) for row in fwd) == [104, 112, 120, 128]      # 13 / 14 stages x 8, + 16 in the digit lift's load phase
    for row in fwd:
        assert row[-8] == row[-7] == row[-6] and row[-5] == "17/18", row

    # inverse blocks: "inv: <kernel> <blocks> <select> <folding> <non-folding>", each "<n> x <sizes>" or "-"
    inv = {}
    for ln in lines:
        m = re.match(r"inv:\s+(.*?>)\s+(\d+)\s+(-|\d+ x \S+)\s+(-|\d+ x \S+)\s+(-|\d+ x \S+)$", ln)
        if m:
            inv[m.group(1)] = (int(m.group(2)),) + tuple(None if g == "-" else (int(g.split(" x ")[0]), g.split(" x ")[1]) for g in m.groups()[2:])
    assert len(inv) == 8
    for name, (n, sel, fo, nf) in inv.items():
        logns = 13 if "<13u" in name else 14
        want_nf, want_n = gen.nofold_count(logns)
        assert n == want_n, name
        if name.endswith("(ArithKind)2>"):
            assert sel is None and nf == (want_nf, "15/16") and fo == (want_n - want_nf, "18/19"), (name, sel, fo, nf)
        else:
            assert sel == (want_n, "19/20") and fo is None and nf is None, (name, sel, fo, nf)

    # one fold block whose v_subb_co_u32 reads another register than the high half of a': refused
    txt = open(LISTING).read()
    m = re.search(r"(v_lshrrev_b32 v124, 28, (v\d+)\n\tv_and_b32 \2, 0xfffffff, \2\n(?:\t[^\n]*\n){12,14}?\tv_add_u32 \2, \2, v126\n"
                  r"\tv_subb_co_u32 v\d+, vcc, v121, )\2(, vcc)", txt)
    assert m, "no fold block tail in the listing"
    broken = tmp_path / "broken.s"
    broken.write_text(txt[:m.start()] + m.group(1) + "v0" + m.group(3) + txt[m.end():])
    r = _check(str(broken))
    assert r.returncode == 1 and "v_subb_co_u32 reads" in r.stdout, r.stdout
