"""The seeded forward butterfly's register contract, checked where it can break: in the compiler's output.

The block (csrc/ntt16_bfly.inc: NTT16_CTS1 / NTT16_CTS1H) reads and writes the halves of its tied operand a through the inputs al / ah,
which is right only while the register allocator keeps those in the two registers of a's pair.  tools/ct_seeded_listing.py asserts
that for every forward block of the device listing of kernels_ntt16.hip; here it runs on the listing of this checkout (no GPU: hipcc
cross-compiles), and on a copy with one block's subtrahend moved to another register, which it has to refuse.  Also: the committed
ntt16_bfly.inc is what tools/gen_ntt16_bfly.py writes.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "ct_seeded_listing.py")
LISTING = os.path.join(CSRC, "build", "kernels_ntt16.s")


def _check(path, *flags):
    return subprocess.run([sys.executable, TOOL, path] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)


def test_generated_blocks_are_the_committed_ones(tmp_path):
    out = tmp_path / "ntt16_bfly.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ntt16_bfly.py")], env=dict(os.environ, NTT16_BFLY_OUT=str(out)),
                          stdout=subprocess.DEVNULL)
    assert out.read_text() == open(os.path.join(CSRC, "ntt16_bfly.inc")).read()


def test_every_forward_block_of_the_listing_aliases(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "build/kernels_ntt16.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = _check(LISTING)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ntt16::ntt16_kernel_t")]
    fwd = [row for row in rows if int(row[-8]) > 0]
    assert len(rows) == 10 and len(fwd) == 4   # 2 slice lengths x {forward, forward with lift, inverse, tensor Barrett, tensor folded}
    for row in rows:     # forward, seeded, aliased, instr, vgpr, spill, scratch, verdict
        assert row[-8] == row[-7] == row[-6] and row[-4:] == ["128", "0", "0", "ok"], row
    assert all(row[-5] == "18/19" for row in fwd)

    # one block whose v_subb_co_u32 reads another register than the high half of a': refused
    txt = open(LISTING).read()
    m = re.search(r"(v_add_u32 (v\d+), \2, v126\n\tv_subb_co_u32 v\d+, vcc, v121, )\2(, vcc)", txt)
    assert m, "no seeded tail in the listing"
    broken = tmp_path / "broken.s"
    broken.write_text(txt[:m.start()] + m.group(1) + "v0" + m.group(3) + txt[m.end():])
    r = _check(str(broken))
    assert r.returncode == 1 and "v_subb_co_u32 reads" in r.stdout, r.stdout
