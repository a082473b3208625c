"""The hand-written arithmetic blocks of csrc/ on the device against exact integer arithmetic: tests/arith_check, a program of its
own that compiles the product's definitions (modarith.h, madasm.h, stage_a_common.h, pie_arith.h, ntt_bfly.h, ntt16_kernel.h)
into one small kernel per block.  One case per group; each runs the program once as a fresh child process and asserts its exit
status, every block's failures, the coverage of every quotient estimate's errors and, for the lazy forms, that the multiple of q
the device leaves equals the host model's case for case (tests/arith_chains.py: check_report)."""
import os
import subprocess

import pytest

from tests import arith_chains as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
EXE = os.path.join(CSRC, "build", "arith_check")

GROUPS = {
    "modarith": ("barrett128", "mulmod", "reduce123", "reduce124", "mul_shoup_lazy", "mul_shoup", "divmod_shoup", "fixfrac", "add128", "mac128"),
    "madasm": ("colacc_mac+carry+value", "colacc_mac2"),
    "stage_a": ("addmod_nb", "colacc_reduce123_lazy", "colacc_reduce<false>", "colacc_reduce<true>"),
    "pie": ("sel_neg/csub_u", "divmod_shoup_u", "mul_shoup_u", "mul_shoup_lazy_u", "reduce123_u", "shoup63_lazy", "shoup63", "divmod63",
            "mulhi_sb", "mfixfrac<asm>,<c>", "colacc_mac_small")
           + tuple("dot128<%d,%s>" % (n, m) for n in (1, 2, 4, 7, 8) for m in ("mul", "mad"))
           + tuple("crt_out<%d,%s>" % (n, m) for n in (1, 2, 4, 7, 8) for m in ("mul", "mad"))
           + tuple("crt_out<%d,mad,lazy>" % n for n in (1, 2, 4, 7)),
    "ntt": ("shoup4", "ct_bfly", "gs_bfly", "lift_digit<qi<2qj>", "lift_digit<qi>=2qj>"),
    "ntt16": tuple(b for b in ac.SHOUP63_BLOCKS if b.startswith("bfly<")) + ("csub_neg", "csub2_neg", "colacc123_to_4q"),
}
_stopped = []   # why no further case may start the program: after a fault or a hang nothing more runs on the GPU


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_arith_blocks_hold_their_contracts_on_the_device(group):
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    subprocess.check_call(["make", "-j8", "-C", CSRC, "build/arith_check"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EXE), "csrc/Makefile did not build " + EXE
    try:
        r = subprocess.run([EXE, group] + ac.chains(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    except subprocess.TimeoutExpired:
        _stopped.append("arith_check %s ran into its time limit" % group)
        raise
    print(r.stdout)
    if r.returncode < 0 or r.returncode not in (0, 1, 2):
        _stopped.append("arith_check %s ended with status %d" % (group, r.returncode))
    assert r.returncode == 0, "status %d\n%s" % (r.returncode, r.stdout[-6000:])
    assert "arith group %s ok" % group in r.stdout
    ac.check_report(ac.parse(r.stdout), GROUPS[group])
