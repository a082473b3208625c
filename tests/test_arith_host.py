"""The host pass of csrc/modarith.h against exact integer arithmetic (tests/arith_check/host_check.cpp): barrett128, mulmod,
reduce123 / reduce124, mul_shoup_lazy, mul_shoup, divmod_shoup, fixfrac, add128, mac128 at uniform operands, the ends of their
contracts and the directed families that reach the largest error of each quotient estimate.  Built with the host compiler under
AddressSanitizer + UndefinedBehaviorSanitizer (runtimes linked into the program) and run as a plain executable."""
import os
import subprocess

from tests import arith_chains as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")


def test_modarith_host_pass_holds_its_contracts_at_worst_case_operands(tmp_path):
    exe = str(tmp_path / "arith_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "arith_check", "host_check.cpp"), os.path.join(CSRC, "params.cpp")])
    r = subprocess.run([exe] + ac.chains(), capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "arith host ok" in r.stdout
    rep = ac.parse(r.stdout)
    ac.check_report(rep, ("barrett128", "mulmod", "reduce123", "reduce124", "mul_shoup_lazy", "mul_shoup", "divmod_shoup", "fixfrac",
                          "add128", "mac128"))
    for t in (ac.T16, ac.T32, ac.T40, ac.T48):   # the plaintext moduli as Mod
        assert ("fixfrac", t) in rep and ("divmod_shoup", t) in rep
