"""host/WireFraming.hpp: messages of two- and three-component ciphertext rows (packRows / checkedRowsHeader / unpackRows).
tests/wire_rows_check.cpp round-trips both through a socket pair, compares a two-component message with packCiphertexts' byte for byte,
and has every malformed message refused: a length that does not match the component count in the header, a count other than 0, 2 or 3
there.  Built with the host compiler, plain and under AddressSanitizer + UndefinedBehaviorSanitizer with their runtimes linked into the
program, and run as a plain executable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("kind", ["plain", "sanitized"])
def test_rows_round_trip_and_refusals(tmp_path, kind):
    exe = str(tmp_path / "wire_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + (SAN if kind == "sanitized" else []) +
                          ["-o", exe, os.path.join(ROOT, "tests", "wire_rows_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "wire rows ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
