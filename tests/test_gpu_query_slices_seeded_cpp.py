"""tests/query_slices_seeded_check.cpp, built and run the way tests/query_slices_check.cpp is: the seeded calls of
host/QuerySlicedBatchedFHEHIPPIE.hpp on three handles against its unseeded calls on three more, as a fresh child process."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_seeded_matches_the_unseeded_facade(tmp_path):
    libdir = os.path.join(ROOT, "nested_hashing_psi_amd")
    exe = str(tmp_path / "query_slices_seeded_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "query_slices_seeded_check.cpp"),
                           "-L" + libdir, "-lpiehip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    assert "seeded query slices check ok: 3 handles, 2 queries per run, 5 result ciphertexts each" in out.stdout
