"""tests/query_slices_check.cpp, built and run the way tests/result_limbs_check.cpp is: host/QuerySlicedBatchedFHEHIPPIE.hpp with four
handles on one device against the unsliced C++ facade, as a fresh child process."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_with_four_handles_matches_the_unsliced_facade(tmp_path):
    libdir = os.path.join(ROOT, "nested_hashing_psi_amd")
    exe = str(tmp_path / "query_slices_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "query_slices_check.cpp"),
                           "-L" + libdir, "-lpiehip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    assert "query slices check ok: 4 handles, 2 queries per run, 5 result ciphertexts each" in out.stdout
