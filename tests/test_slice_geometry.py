"""The copy geometry of the slice-input setters (csrc/slice_geometry.h) without a GPU: tests/slice_geometry_check.cpp performs the
planned copies with memcpy for every unit range of three small shapes, both pieces, both source layouts, seeded and not, and compares
with the definition of a slice.  Built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer (their runtimes
linked into the program) and run as a plain executable: a row outside the source or the owned copy, or a sanitizer report, is a
non-zero exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_copies_cut_the_slice_by_its_definition(tmp_path):
    exe = str(tmp_path / "slice_geometry_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "slice_geometry_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "slice geometry ok" in r.stdout
