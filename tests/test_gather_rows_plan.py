"""The plan of piehip_gather_results for result rows of any shape (csrc/exchange_plan.h: ExchangeShape's ncomp and row_limbs), without
a GPU: tests/gather_rows_plan_check.cpp carries the plan out with memcpy for rows of (components, limbs) in {(2, L), (2, 1), (3, L),
(3, 2)}, G = 1..5, every root, b in {1, 4, 5, 14} and nq in {1, 3} -- every word of the root's list written exactly once, by the rank
that owns its layer, both ends of a transfer naming one word count -- and compares the default-initialised shape's plan with the plan
as it was before rows had a shape.  Built twice with the host compiler -- plain, and under AddressSanitizer +
UndefinedBehaviorSanitizer with their runtimes linked into the program -- and run as plain executables.  Ranks that plan with
different row shapes must fail the same check, so the check can fail."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gather_rows_plan_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gather_rows_plan") / ("gather_rows_plan_check_" + request.param))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + (SAN if request.param == "sanitized" else []) + ["-o", out, SRC])
    return out


def test_every_word_once_from_its_owner_and_the_default_plan_stays(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gather rows plan ok: %d cases" % (4 * 2 * 15 * 4) in r.stdout


def test_ranks_with_different_row_shapes_fail_the_check(exe):
    r = subprocess.run([exe, "wrong"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "are caught" in r.stdout and "words" in r.stdout
