"""The plan of piehip_rccl_scatter_query, piehip_rccl_exchange_accumulators and piehip_gather_results (csrc/exchange_plan.h) without a
GPU: tests/exchange_plan_check.cpp matches every send with its receive, runs every rank's list in its posting order over channels
without any buffering -- each collective alone, and the gather as the third step behind the scatter and the exchange -- and carries the
plan out with memcpy, for G = 1..9, every root and five shapes that include G > K L and G > b (ranks without bin layers post nothing in
the gather; every word of the root's [b][nq][2][L][N] is written exactly once, its own rows by the device copy's stand-in).  Built twice with
the host compiler -- plain, and under AddressSanitizer + UndefinedBehaviorSanitizer with their runtimes linked into the program --
and run as plain executables.  The ranges it prints are compared with piehip_query_slice and piehip_rccl_bin_slice of the built
library; and posting all sends first must deadlock in the same simulation, so the simulation can fail."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "exchange_plan_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("exchange_plan") / ("exchange_plan_check_" + request.param))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + (SAN if request.param == "sanitized" else []) + ["-o", out, SRC])
    return out


def test_plan_matches_completes_and_places_every_word_once(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "exchange plan ok" in r.stdout
    from nested_hashing_psi_amd import _lib
    lib = _lib.lib()
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("range ")]
    assert len(rows) == 5 * sum(range(1, 10))
    for G, K, L, b, rank, u_lo, u_hi, b_lo, b_hi in rows:
        lo, hi = C.c_uint32(), C.c_uint32()
        assert lib.piehip_query_slice(K, L, G, rank, C.byref(lo), C.byref(hi)) == 0
        assert (lo.value, hi.value) == (u_lo, u_hi), (G, K, L, rank)
        assert lib.piehip_rccl_bin_slice(b, G, rank, C.byref(lo), C.byref(hi)) == 0
        assert (lo.value, hi.value) == (b_lo, b_hi), (G, b, rank)


def test_all_sends_first_deadlocks_in_the_simulation(exe):
    r = subprocess.run([exe, "naive"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "naive order deadlocks" in r.stdout
