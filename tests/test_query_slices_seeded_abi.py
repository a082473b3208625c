"""Seeded query slices without a GPU: the four setters are declared in include/piehip.h, exported by libpiehip.so and prototyped in
_lib.py; they refuse a null handle before anything else, and the C++ facade's seeded calls compile warning-free against the header."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["piehip_set_index_slice_seeded_q", "piehip_set_minus_slice_seeded_q", "piehip_set_index_slice_seeded_from_q",
         "piehip_set_minus_slice_seeded_from_q"]


def test_the_four_setters_are_declared_exported_and_prototyped():
    from nested_hashing_psi_amd import build
    path = build()
    from nested_hashing_psi_amd._lib import SYMBOLS, lib, u8p, u64p
    hdr = open(os.path.join(ROOT, "include", "piehip.h")).read()
    raw = C.CDLL(path if isinstance(path, str) and path.endswith(".so") else os.path.join(ROOT, "nested_hashing_psi_amd", "libpiehip.so"))
    L = lib()
    assert L.piehip_version() == 102    # new symbols, no new number
    for n in NAMES:
        assert ("int " + n + "(piehip_handle h, uint32_t q, const uint64_t *") in hdr, n
        assert hasattr(raw, n), n
        assert SYMBOLS[n] == (C.c_int, [C.c_void_p, C.c_uint32, u64p, u8p]), n
        assert getattr(L, n)(None, 0, None, None) == -1 and L.piehip_last_error()


def test_cpp_facade_seeded_calls_compile(tmp_path):
    src = tmp_path / "seeded_slices_facade.cpp"
    src.write_text('''#include "nested_hashing_psi_amd/host/QuerySlicedBatchedFHEHIPPIE.hpp"
size_t f(piehip::QuerySlicedBatchedFHEHIPPIE &op, const uint64_t *c0, const uint8_t *s)
{
    op.setIndexSeeded(c0, s);
    op.setIndexSeeded(1, c0, s);
    op.setMinusCompareElementSeeded(c0, s);
    op.setMinusCompareElementSeeded(1, c0, s);
    return op.uploadedBytes(0);
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + ROOT, str(src)])
