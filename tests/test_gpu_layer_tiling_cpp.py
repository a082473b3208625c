"""tests/layer_tiling_check.cpp, built and run the way tests/chain_limbs_check.cpp is: the C++ facade with layerTiling (list length b',
bits equal to the vectors written here) and the server driver with setLayerTiling (b' result messages, their bits).  The vectors are
those of tests/test_gpu_layer_tiling.py: C1's packing tiled by 3 for the facade and by 7, piehip_layer_tiling's choice, for the server."""
import os
import subprocess

import pytest

from tests.test_gpu_layer_tiling import C1, _reference, _shape, drop_references

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_and_server_with_layer_tiling(ob, tmp_path):
    libdir = os.path.join(ROOT, "nested_hashing_psi_amd")
    exe = str(tmp_path / "layer_tiling_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "layer_tiling_check.cpp"),
                           "-L" + libdir, "-lpiehip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    N, L, t, k, e, K, b, E, nS = C1
    assert (N, L, t, k, e, K, b, E, nS) == (4096, 2, 65537, 3, 110, 2, 7, 3, 1500)     # the program's constants
    d = _shape(ob, C1)
    idx, minus, want = _reference(ob, C1, 3)
    idx7, minus7, want7 = _reference(ob, C1, 7)
    assert want.shape == (3, 2, L, N) and want7.shape == (1, 2, L, N)
    for name, a in (("table", d["tbl0"]), ("server", d["server"]), ("evk", d["evk"]), ("minus", minus), ("idx", idx), ("want", want),
                    ("minus7", minus7), ("idx7", idx7), ("want7", want7)):
        a.tofile(str(tmp_path / (name + ".bin")))
    drop_references()
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, timeout=300, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    assert "facade ok: 3 result ciphertexts for 7 bin layers tiled by 3" in out.stdout
    assert "server ok: 1 result message(s) for 7 bin layers" in out.stdout
