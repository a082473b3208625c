"""tests/result_limbs_check.cpp, built and run the way tests/facade_check.cpp is: the C++ facade's setResultLimbs (single-query
operator and query batch) against digests computed here from the oracle and the exact definition, and BatchedFHEPSIServer's result
messages framed with `keep` limbs."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_result_limbs import mod_reduce_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fnv(cts):
    h = 0xCBF29CE484222325
    for w in np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1).tolist():
        h = ((h ^ w) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_facade_and_server_with_result_limbs(ob, tmp_path):
    libdir = os.path.join(ROOT, "nested_hashing_psi_amd")
    exe = str(tmp_path / "result_limbs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "result_limbs_check.cpp"),
                           "-L" + libdir, "-lpiehip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    keep, N, L, t = 1, 1024, 2, 65537
    k, e, K, b, E = 2, 2, 2, 2, 3
    out = subprocess.run([exe, str(keep)], stdout=subprocess.PIPE, timeout=300, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    m = re.search(r"facade full ([0-9a-f]{16}) keep ([0-9a-f]{16}) batch1 ([0-9a-f]{16})", out.stdout)
    assert m and "server ok: %d result messages of %d limb(s)" % (2, keep) in out.stdout
    # the same queries on the oracle: facade_check.cpp's table, seeds 6 / 7, result_limbs_check.cpp's towers
    o = ob.Oracle(N, L, t)
    tbl = ((np.arange(k * e * K * b * E, dtype=np.uint64) * np.uint64(7919)) % np.uint64(65536) + np.uint64(1)).reshape(k, e, K, b, E)
    ob.hct_shuffle_bins(tbl, 6)
    slots = ob.pack_db(tbl)
    db = np.stack([o.encode_eval(slots[h, bn, j]) for h in range(K) for bn in range(b) for j in range(E)]).reshape(K, b, E, L, N)
    mk = ob.masks(t, b, k * e, 7)
    masks = np.stack([o.encode_eval(mk[bn]) for bn in range(b)])

    def towers(shape, seed):     # result_limbs_check.cpp's towers()
        w = np.arange(1, int(np.prod(shape)) + 1, dtype=np.uint64)
        return ((w * np.uint64(2654435761) + np.uint64(seed * 40503)) % np.uint64(65521)).reshape(shape)
    evk = towers((L, 2, L, N), 1)

    def query(base, minus):
        idx = np.zeros((K, E, 2, L, N), dtype=np.uint64)
        for h in range(K):
            for j in range(E):
                idx[h, j] = towers((2, L, N), base + h + 2 * j)
        return o.pie_run(idx, towers((2, L, N), minus), db, masks, evk)
    full0, full1 = query(5, 3), query(12, 4)
    assert not (full0 == full1).all() and len(np.unique(mod_reduce_exact(o, full0, keep))) > N
    assert int(m.group(1), 16) == _fnv(full0)
    assert int(m.group(2), 16) == _fnv(mod_reduce_exact(o, full0, keep))
    assert int(m.group(3), 16) == _fnv(mod_reduce_exact(o, full1, keep))
