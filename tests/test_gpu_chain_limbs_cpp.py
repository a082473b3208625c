"""tests/chain_limbs_check.cpp, built and run the way tests/result_relin_check.cpp is: the C++ facade's setChainLimbs (single-query
operator, then keep = 1 below the level, then a query batch of two with its own setting) against the vectors computed here from the
oracle and the exact definition, which the program reads from a temporary directory."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_chain_limbs import level_oracle, run_chain_limbs_exact
from tests.test_result_limbs import mod_reduce_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_with_the_chain_on_fewer_limbs(ob, tmp_path):
    libdir = os.path.join(ROOT, "nested_hashing_psi_amd")
    exe = str(tmp_path / "chain_limbs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "chain_limbs_check.cpp"),
                           "-L" + libdir, "-lpiehip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    N, L, Lc, t = 4096, 3, 2, 65537
    k, e, K, b, E = 2, 2, 2, 2, 3
    # the program's queries on the oracle: facade_check.cpp's table, seeds 6 / 7, chain_limbs_check.cpp's towers
    o = ob.Oracle(N, L, t)
    tbl = ((np.arange(k * e * K * b * E, dtype=np.uint64) * np.uint64(7919)) % np.uint64(65536) + np.uint64(1)).reshape(k, e, K, b, E)
    ob.hct_shuffle_bins(tbl, 6)
    slots = ob.pack_db(tbl)
    db = np.stack([o.encode_eval(slots[h, bn, j]) for h in range(K) for bn in range(b) for j in range(E)]).reshape(K, b, E, L, N)
    mk = ob.masks(t, b, k * e, 7)
    masks = np.stack([o.encode_eval(mk[bn]) for bn in range(b)])

    def towers(shape, seed):     # chain_limbs_check.cpp's towers()
        w = np.arange(1, int(np.prod(shape)) + 1, dtype=np.uint64)
        return ((w * np.uint64(2654435761) + np.uint64(seed * 40503)) % np.uint64(65521)).reshape(shape)
    evk = towers((L, 2, L, N), 21)

    def query(base, minus):
        idx = np.zeros((K, E, 2, L, N), dtype=np.uint64)
        for h in range(K):
            for j in range(E):
                idx[h, j] = towers((2, L, N), base + h + 2 * j)
        return run_chain_limbs_exact(ob, o, idx, towers((2, L, N), minus), db, masks, evk, Lc)
    want = np.stack([query(5, 3), query(12, 4)])
    assert want.shape == (2, b, 2, Lc, N) and not (want[0] == want[1]).all() and len(np.unique(want[0])) > N
    one = mod_reduce_exact(level_oracle(ob, o, Lc), want[0], 1)
    assert one.shape == (b, 2, 1, N)
    np.concatenate([want.reshape(-1), one.reshape(-1)]).tofile(str(tmp_path / "want.bin"))
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, timeout=300, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    assert "facade ok: %d + %d + 2 x %d result ciphertexts from a chain on %d of %d limbs" % (b, b, b, Lc, L) in out.stdout
