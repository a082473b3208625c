"""tests/chain_schedule_check.cpp, built and run the way tests/chain_limbs_check.cpp is: the C++ facade's setChainSchedule (single-query
operator, a slot set through the C ABI, a query batch of two with its own schedule) against the vectors computed here from the oracle
and the exact definition, which the program reads from a temporary directory."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_chain_schedule import run_chain_schedule_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_with_a_chain_schedule(ob, tmp_path):
    libdir = os.path.join(ROOT, "nested_hashing_psi_amd")
    exe = str(tmp_path / "chain_schedule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "chain_schedule_check.cpp"),
                           "-L" + libdir, "-lpiehip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    N, L, t, sched = 4096, 3, 65537, (3, 2)
    k, e, K, b, E = 2, 2, 3, 2, 2
    # the program's queries on the oracle: its table, seeds 6 / 7, its towers
    o = ob.Oracle(N, L, t)
    tbl = ((np.arange(k * e * K * b * E, dtype=np.uint64) * np.uint64(7919)) % np.uint64(65536) + np.uint64(1)).reshape(k, e, K, b, E)
    ob.hct_shuffle_bins(tbl, 6)
    slots = ob.pack_db(tbl)
    db = np.stack([o.encode_eval(slots[h, bn, j]) for h in range(K) for bn in range(b) for j in range(E)]).reshape(K, b, E, L, N)
    mk = ob.masks(t, b, k * e, 7)
    masks = np.stack([o.encode_eval(mk[bn]) for bn in range(b)])

    def towers(shape, seed):     # chain_schedule_check.cpp's towers()
        w = np.arange(1, int(np.prod(shape)) + 1, dtype=np.uint64)
        return ((w * np.uint64(2654435761) + np.uint64(seed * 40503)) % np.uint64(65521)).reshape(shape)
    evk = towers((L, 2, L, N), 21)

    def query(base, minus):
        idx = np.zeros((K, E, 2, L, N), dtype=np.uint64)
        for h in range(K):
            for j in range(E):
                idx[h, j] = towers((2, L, N), base + h + K * j)
        return run_chain_schedule_exact(ob, o, idx, towers((2, L, N), minus), db, masks, evk, sched)
    want = np.stack([query(5, 3), query(12, 4)])
    assert want.shape == (2, b, 2, 2, N) and not (want[0] == want[1]).all() and len(np.unique(want[0])) > N
    want.reshape(-1).tofile(str(tmp_path / "want.bin"))
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, timeout=300, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    assert "facade ok: %d + %d + 2 x %d result ciphertexts from the schedule (3,2) on %d limbs" % (b, b, b, L) in out.stdout
