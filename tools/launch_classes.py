"""launch count and algorithmic bytes per profile class (piehip_profile_read_n) of ONE run() per shape, for comparing two checkouts:
python tools/launch_classes.py [root of the checkout whose library is measured; default: this one].  Times are left out: the table of
two checkouts that enqueue the same launches is the same text."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..")))
from nested_hashing_psi_amd import pie  # noqa: E402


def table(N, L, K, E, b, nq, queues, keep, host):
    cc = pie.PieContext(N, L, 65537 if N <= 4096 else 4296540161)
    rng = np.random.default_rng(1)
    rand = lambda *shape: np.stack([rng.integers(0, int(m), shape + (N,), dtype=np.uint64) for m in cc.q], axis=-2)
    cc.load_relin_key(rand(L, 2))
    cc.set_run_streams(queues)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=rand(K, b, E), preCalcRandomMask=rand(b))
    op.setQueryBatch(nq)
    op.setResultLimbs(keep)
    idx, minus = rand(nq, K, E, 2), rand(nq, 2)
    for q in range(nq):
        op.setMinusCompareElement(minus[q], query=q)
        op.setIndex(idx[q], query=q)
    cc.set_profiling(True)
    if host:
        op.runHost(idx if nq > 1 else idx[0], minus if nq > 1 else minus[0])
    else:
        op.run()
    print("N=%d L=%d K=%d E=%d b=%d nq=%d queues=%d result_limbs=%d results=%s" % (N, L, K, E, b, nq, queues, keep, "host" if host else "device"))
    for name, p in cc.profile().items():
        print("    %-16s launches %3d  alg_bytes %.0f" % (name, p["launches"], p["alg_bytes"]))
    cc.close()


for K in (1, 3):
    for nq in (1, 3):
        for queues in (1, 2):
            for keep in (2, 1):
                for host in (False, True):
                    table(4096, 2, K, 2, 3, nq, queues, keep, host)
table(16384, 4, 2, 14, 14, 3, 0, 4, False)   # the benchmark's default shape: C3, a batch of three, two queues
table(16384, 4, 2, 14, 14, 3, 0, 4, True)
