"""A C3-shaped query-sliced step with seeded inputs on G handles of ONE device, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -o seeded_slices -- python tools/seeded_slices_profile.py [--rounds R] [--handles G]
Every round sets a batch of three seeded queries on every handle and runs the sliced operator: one expand_uniform_limb_kernel launch
per handle and round, nq (E + 1) u_n jobs of ceil(N / 10) Keccak permutations each.  Beside it, in the same process, R calls of
piehip_expand_uniform_device with as many seeds as give about the same number of permutations per launch (seeds x L limbs), so that
the trace holds both kernels' time per permutation.  Random residues stand for the database and the c0 halves: the kernels do not care.
Handles on one device serialise: the trace says what the launches cost, not what G devices would do."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--handles", type=int, default=8)
    a = ap.parse_args()
    import torch
    from nested_hashing_psi_amd import pie
    N, L, t, K, E, b, nq, G = 16384, 4, 4296540161, 2, 14, 14, 3, a.handles
    ccs = [pie.PieContext(N, L, t) for _ in range(G)]
    q = ccs[0].q
    rng = np.random.default_rng(1)

    def limbs(*prefix):
        out = np.empty(prefix + (L, N), dtype=np.uint64)
        for i, m in enumerate(q):
            out[..., i, :] = rng.integers(0, int(m), prefix + (N,), dtype=np.uint64)
        return out

    op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=limbs(K, b, E), preCalcRandomMask=limbs(b))
    op.setQueryBatch(nq)
    evk = limbs(L, 2)
    for cc in ccs:
        cc.load_relin_key(evk)
    chunks = (N + 9) // 10
    un = [hi - lo for lo, hi in op.unitSlices]
    for r in range(a.rounds):
        for i in range(nq):
            op.setIndexSeeded(limbs(K, E), rng.integers(0, 256, (K, E, 32), dtype=np.uint8), query=i)
            op.setMinusCompareElementSeeded(limbs(), rng.integers(0, 256, 32, dtype=np.uint8), query=i)
        op.run()
    per_launch = max(un) * nq * (E + 1) * chunks
    nseeds = max(1, round(per_launch / (L * chunks)))
    d = torch.zeros((nseeds, L, N), dtype=torch.int64, device="cuda")
    for r in range(a.rounds):
        ccs[0].expand_uniform_device(rng.integers(0, 256, (nseeds, 32), dtype=np.uint8), d.data_ptr())
    torch.cuda.synchronize()
    print("expand_uniform_limb_kernel: %d launches, permutations per launch by handle: %s" % (a.rounds * sum(1 for n in un if n),
          [n * nq * (E + 1) * chunks for n in un]))
    print("expand_uniform_kernel: %d launches of %d seeds x %d limbs = %d permutations" % (a.rounds, nseeds, L, nseeds * L * chunks))
    for cc in ccs:
        cc.close()


if __name__ == "__main__":
    main()
