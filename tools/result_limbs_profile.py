"""A C3 batch of three with reduced result lists, for a kernel trace: python tools/result_limbs_profile.py --keep 1 [--steps 50]

    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/result_limbs_profile.py --keep 1

Synthetic contents (uniform residues), one queue per run() so that the launches do not overlap in the trace.  Also prints the
library's own per-class times of one profiled run() (piehip_set_profiling): result_ntt_inv, limb_drop and result_ntt_fwd are the
reduction's three launches.  keep = 4 runs the plain step.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    from nested_hashing_psi_amd import pie
    N, L, t, K, E, b, nq = 16384, 4, 4296540161, 2, 14, 14, 3   # C3's shape
    rng = np.random.default_rng(7)
    cc = pie.PieContext(N, L, t)

    def limbs(*shape):
        out = np.empty(shape + (L, N), dtype=np.uint64)
        for i in range(L):
            out[..., i, :] = rng.integers(0, int(cc.q[i]), shape + (N,), dtype=np.uint64)
        return out
    cc.load_relin_key(limbs(L, 2))
    cc.set_run_streams(1)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=limbs(K, b, E), preCalcRandomMask=limbs(b))
    op.setQueryBatch(nq)
    for q in range(nq):
        op.setMinusCompareElement(limbs(2), query=q)
        op.setIndex(limbs(K, E, 2), query=q)
    op.setResultLimbs(args.keep)
    for _ in range(args.steps):
        op.run(sync=False)
    op.sync()
    cc.set_profiling(True)
    op.run()
    prof = cc.profile()
    cc.set_profiling(False)
    print(json.dumps({"keep": args.keep, "steps": args.steps, "profiled_run_ms": {k: round(v["ms"], 4) for k, v in prof.items()},
                      "launches": {k: v["launches"] for k, v in prof.items()}}))
    cc.close()


if __name__ == "__main__":
    main()
