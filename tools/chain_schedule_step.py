"""run() with a chain schedule against the uniform settings, K = 3, in one process:
    python tools/chain_schedule_step.py [--config C3K3|C5] [--lib PATH] [--out FILE] [--profile]

One handle, a batch of three queries per run(), inputs resident in HBM, results left in HBM.  Legs, each a schedule
(piehip_set_chain_schedule; product 1 on the first entry's limbs, product 2 and the mask multiply on the second's):
  C3K3   C3's ring with three inner hash functions (N = 16384, L = 4, E = 14, b = 14):   default (4,4) | (4,3)
  C5     N = 32768, L = 6, K = 3, E = 30, b = 30:                                        (6,6) | (4,4) | (4,3)
A block is `--runs` run()s back to back and one sync; the blocks ALTERNATE between the legs, so that a drift of the box shows in
every leg alike; the first `--warmup` blocks of every leg are not counted.  Reported per leg: median [min, max] of the counted
blocks, in microseconds per step (one run() of three queries).  The tool measures and gates nothing; its verdicts compare medians
against the spread (max - min) of the leg compared with.
--lib PATH: another build of the library in this process instead -- the parent commit's, which has no schedule: only the default
leg runs.  One handle per process: a second handle's streams would share the runtime's four hardware queues with the first
(profiles/chain_limbs/README.txt), so the parent's library is timed by a second call in the same session, not beside this tree's.
--profile: per-class launch times of every leg on one queue, from the library's own event brackets, after the timed legs.
Python's cyclic GC is off inside the legs.  Query contents are synthetic (uniform residues).  Prints one JSON line.
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T32 = 4296540161
CONFIGS = {
    "C3K3": (dict(N=16384, L=4, t=T32, k=2, e=4949, K=3, E=14, b=14), [(4, 4), (4, 3)]),
    "C5": (dict(N=32768, L=6, t=T32, k=2, e=13004, K=3, E=30, b=30), [(6, 6), (4, 4), (4, 3)]),
}


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "blocks": len(s)}


def leg_name(sched):
    return "(%s)" % ",".join(str(v) for v in sched)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3K3", choices=sorted(CONFIGS))
    ap.add_argument("--blocks", type=int, default=17, help="counted blocks per leg")
    ap.add_argument("--warmup", type=int, default=3, help="uncounted blocks per leg")
    ap.add_argument("--runs", type=int, default=20, help="run()s per block")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--lib", default=None, help="time another build of the library (the parent commit's: the default leg alone)")
    ap.add_argument("--profile", action="store_true", help="per-class launch times of every leg, one queue")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from nested_hashing_psi_amd import _lib, pie
    has_setting = True
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        has_setting = hasattr(C.CDLL(_lib.LIB_PATH), "piehip_set_chain_schedule")
        if not has_setting:
            for s_ in ("piehip_set_chain_schedule", "piehip_get_chain_schedule"):
                _lib.SYMBOLS.pop(s_, None)
    cfg, scheds = CONFIGS[args.config]
    N, L, t, K, E, b = (cfg[v] for v in ("N", "L", "t", "K", "E", "b"))
    B, nq = cfg["k"] * cfg["e"], args.batch
    if not has_setting:
        scheds = scheds[:1]
    rng = np.random.default_rng(2026)
    cc = pie.PieContext(N, L, t)
    q = cc.q

    def limbs(*shape):
        out = np.empty(shape + (L, N), dtype=np.uint64)
        for i in range(L):
            out[..., i, :] = rng.integers(0, int(q[i]), shape + (N,), dtype=np.uint64)
        return out
    slots = rng.integers(0, t, (K, b, E, B), dtype=np.int64)
    slots[slots > t // 2] -= t
    mask_slots = rng.integers(1, t, (b, B), dtype=np.int64)
    mask_slots[mask_slots > t // 2] -= t
    cc.load_relin_key(limbs(L, 2))
    op = pie.BatchedFHEHIPPIE(cc, slots=slots, mask_slots=mask_slots)
    op.setQueryBatch(nq)
    idx_h, minus_h = limbs(K, E, 2), limbs(2)
    dev = []
    for i in range(nq):
        di, dm = torch.from_numpy(idx_h.view(np.int64)).cuda(), torch.from_numpy(minus_h.view(np.int64)).cuda()
        dev.append((di, dm))
        op.setIndexDevice(di.data_ptr(), query=i)
        op.setMinusCompareElementDevice(dm.data_ptr(), query=i)
    torch.cuda.synchronize()

    def prepare(sched):
        if has_setting:
            op.setChainSchedule(sched)

    us = {leg_name(s): [] for s in scheds}
    gc.collect()
    for blk in range(args.warmup + args.blocks):
        for sched in scheds:
            prepare(sched)
            op.run()
            gc.disable()
            t0 = time.perf_counter()
            for _ in range(args.runs):
                op.run(sync=False)
            op.sync()
            dt = time.perf_counter() - t0
            gc.enable()
            if blk >= args.warmup:
                us[leg_name(sched)].append(dt * 1e6 / args.runs)
    step = {name: stats(v) for name, v in us.items()}
    ref = leg_name(scheds[0])
    verdict = {}
    for sched in scheds[1:]:
        a = leg_name(sched)
        d, spread = step[a]["median"] - step[ref]["median"], step[ref]["max"] - step[ref]["min"]
        verdict["%s_vs_%s" % (a, ref)] = "%s is %.1f us %s than %s (%s's spread: %.1f us)" % (a, abs(d), "shorter" if d < 0 else "longer", ref, ref, spread)
    out = {"config": args.config, "shape": cfg, "queries_per_run": nq, "runs_per_block": args.runs, "step_us": step, "verdict": verdict,
           "library": args.lib or "this tree's", "device": torch.cuda.get_device_name(0),
           "block_order": "legs alternate; the first %d blocks of every leg are not counted" % args.warmup}
    if args.profile:
        out["per_class_us"] = {}
        for sched in scheds:
            prepare(sched)
            cc.set_run_streams(1)   # one queue: the brackets of two queues overlap
            cc.set_profiling(True)
            acc = {}
            for _ in range(9):
                op.run()
                for kname, rec in cc.profile().items():
                    acc.setdefault(kname, []).append(rec["ms"] * 1e3)
            cc.set_profiling(False)
            cc.set_run_streams(0)
            out["per_class_us"][leg_name(sched)] = {kname: sorted(v)[len(v) // 2] for kname, v in acc.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    cc.close()


if __name__ == "__main__":
    main()
