"""C3 run() with and without the last relinearisation, in one process: python tools/result_relin_step.py [--out FILE] [--lib PATH]

Step legs: one handle, C3's shape, a batch of three queries per run(), inputs resident in HBM, results left in HBM.  Legs
  on_full   piehip_set_result_relin(1), keep = L   (the default path: what the parent commit runs)
  off_full  piehip_set_result_relin(0), keep = L   (rows of three components)
  on_keep1 / off_keep1   the same with piehip_set_result_limbs(1)
A block is `--runs` run()s back to back and one sync; the blocks ALTERNATE between the legs, so that a drift of the box shows in
every leg alike; the first `--warmup` blocks of every leg are not counted.  Reported per leg: median, minimum and maximum of the
counted blocks, in microseconds per step (one run() of three queries).  An off leg is called faster than its on leg only if its
median is lower by more than the on leg's own spread (max - min).
Stream legs (--stream): tools/result_limbs_stream.py's host-memory query stream over three query slots with keep = 1, relin on and
off -- where the third component costs link time.
--lib PATH: time another build of the library (the parent commit's, for the default path: it has no setting, so only the on legs
run; or a -DPIEHIP_RESULT_EVAL_Q=0 build, for the fallback schedule on a fused ring).
Python's cyclic GC is off inside the legs.  Query contents are synthetic (uniform residues).  Prints one JSON line.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("piehip_set_result_relin", "piehip_get_result_relin", "piehip_get_result_components", "piehip_client_decrypt_deg2")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "blocks": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=17, help="counted blocks per leg")
    ap.add_argument("--warmup", type=int, default=3, help="uncounted blocks per leg")
    ap.add_argument("--runs", type=int, default=20, help="run()s per block")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--stream", action="store_true", help="also the host-memory stream legs")
    ap.add_argument("--lib", default=None, help="another libpiehip.so to time")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from nested_hashing_psi_amd import _lib
    has_setting = True
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        import ctypes
        import torch  # noqa: F401  (one HIP runtime per process: see _lib.lib)
        probe = ctypes.CDLL(_lib.LIB_PATH)
        has_setting = hasattr(probe, NEW_SYMBOLS[0])
        if not has_setting:
            for s in NEW_SYMBOLS:
                _lib.SYMBOLS.pop(s, None)
            _lib.NKERNELS = 17
    import torch
    from nested_hashing_psi_amd import pie
    N, L, t, k, e, K, E, b = 16384, 4, 4296540161, 2, 4949, 2, 14, 14   # C3 (bench.CONFIGS["C3"])
    B, nq = k * e, args.batch
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
        dev += [di, dm]
        op.setIndexDevice(di.data_ptr(), query=i)
        op.setMinusCompareElementDevice(dm.data_ptr(), query=i)
    torch.cuda.synchronize()
    legs = [("on_full", True, L), ("off_full", False, L), ("on_keep1", True, 1), ("off_keep1", False, 1)]
    if not has_setting:
        legs = [l for l in legs if l[1]]

    def setting(o, relin, keep):
        if has_setting:
            o.setResultRelin(relin)
        o.setResultLimbs(keep)

    us = {name: [] for name, _, _ in legs}
    gc.collect()
    for blk in range(args.warmup + args.blocks):
        for name, relin, keep in legs:
            setting(op, relin, keep)
            op.run()
            gc.disable()
            t0 = time.perf_counter()
            for _ in range(args.runs):
                op.run(sync=False)
            op.sync()
            dt = time.perf_counter() - t0
            gc.enable()
            if blk >= args.warmup:
                us[name].append(dt * 1e6 / args.runs)
    step = {name: stats(v) for name, v in us.items()}
    verdict = {}
    for keep in ("full", "keep1"):
        on, off = step.get("on_" + keep), step.get("off_" + keep)
        if on and off:
            spread = on["max"] - on["min"]
            verdict[keep] = ("off faster than on by more than the on leg's spread" if on["median"] - off["median"] > spread
                             else "off slower than on by more than the on leg's spread" if off["median"] - on["median"] > spread
                             else "within the on leg's spread")
    out = {"config": "C3", "queries_per_run": nq, "library": args.lib or "this tree's", "runs_per_block": args.runs,
           "step_us": step, "verdict": verdict, "device": torch.cuda.get_device_name(0),
           "block_order": "legs alternate; the first %d blocks of every leg are not counted" % args.warmup}
    if args.stream:
        out["stream"] = stream_legs(args, pie, torch, cc, op, limbs, has_setting, N, L, t, K, E, b, nq)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    cc.close()


def stream_legs(args, pie, torch, cc, op, limbs, has_setting, N, L, t, K, E, b, nq, nsl=3, batches=24, passes=3):
    """the host-memory stream of tools/result_limbs_stream.py with keep = 1: relinearisation on and off, passes alternating"""
    streams = [torch.cuda.Stream() for _ in range(nsl - 1)]
    ops = [op] + [pie.BatchedFHEHIPPIE(pie.PieContext(N, L, t, stream=s.cuda_stream), attachTo=op) for s in streams]
    for o in ops:
        o.setQueryBatch(nq)
        o.cc.set_run_streams(1)
    idx_h, minus_h = limbs(K, E, 2), limbs(2)
    legs = [("on_keep1", True), ("off_keep1", False)] if has_setting else [("on_keep1", True)]

    def prepare(relin):
        bufs = []
        for o in ops:
            if has_setting:
                o.setResultRelin(relin)
            o.setResultLimbs(1)
            qb = []
            for q_ in range(nq):
                bi, bm, br = o.hostBuffers(query=q_)
                bi[...] = idx_h
                bm[...] = minus_h
                qb.append((bi, bm, br))
            bufs.append(qb)
        return bufs

    def one_pass(bufs):
        nb = max(batches // nsl, 2) * nsl
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(nb + nsl):
            o, qb = ops[i % nsl], bufs[i % nsl]
            if i >= nsl:
                o.waitHost()
            if i < nb:
                for q_ in range(nq):
                    o.stageMinus(qb[q_][1], query=q_)
                for h in range(K):
                    for q_ in range(nq):
                        o.stageIndexRow(h, qb[q_][0][h], query=q_)
                o.runStaged(qb[0][2])
        return (time.perf_counter() - t0) * 1e3 / (nb * nq)

    ms = {name: [] for name, _ in legs}
    for rnd in range(passes + 1):
        for name, relin in legs:
            bufs = prepare(relin)
            gc.disable()
            p = one_pass(bufs)
            gc.enable()
            if rnd:
                ms[name].append(p)
    res = {"ms_per_query_passes": ms, "best_ms_per_query": {n: min(v) for n, v in ms.items()},
           "result_mib_down_per_query": {"on_keep1": b * 2 * N * 8 / 2**20, "off_keep1": b * 3 * N * 8 / 2**20}, "slots": nsl}
    for o in ops[1:]:
        o.cc.close()
    return res


if __name__ == "__main__":
    main()
