"""C2 run() on an untiled database (b = 12 bin layers) and on the same database tiled by R = 6 (b' = 2), in one process:
    python tools/layer_tiling_step.py [--batches 3,8] [--out FILE]

C2 at its full size (bench.CONFIGS["C2"]: N = 8192, L = 3, t = 4296540161, |S| = 2^16, k = 3, e = 443, K = 2, E = 12, b = 12): k e = 1329
of 8192 slots, so piehip_layer_tiling packs six bin layers into every plaintext.  Two handles, each built from the server set by
piehip_build_db (the tiled one under piehip_set_layer_tiling): same seeds, so the same table, shuffle and masks.  The queries are real
ones from the device client (layerTiling on the tiled leg), resident in HBM; results are left in HBM.
A block is `--runs` run()s back to back and one sync; the blocks ALTERNATE between the two legs, so that a drift of the box shows in
both alike; the first `--warmup` blocks of every leg are not counted.  Per leg and batch size: median [min, max] of the counted blocks
in microseconds per step and per query, database bytes, result bytes per query, the offline phase (piehip_build_db, median of
`--offline` builds after one uncounted), and the noise budgets of the results (piehip_client_decrypt_budget, min over a query's rows).
The tool measures and gates nothing; its verdict compares medians against the spread (max - min) of the untiled leg.
Python's cyclic GC is off inside the legs.  Prints one JSON line.
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


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "blocks": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=17, help="counted blocks per leg")
    ap.add_argument("--warmup", type=int, default=3, help="uncounted blocks per leg")
    ap.add_argument("--runs", type=int, default=20, help="run()s per block")
    ap.add_argument("--batches", default="3,8", help="queries per run(), one measurement each")
    ap.add_argument("--offline", type=int, default=5, help="counted builds of the database per leg")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from nested_hashing_psi_amd import pie
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    N, L, t, k, e, K, E, b, nS, nC = 8192, 3, 4296540161, 3, 443, 2, 12, 12, 1 << 16, 1 << 10   # C2
    R, bt = pie.layer_tiling(N, k, e, b)
    rng = np.random.default_rng(2026)
    items = np.unique(rng.integers(1, t, nS + nC + 4096, dtype=np.uint64))
    rng.shuffle(items)
    server = items[:nS].copy()
    clientset = np.concatenate([server[:nC // 2 + 1], items[nS:nS + nC // 2 - 1]])
    hp = dict(k=k, e=e, K=K, b=b, E=E, hash_seed=987654321, evict_seed=1, shuffle_seed=2, mask_seed=3)
    legs = {}
    for name, r in (("untiled", 1), ("tiled", R)):
        cc = pie.PieContext(N, L, t)
        cl = BatchedFHEPSIClient(cc, k, e, K, E, b, layerTiling=r)
        cc.load_relin_key(cl.runSetUpPhase())
        cc.setLayerTiling(r)
        cc.reserve(nS, k, e, K, b, E)
        builds = []
        for _ in range(1 + args.offline):
            t0 = time.perf_counter()
            op = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=hp, layerTiling=r)
            op.sync()
            builds.append((time.perf_counter() - t0) * 1e3)
        layers = op.b
        legs[name] = dict(cc=cc, cl=cl, op=op, R=r, layers=layers, offline_ms=stats(builds[1:]),
                          database_bytes=(K * layers * E + layers) * L * N * 8, result_bytes_per_query=layers * 2 * L * N * 8)
    out = {"config": "C2", "R": R, "bin_layers": b, "tiled_layers": bt, "runs_per_block": args.runs, "batches": {},
           "device": torch.cuda.get_device_name(0),
           "block_order": "legs alternate; the first %d blocks of every leg are not counted" % args.warmup}
    for nq in [int(v) for v in args.batches.split(",")]:
        keep = []
        for leg in legs.values():
            op, cl = leg["op"], leg["cl"]
            op.setQueryBatch(nq)
            for q in range(nq):     # one client set, fresh encryption randomness per query of the batch
                minus, idx = cl.runOfflinePhase(clientset, encSeedBase=100 + 1000 * q)
                di, dm = torch.from_numpy(idx.view(np.int64)).cuda(), torch.from_numpy(minus.view(np.int64)).cuda()
                keep.append((di, dm))
                op.setIndexDevice(di.data_ptr(), query=q)
                op.setMinusCompareElementDevice(dm.data_ptr(), query=q)
        torch.cuda.synchronize()
        us = {name: [] for name in legs}
        gc.collect()
        for blk in range(args.warmup + args.blocks):
            for name, leg in legs.items():
                op = leg["op"]
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
        rec = {}
        truth = sorted(int(v) for v in server[:nC // 2 + 1])
        for name, leg in legs.items():
            res = leg["op"].getResultList().copy()
            res = res[None] if nq == 1 else res
            budgets = []
            for q in range(nq):
                budgets.append(int(leg["cl"].decrypt(res[q], budget=True)[1].min()))
                assert sorted(int(v) for v in leg["cl"].extractIntersection(res[q])) == truth, "%s, query %d" % (name, q)
            st = stats(us[name])
            rec[name] = {"step_us": st, "per_query_us": {k_: (v / nq if k_ != "blocks" else v) for k_, v in st.items()},
                         "budget_bits_min_per_query": budgets}
        d = rec["tiled"]["step_us"]["median"] - rec["untiled"]["step_us"]["median"]
        spread = rec["untiled"]["step_us"]["max"] - rec["untiled"]["step_us"]["min"]
        rec["verdict"] = "tiled is %.1f us %s than untiled per step (untiled's spread: %.1f us); ratio of medians %.2f" % (
            abs(d), "shorter" if d < 0 else "longer", spread, rec["untiled"]["step_us"]["median"] / rec["tiled"]["step_us"]["median"])
        out["batches"][str(nq)] = rec
        del keep
    out["legs"] = {name: {k_: leg[k_] for k_ in ("R", "layers", "offline_ms", "database_bytes", "result_bytes_per_query")}
                   for name, leg in legs.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for leg in legs.values():
        leg["cc"].close()


if __name__ == "__main__":
    main()
