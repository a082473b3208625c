"""C3 host-memory query stream with full and with reduced result lists, in one process: python tools/result_limbs_stream.py [--out FILE]

The stream is tools/seeded_stream.py's: query slots on one database (piehip_attach_database), batches of three queries per run(),
every query staged piece by piece from page-locked arrays, the result lists [b][3] back in page-locked host memory; while one slot
evaluates and downloads, the next slot's batch crosses PCIe.  Legs, over the same slots:
  full          results as they are: [2][4][N] per ciphertext, 14 MiB per query down
  keep1         piehip_set_result_limbs(1): 3.5 MiB per query down
  seeded_keep1  the same with seeded queries (c0 + seeds up: 14.5 MiB per query instead of 29)
  keep2         piehip_set_result_limbs(2): 7 MiB per query down
The passes ALTERNATE between the legs (full, keep1, seeded_keep1, keep2, full, ...), so that a drift of the box shows in every leg
alike; the first pass of every leg is a warm-up and is not counted.  The comparison is against the full leg of the same run: a
reduced leg is called faster only if its best pass beats the full leg's best pass by more than the full leg's own spread between
its counted passes.  Python's cyclic GC is off inside the legs, as in bench.py.  Per pass the device-side upload and
evaluate+download times (piehip_set_host_path_timing) are reported too.  Query contents are synthetic (uniform residues).
Prints one JSON line.
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

LEGS = (("full", 4, False), ("keep1", 1, False), ("seeded_keep1", 1, True), ("keep2", 2, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=3, help="query slots")
    ap.add_argument("--batches", type=int, default=24, help="batches per pass (every slot gets batches / slots)")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3, help="counted passes per leg (one more, the first, warms up)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from nested_hashing_psi_amd import pie
    N, L, t, k, e, K, E, b = 16384, 4, 4296540161, 2, 4949, 2, 14, 14   # C3 (bench.CONFIGS["C3"])
    B, nq, nsl = k * e, args.batch, args.slots
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
    streams = [torch.cuda.Stream() for _ in range(nsl - 1)]
    ops = [op] + [pie.BatchedFHEHIPPIE(pie.PieContext(N, L, t, stream=s.cuda_stream), attachTo=op) for s in streams]
    for o in ops:
        o.setQueryBatch(nq)
        o.cc.set_run_streams(1)   # one queue per run() on every slot, as bench.py's stream legs
    idx_h, minus_h = limbs(K, E, 2), limbs(2)
    c0i_h, c0m_h = np.ascontiguousarray(idx_h[:, :, 0]), np.ascontiguousarray(minus_h[0])
    seeds_i = rng.integers(0, 256, (K, E, 32), dtype=np.uint8)
    seeds_m = rng.integers(0, 256, (32,), dtype=np.uint8)

    def prepare(keep, seeded):
        """the setting on every slot, its page-locked arrays (the result array follows the setting) and their contents"""
        bufs = []
        for o in ops:
            o.setResultLimbs(keep)
            qb = []
            for q_ in range(nq):
                bi, bm, br = o.hostBuffers(query=q_)
                ci = bi.reshape(-1)[:K * E * L * N].reshape(K, E, L, N)
                cm = bm.reshape(-1)[:L * N].reshape(L, N)
                if seeded:
                    ci[...] = c0i_h
                    cm[...] = c0m_h
                else:
                    bi[...] = idx_h
                    bm[...] = minus_h
                qb.append((bi, bm, br, ci, cm))
            bufs.append(qb)
        return bufs

    def one_pass(bufs, seeded):
        nb = max(args.batches // nsl, 2) * nsl
        for o in ops:
            o.cc.set_host_path_timing(True)
        torch.cuda.synchronize()
        times = []
        t0 = time.perf_counter()
        for i in range(nb + nsl):
            o, qb = ops[i % nsl], bufs[i % nsl]
            if i >= nsl:
                o.waitHost()
                times.append(o.cc.host_path_times())
            if i < nb:
                for q_ in range(nq):
                    if seeded:
                        o.stageMinusSeeded(qb[q_][4], seeds_m, query=q_)
                    else:
                        o.stageMinus(qb[q_][1], query=q_)
                for h in range(K):
                    for q_ in range(nq):
                        if seeded:
                            o.stageIndexRowSeeded(h, qb[q_][3][h], seeds_i[h], query=q_)
                        else:
                            o.stageIndexRow(h, qb[q_][0][h], query=q_)
                o.runStaged(qb[0][2])
        wall = time.perf_counter() - t0
        for o in ops:
            o.cc.set_host_path_timing(False)
        up = sorted(x[0] for x in times)
        rest = sorted(x[1] for x in times)
        return {"ms_per_query": wall * 1e3 / (nb * nq), "upload_ms_per_run": up[len(up) // 2],
                "evaluate_and_download_ms_per_run": rest[len(rest) // 2], "batches": nb}

    passes = {name: [] for name, _, _ in LEGS}
    gc.collect()
    for rnd in range(args.passes + 1):
        for name, keep, seeded in LEGS:
            bufs = prepare(keep, seeded)
            gc.disable()
            p = one_pass(bufs, seeded)
            gc.enable()
            if rnd:   # round 0 warms every leg up
                passes[name].append(p)
    ms = {name: [p["ms_per_query"] for p in ps] for name, ps in passes.items()}
    best = {name: min(v) for name, v in ms.items()}
    full_spread = max(ms["full"]) - min(ms["full"])
    verdict = {name: ("faster than the full leg by more than its spread" if best["full"] - best[name] > full_spread
                      else "not faster than the full leg by more than its spread")
               for name in best if name != "full"}
    out = {"config": "C3", "queries_per_run": nq, "slots": nsl, "ms_per_query_passes": ms, "best_ms_per_query": best,
           "full_leg_spread_ms_per_query": full_spread, "verdict": verdict,
           "result_mib_down_per_query": {name: b * 2 * keep * N * 8 / 2**20 for name, keep, _ in LEGS},
           "query_mib_up_per_query": {name: ((c0i_h.nbytes + c0m_h.nbytes) if seeded else (idx_h.nbytes + minus_h.nbytes)) / 2**20
                                      for name, _, seeded in LEGS},
           "passes": passes, "device": torch.cuda.get_device_name(0),
           "pass_order": "legs alternate; the first pass of every leg is a warm-up and is not counted"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for o in ops[1:]:
        o.cc.close()
    cc.close()


if __name__ == "__main__":
    main()
