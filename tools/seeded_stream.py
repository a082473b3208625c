"""C3 host-memory query stream with full and with seeded queries, in one process: python tools/seeded_stream.py [--out FILE]

The stream is bench.py's staged batch leg (reference_timer, "staged_batch_stream"): query slots on one database
(piehip_attach_database), batches of three queries per run(), every query staged piece by piece from its own page-locked arrays
(minus elements first, then the index matrices row by row across the batch), the result lists [b][3] back in host memory; while one
slot evaluates and downloads, the next slot's batch crosses PCIe.  Python's cyclic GC is off inside the legs, as in bench.py.
  full     piehip_stage_minus_q / piehip_stage_index_row_q: 29 MiB per query up, c0 and c1
  seeded   piehip_stage_minus_seeded_q / piehip_stage_index_row_seeded_q: c0 only (14.5 MiB) + 32-byte seeds; run_staged queues
           one expansion launch per batch (kernels_seed.hip) in front of the evaluation
Every leg is a warm-up pass and two timed passes; the figure is the faster timed pass (bench.py's rule).  Per pass the device-side
upload and evaluate+download times (piehip_set_host_path_timing) are reported too.  The query contents are synthetic (uniform
residues): the work is that of any query.  Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="2,3", help="query slot counts to measure")
    ap.add_argument("--batches", type=int, default=24, help="batches per timed pass (every slot gets batches / slots)")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
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
    nslots_all = [int(x) for x in args.slots.split(",")]
    streams = [torch.cuda.Stream() for _ in range(max(nslots_all) - 1)]
    ops = [op] + [pie.BatchedFHEHIPPIE(pie.PieContext(N, L, t, stream=s.cuda_stream), attachTo=op) for s in streams]
    for o in ops:
        o.setQueryBatch(nq)
        o.cc.set_run_streams(1)   # one queue per run() on every slot, as bench.py's stream legs
    # per slot and query: page-locked staging holding a full query; the seeded form uses the first half of the same arrays
    idx_h, minus_h = limbs(K, E, 2), limbs(2)
    c0i_h, c0m_h = np.ascontiguousarray(idx_h[:, :, 0]), np.ascontiguousarray(minus_h[0])
    seeds_i = rng.integers(0, 256, (K, E, 32), dtype=np.uint8)
    seeds_m = rng.integers(0, 256, (32,), dtype=np.uint8)
    bufs = []
    for o in ops:
        qb = []
        for q_ in range(nq):
            bi, bm, br = o.hostBuffers(query=q_)
            ci = bi.reshape(-1)[:K * E * L * N].reshape(K, E, L, N)
            cm = bm.reshape(-1)[:L * N].reshape(L, N)
            qb.append((bi, bm, br, ci, cm))
        bufs.append(qb)

    def fill(seeded):
        for qb in bufs:
            for bi, bm, _, ci, cm in qb:
                if seeded:
                    ci[...] = c0i_h
                    cm[...] = c0m_h
                else:
                    bi[...] = idx_h
                    bm[...] = minus_h

    def leg(allops, seeded):
        nsl = len(allops)
        nb = max(args.batches // nsl, 2) * nsl
        for o in allops:
            o.cc.set_host_path_timing(True)
        passes = []
        for _ in range(3):
            torch.cuda.synchronize()
            times = []
            t0 = time.perf_counter()
            for i in range(nb + nsl):
                o, qb = allops[i % nsl], bufs[i % nsl]
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
            up = sorted(x[0] for x in times)
            rest = sorted(x[1] for x in times)
            passes.append({"ms_per_query": wall * 1e3 / (nb * nq), "upload_ms_per_run": up[len(up) // 2],
                           "evaluate_and_download_ms_per_run": rest[len(rest) // 2], "batches": nb})
        for o in allops:
            o.cc.set_host_path_timing(False)
        return min(p["ms_per_query"] for p in passes[1:]), passes

    gc.collect()
    gc.disable()
    res = {"full": {}, "seeded": {}}
    passes = {"full": {}, "seeded": {}}
    for nsl in nslots_all:
        for mode in ("full", "seeded"):
            fill(mode == "seeded")
            res[mode][str(nsl)], passes[mode][str(nsl)] = leg(ops[:nsl], mode == "seeded")
    gc.enable()
    best_full = min(res["full"].values())
    best_seeded = min(res["seeded"].values())
    mib_full = (idx_h.nbytes + minus_h.nbytes) / 2**20
    mib_seeded = (c0i_h.nbytes + c0m_h.nbytes + seeds_i.nbytes + seeds_m.nbytes) / 2**20
    out = {"config": "C3", "queries_per_run": nq, "full_ms_per_query": res["full"], "seeded_ms_per_query": res["seeded"],
           "best_full_ms_per_query": best_full, "best_seeded_ms_per_query": best_seeded, "seeded_over_full": best_seeded / best_full,
           "query_mib_up": {"full": mib_full, "seeded": mib_seeded}, "result_mib_down": b * 2 * L * N * 8 / 2**20,
           "full_ct_per_s": b / (best_full * 1e-3), "seeded_ct_per_s": b / (best_seeded * 1e-3), "passes": passes,
           "device": torch.cuda.get_device_name(0), "stream_figure": "the faster of two timed passes per leg (after a warm-up pass)"}
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
