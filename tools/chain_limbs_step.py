"""C3 run() with the product chain on all four limbs and on three, in one process:
    python tools/chain_limbs_step.py [--parent-lib PATH] [--lib PATH] [--out FILE] [--profile]

Step legs: one handle, C3's shape, a batch of three queries per run(), inputs resident in HBM, results left in HBM.  Legs
  default      piehip_set_chain_limbs(L), keep = L      (what the parent commit runs)
  lc3          piehip_set_chain_limbs(3), keep = L      (rows of three limbs)
  lc3_keep1    piehip_set_chain_limbs(3), keep = 1
  keep1        piehip_set_chain_limbs(L), keep = 1
  parent       --parent-lib PATH: the same default step through another build of the library (the parent commit's), loaded beside
               this tree's into the same process, on a handle of its own with the same database, key and queries
A block is `--runs` run()s back to back and one sync; the blocks ALTERNATE between the legs, so that a drift of the box shows in
every leg alike; the first `--warmup` blocks of every leg are not counted.  Reported per leg: median [min, max] of the counted
blocks, in microseconds per step (one run() of three queries).  The tool measures and gates nothing; its verdicts compare medians
against the spread (max - min) of the leg compared with.
--lib PATH: time another build of the library in this process instead: a -DPIEHIP_CHAIN_DROP_FUSED=0 build (the fallback), or the
parent commit's (it has no setting: only the default and keep1 legs run).  A handle of the parent library beside this tree's brings
the process to six streams; with the runtime's default of four hardware queues two of them then share one and a two-queue run()
serialises (measured: profiles/chain_limbs/README.txt), so the fifth leg wants GPU_MAX_HW_QUEUES=8 in the environment.
--lc3-only: one leg, for a kernel trace of the lc3 step taken alone.  --profile: per-class launch times of the default and the
lc3 step from the library's own event brackets (piehip_profile_read_n), after the timed legs.
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


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "blocks": len(s)}


class ParentStep:
    """the default step through another libpiehip.so, by its C entry points (every one of them older than this tool)"""

    def __init__(self, path, symbols, N, L, t, key, slots, mask_slots, nq, dev_inputs):
        self.lib = C.CDLL(os.path.abspath(path))
        names = ("piehip_create", "piehip_destroy", "piehip_load_relin_key", "piehip_load_db_slots", "piehip_set_query_batch",
                 "piehip_set_index_device_q", "piehip_set_minus_device_q", "piehip_run", "piehip_sync", "piehip_last_error")
        for n in names:
            f = getattr(self.lib, n)
            f.restype, f.argtypes = symbols[n]
        self.h = C.c_void_p()
        u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        self.ok(self.lib.piehip_create(C.byref(self.h), N, L, t, None, None, 0, None))
        self.ok(self.lib.piehip_load_relin_key(self.h, key.ctypes.data_as(u64p)))
        K, b, E, B = slots.shape
        self.ok(self.lib.piehip_load_db_slots(self.h, K, b, E, B, slots.ctypes.data_as(i64p), mask_slots.ctypes.data_as(i64p)))
        self.ok(self.lib.piehip_set_query_batch(self.h, nq))
        for i, (di, dm) in enumerate(dev_inputs):
            self.ok(self.lib.piehip_set_index_device_q(self.h, i, C.c_void_p(di.data_ptr())))
            self.ok(self.lib.piehip_set_minus_device_q(self.h, i, C.c_void_p(dm.data_ptr())))

    def ok(self, rc):
        if rc:
            raise RuntimeError("parent library: %s" % self.lib.piehip_last_error().decode())

    def run(self, sync=True):
        self.ok(self.lib.piehip_run(self.h))
        if sync:
            self.sync()

    def sync(self):
        self.ok(self.lib.piehip_sync(self.h))

    def close(self):
        self.lib.piehip_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=17, help="counted blocks per leg")
    ap.add_argument("--warmup", type=int, default=3, help="uncounted blocks per leg")
    ap.add_argument("--runs", type=int, default=20, help="run()s per block")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libpiehip.so: the fifth leg")
    ap.add_argument("--lib", default=None, help="time another build of THIS tree's library (-DPIEHIP_CHAIN_DROP_FUSED=0: the fallback)")
    ap.add_argument("--lc3-only", action="store_true", help="only the lc3 leg (for a kernel trace of that step alone)")
    ap.add_argument("--profile", action="store_true", help="per-class launch times of the default and the lc3 step")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from nested_hashing_psi_amd import _lib, pie
    has_setting = True
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        has_setting = hasattr(C.CDLL(_lib.LIB_PATH), "piehip_set_chain_limbs")
        if not has_setting:   # the parent commit's library in a process of its own: the legs without the setting
            for s_ in ("piehip_set_chain_limbs", "piehip_get_chain_limbs"):
                _lib.SYMBOLS.pop(s_, None)
    N, L, t, k, e, K, E, b = 16384, 4, 4296540161, 2, 4949, 2, 14, 14   # C3 (bench.CONFIGS["C3"])
    B, nq, Lc = k * e, args.batch, 3
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
    key = limbs(L, 2)
    cc.load_relin_key(key)
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
    parent = None
    if args.parent_lib and not args.lc3_only:
        parent = ParentStep(args.parent_lib, _lib.SYMBOLS, N, L, t, key, np.ascontiguousarray(slots), np.ascontiguousarray(mask_slots), nq, dev)
    legs = [("default", L, L), ("lc3", Lc, L), ("lc3_keep1", Lc, 1), ("keep1", L, 1)]
    if args.lc3_only:
        legs = [legs[1]]
    if not has_setting:
        legs = [l for l in legs if l[1] == L]
    if parent:
        legs.append(("parent", None, None))

    def prepare(name, lc, keep):
        if name == "parent":
            return parent
        if has_setting:
            op.setChainLimbs(lc)
        op.setResultLimbs(keep)
        return op

    us = {name: [] for name, _, _ in legs}
    gc.collect()
    for blk in range(args.warmup + args.blocks):
        for name, lc, keep in legs:
            o = prepare(name, lc, keep)
            o.run()
            gc.disable()
            t0 = time.perf_counter()
            for _ in range(args.runs):
                o.run(sync=False)
            o.sync()
            dt = time.perf_counter() - t0
            gc.enable()
            if blk >= args.warmup:
                us[name].append(dt * 1e6 / args.runs)
    step = {name: stats(v) for name, v in us.items()}

    def compare(a, ref):   # leg a against leg ref, by ref's own spread
        if a not in step or ref not in step:
            return None
        d, spread = step[a]["median"] - step[ref]["median"], step[ref]["max"] - step[ref]["min"]
        return "%s is %.1f us %s than %s (%s's spread: %.1f us)" % (a, abs(d), "shorter" if d < 0 else "longer", ref, ref, spread)
    verdict = {k_: v for k_, v in (("default_vs_parent", compare("default", "parent")), ("lc3_vs_default", compare("lc3", "default")),
                                   ("lc3_keep1_vs_keep1", compare("lc3_keep1", "keep1"))) if v}
    out = {"config": "C3", "queries_per_run": nq, "runs_per_block": args.runs, "step_us": step, "verdict": verdict,
           "library": args.lib or "this tree's", "parent_library": args.parent_lib, "device": torch.cuda.get_device_name(0),
           "block_order": "legs alternate; the first %d blocks of every leg are not counted" % args.warmup}
    if args.profile and has_setting:
        out["per_class_us"] = {}
        for name, lc in (("default", L), ("lc3", Lc)):
            op.setChainLimbs(lc)
            op.setResultLimbs(L)
            cc.set_run_streams(1)   # one queue: the brackets of two queues overlap
            cc.set_profiling(True)
            acc = {}
            for _ in range(9):
                op.run()
                for kname, rec in cc.profile().items():
                    acc.setdefault(kname, []).append(rec["ms"] * 1e3)
            cc.set_profiling(False)
            cc.set_run_streams(0)
            out["per_class_us"][name] = {kname: sorted(v)[len(v) // 2] for kname, v in acc.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if parent:
        parent.close()
    cc.close()


if __name__ == "__main__":
    main()
