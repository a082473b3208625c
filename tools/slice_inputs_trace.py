"""The copies behind the eight host setters of a sliced handle's inputs, for a memory-copy trace (no counters in that run):
    rocprofv3 --memory-copy-trace --kernel-trace --output-format json -d DIR -o slice_inputs -- python tools/slice_inputs_trace.py [--lib SO]
    python tools/slice_inputs_trace.py --table DIR/slice_inputs_results.json
One process, one handle with the three units [2, 5) at N = 4096, L = 4, K = 2, E = 3, b = 2, a batch of two (the shape of
tests/test_gpu_slice_inputs.py).  Each setter is called once; a 40 KiB host-to-device copy in front of each marks the trace, and one
more in front of and behind each of the two closing piehip_run_slice.  The first has query 0's two seeded pieces to expand: one
job-table copy ((3 + 1) * 3 jobs: small, so it shows as a __amd_rocclr_copyBuffer blit kernel, not as a memory-copy record) and one
expansion launch in front of stage A; the second has nothing pending.  --lib: another build of libpiehip.so (the parent commit's)
behind the same Python.
--table prints, per section, the copies to the device in trace order with their bytes, and the kernels of the two runs."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARK = 40960   # small copies travel in a blit kernel and are no memory-copy records: the marker must be one
SETTERS = ["set_index_slice_q", "set_minus_slice_q", "set_index_slice_from_q", "set_minus_slice_from_q", "set_index_slice_seeded_q",
           "set_minus_slice_seeded_q", "set_index_slice_seeded_from_q", "set_minus_slice_seeded_from_q"]


def run(lib_path):
    import torch
    from nested_hashing_psi_amd import _lib, pie
    if lib_path:
        _lib.LIB_PATH = os.path.abspath(lib_path)
    lib = _lib.lib()
    N, L, K, E, b, nq, ul, uh, t = 4096, 4, 2, 3, 2, 2, 2, 5, 4296540161
    un = uh - ul
    cc = pie.PieContext(N, L, t)
    rng = np.random.default_rng(1)
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    P, S = lambda a: a.ctypes.data_as(u64p), lambda a: a.ctypes.data_as(u8p)

    def limbs(*shape):   # residues below every modulus of the chain
        return rng.integers(0, int(min(cc.q)), shape, dtype=np.uint64)

    def ok(rc):
        assert rc == 0, lib.piehip_last_error().decode()

    ok(lib.piehip_load_db_sliced(cc._h, K, b, E, ul, uh, P(limbs(un, b, E, N)), 0, b, P(limbs(b, L, N))))
    ok(lib.piehip_set_query_batch(cc._h, nq))
    mark_src, mark_dst = torch.zeros(MARK // 8, dtype=torch.int64), torch.zeros(MARK // 8, dtype=torch.int64, device="cuda")
    seeds = rng.integers(0, 256, (K, E, 32), dtype=np.uint8)
    args = [(1, limbs(un, E, 2, N)), (1, limbs(un, 2, N)), (0, limbs(K, E, 2, L, N)), (0, limbs(2, L, N)),
            (0, limbs(un, E, N), seeds), (0, limbs(un, N), seeds[0, 0]), (0, limbs(K, E, L, N), seeds), (0, limbs(L, N), seeds[0, 0])]
    torch.cuda.synchronize()
    for name, (q, src, *sd) in zip(SETTERS, args):
        mark_dst.copy_(mark_src)
        torch.cuda.synchronize()
        ok(getattr(lib, "piehip_" + name)(cc._h, q, P(src), *[S(np.ascontiguousarray(s)) for s in sd]))
    for _ in range(2):   # around the run: the job table and the expansion of query 0's pieces, stage A
        mark_dst.copy_(mark_src)
        torch.cuda.synchronize()
        ok(lib.piehip_run_slice(cc._h))
        ok(lib.piehip_sync(cc._h))
    mark_dst.copy_(mark_src)
    torch.cuda.synchronize()
    cc.close()
    print("slice_inputs_trace: %d setters and two piehip_run_slice on one handle with %d units" % (len(SETTERS), un))


def table(path):
    recs = json.load(open(path))["rocprofiler-sdk-tool"][0]
    names = {s["kernel_id"]: s["truncated_kernel_name"] for s in recs["kernel_symbols"]}
    # every copy the trace holds goes to the device; the 2D copies out of pageable memory are staged and show as device-to-device
    h2d = sorted(recs["buffer_records"]["memory_copy"], key=lambda r: r["start_timestamp"])
    marks = [i for i, r in enumerate(h2d) if r["bytes"] == MARK]
    assert len(marks) == len(SETTERS) + 3, "markers in the trace: %d" % len(marks)
    sections = SETTERS + ["run_slice (two seeded pieces pending)", "run_slice (nothing pending)"]
    print("%-42s %6s  %s" % ("section", "copies", "bytes per copy to the device, in trace order"))
    for k, name in enumerate(sections):
        part = h2d[marks[k] + 1:marks[k + 1]]
        print("%-42s %6d  %s" % (name, len(part), " ".join(str(r["bytes"]) for r in part)))
    for k in (len(SETTERS), len(SETTERS) + 1):
        t0, t1 = h2d[marks[k]]["start_timestamp"], h2d[marks[k + 1]]["start_timestamp"]
        ks = sorted((r for r in recs["buffer_records"]["kernel_dispatch"] if t0 <= r["start_timestamp"] < t1), key=lambda r: r["start_timestamp"])
        print("kernels of %s:" % sections[k])
        for r in ks:
            print("    %s" % names[r["dispatch_info"]["kernel_id"]])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--table")
    a = ap.parse_args()
    table(a.table) if a.table else run(a.lib)
