"""piehip_create + the device-side database build + the first run() of a fresh process, C3 shape: python tools/first_run_timing.py TREE
(the tree whose package and library are used).  One JSON line: milliseconds per step."""
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch  # noqa: F401  (before the library, as _lib does)

import bench
from nested_hashing_psi_amd import pie
from nested_hashing_psi_amd.client import BatchedFHEPSIClient
assert os.path.dirname(os.path.abspath(pie.__file__)).startswith(root), pie.__file__

cfg = bench.CONFIGS["C3"]
t, k, e, K, E, b = cfg["t"], cfg["k"], cfg["e"], cfg["K"], cfg["E"], cfg["b"]
rng = np.random.default_rng(1)
items = np.unique(rng.integers(1, t, cfg["S"] + cfg["C"] + 8192, dtype=np.uint64))
rng.shuffle(items)
server, clientset = items[:cfg["S"]].copy(), items[cfg["S"] - 500:cfg["S"] + 524].copy()
T = {}
t0 = time.perf_counter()
cc = pie.PieContext(cfg["N"], cfg["L"], t)
T["create"] = time.perf_counter() - t0
t0 = time.perf_counter()
cl = BatchedFHEPSIClient(cc, k, e, K, E, b)
evk = cl.runSetUpPhase()
cc.load_relin_key(evk)
T["client_setup_and_key"] = time.perf_counter() - t0
t0 = time.perf_counter()
srv = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=dict(k=k, e=e, K=K, b=b, E=E, evict_seed=1, shuffle_seed=2, mask_seed=3))
T["build_db"] = time.perf_counter() - t0
t0 = time.perf_counter()
minus_ct, idx_ct = cl.runOfflinePhase(clientset)
srv.setMinusCompareElement(minus_ct)
srv.setIndex(idx_ct)
T["client_offline_and_inputs"] = time.perf_counter() - t0
t0 = time.perf_counter()
srv.run()
T["first_run"] = time.perf_counter() - t0
t0 = time.perf_counter()
srv.run()
T["second_run"] = time.perf_counter() - t0
res = srv.getResultList()
out = {n: round(v * 1e3, 3) for n, v in T.items()}
out["create_build_db_first_run"] = round((T["create"] + T["build_db"] + T["first_run"]) * 1e3, 3)
out["tree"] = sys.argv[1]
out["result_digest"] = int(np.bitwise_xor.reduce(res.reshape(-1)))
print(json.dumps(out))
