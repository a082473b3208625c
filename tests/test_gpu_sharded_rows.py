"""host/ShardedBatchedFHEHIPPIE.hpp (one process, one context per device) with setResultLimbs, setChainLimbs, setChainSchedule,
setResultRelin and the layerTiling constructor argument: tests/sharded_rows_check.cpp drives it over three contexts on the one device
-- every setter alone and together, the roll-back when one shard refuses, a K = 2 run with no key on any context, C1's packing R = 3 of
b = 7 bin layers into three tiled layers -- and compares every result list with a file written here from the definitions
(exact_rows of tests/test_gpu_gather_rows.py; the database from the oracle's shuffle, packing and masks, tiled by tests/layer_tiling.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests.layer_tiling import tile_db_slots, tile_masks
from tests.slice_ranks_util import T16, rand_limbs
from tests.test_gpu_gather_rows import exact_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "nested_hashing_psi_amd")
N, L, T, k, e, K, b, E = 4096, 3, T16, 2, 5, 2, 7, 3     # (the constants of the program)
SHUFFLE, MASK = 11, 22


def test_settings_tiling_and_roll_back_over_three_shards(ob, tmp_path):
    exe = str(tmp_path / "sharded_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "sharded_rows_check.cpp"),
                           "-L" + LIBDIR, "-lpiehip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    o = ob.Oracle(N, L, T)
    rng = np.random.default_rng(2024)
    q = o.moduli[:L]
    tbl = rng.integers(1, 65000, (k, e, K, b, E), dtype=np.uint64)
    tbl.tofile(tmp_path / "table.bin")
    evk, idx, minus = rand_limbs(rng, q, (L, 2), N), rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)
    evk.tofile(tmp_path / "evk.bin")
    idx.tofile(tmp_path / "idx.bin")
    minus.tofile(tmp_path / "minus.bin")
    # the operator's database: bin layers shuffled, packed, masks drawn, encoded (BatchedFHEHIPPIE.cpp:23-82)
    shuffled = tbl.copy()
    ob.hct_shuffle_bins(shuffled, SHUFFLE)
    slots = ob.pack_db(shuffled)
    encode = lambda s: np.stack([o.encode_eval(v) for v in s.reshape(-1, s.shape[-1])]).reshape(s.shape[:-1] + (L, N))
    db, masks = encode(slots), encode(ob.masks(T, b, k * e, MASK))
    db_t, masks_t = encode(tile_db_slots(slots, 3)), encode(tile_masks(ob, T, b, k * e, MASK, 3))
    assert db_t.shape == (K, 3, E, L, N) and masks_t.shape == (3, L, N)
    wants = {
        "full": exact_rows(ob, o, idx, minus, db, masks, evk, "0:1:0"),
        "keep1": exact_rows(ob, o, idx, minus, db, masks, evk, "1:1:0"),
        "chain2": exact_rows(ob, o, idx, minus, db, masks, evk, "0:1:2"),
        "deg2": exact_rows(ob, o, idx, minus, db, masks, None, "0:0:0"),
        "deg2_keep2": exact_rows(ob, o, idx, minus, db, masks, None, "2:0:0"),
        "all": exact_rows(ob, o, idx, minus, db, masks, evk, "1:0:2"),
        "tiled": exact_rows(ob, o, idx, minus, db_t, masks_t, evk, "0:1:0"),
        "tiled_keep1": exact_rows(ob, o, idx, minus, db_t, masks_t, evk, "1:1:0"),
    }
    assert wants["all"].shape == (b, 3, 1, N) and wants["tiled"].shape == (3, 2, L, N)
    for name, w in wants.items():
        np.ascontiguousarray(w, dtype=np.uint64).tofile(tmp_path / ("want_%s.bin" % name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sharded rows ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
