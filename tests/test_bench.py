"""bench.py's own contract: a plain run times exactly --steps steps and prints one JSON line; --dump-outputs writes the last
timed step's result ciphertexts exactly, bounded in size, the same from run to run and with or without --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_dump(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_plain_run_is_the_default():
    import bench
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None and a.repeats is None
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--steps", "7"])
    assert a.full and a.dump_outputs == "out" and a.steps == 7
    assert bench.parse_args(["--timed-only"]).full          # the per-kernel passes belong to --full


def test_dump_outputs_are_exact_and_bounded(tmp_path):
    import bench
    q = (1 << 60) - 93
    rng = np.random.default_rng(5)
    # C3's timed step: 14 bin layers x 3 queries, N = 16384, 4 primes -- more than the limit, so a sample of positions
    res = rng.integers(0, q, (14, 3, 2, 4, 16384), dtype=np.uint64)
    res[0, 0, 0, 0, :4] = [0, 1, (1 << 30) - 1, q - 1]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res)
    a, b = load_dump(str(tmp_path / "a")), load_dump(str(tmp_path / "b"))
    assert sorted(a) == ["result_hi.npy", "result_lo.npy", "result_positions.npy"]
    assert all((a[n] == b[n]).all() and a[n].dtype == np.float64 for n in a)
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in a) <= 64 * 2**20
    pos = a["result_positions.npy"].astype(np.int64)
    assert len(pos) < 16384 and (np.diff(pos) > 0).all() and a["result_hi.npy"].size <= bench.DUMP_RESIDUES
    got = a["result_hi.npy"].astype(np.uint64) * np.uint64(1 << 30) + a["result_lo.npy"].astype(np.uint64)
    assert (got == res[..., pos]).all()
    # a small result is written whole
    small = res[:2, :1, :, :2, :64]
    bench.dump_outputs(str(tmp_path / "c"), small)
    c = load_dump(str(tmp_path / "c"))
    assert (c["result_positions.npy"] == np.arange(64)).all()
    assert (c["result_hi.npy"].astype(np.uint64) * np.uint64(1 << 30) + c["result_lo.npy"].astype(np.uint64) == small).all()


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """config C1 (a batch of three queries per run()): two plain runs and one --timed-only run (per-kernel passes, and the further
    query slots of --full made) dump the same results, laid out [bin layer][query]: a run with one query per run() dumps exactly
    the batch's query 0"""
    def bench(d, *extra):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "6",
                            "--warmup", "2", "--dump-outputs", str(tmp_path / d)] + list(extra),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    line = bench("a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 6 and line["repeats"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(3 * 7 / (line["ms_per_step"] * 1e-3))
    for k in ("kernels", "roofline", "one_query_at_a_time", "ref_timer", "e2e_psi", "cpu_baseline"):
        assert k not in line, k
    full = bench("c", "--timed-only")
    assert "kernels" in full and full["roofline"] is not None
    bench("b")
    one = bench("d", "--batch", "1")
    assert one["queries_per_step"] == 1
    a, b, c, d = (load_dump(str(tmp_path / d)) for d in "abcd")
    assert sorted(a) == ["result_hi.npy", "result_lo.npy", "result_positions.npy"]
    assert a["result_hi.npy"].shape == (7, 3, 2, 2, 4096)      # C1: b = 7, three queries, 2 primes, N = 4096, all positions
    assert (a["result_hi.npy"] < 2**30).all() and (a["result_lo.npy"] < 2**30).all() and a["result_hi.npy"].any()
    for n in a:
        assert (a[n] == b[n]).all() and (a[n] == c[n]).all(), n
    assert d["result_hi.npy"].shape == (7, 1, 2, 2, 4096) and (d["result_positions.npy"] == a["result_positions.npy"]).all()
    for n in ("result_hi.npy", "result_lo.npy"):
        assert (d[n][:, 0] == a[n][:, 0]).all(), n                 # every bin layer of query 0 in its own cell
        assert (a[n][:, 1] != a[n][:, 0]).any() and (a[n][1:] != a[n][:1]).any(), n
