"""The native collectives (csrc/piehip_rccl.cpp) with result rows of another shape than [2][L][N]: piehip_set_result_limbs,
piehip_set_result_relin(0) and piehip_set_chain_limbs / _schedule on every rank, piehip_rccl_agree_rows, then the gather of rows
[ncomp][rl][N] -- as 2 and 3 processes on one GPU over the stand-in transport of tests/fake_rccl, which tests/rows_ranks_main.cpp loads
by the path it is handed (no process started here has its loader environment touched).

Every comparison is bit for bit, on every word, against the definitions the one-handle tests use: o.pie_run, run_deg2_exact
(tests/test_result_relin.py), run_chain_limbs_exact (chain_layer_exact, level_key, level_oracle of tests/test_chain_limbs.py),
run_chain_schedule_exact (tests/test_chain_schedule.py, which composes the same pieces per product) and mod_reduce_exact
(tests/test_result_limbs.py) on the level the rows leave the chain at.  Nothing is compared with a one-handle GPU run.

  test_rows_of_every_setting_are_gathered   the settings alone and together, uneven shares, a root other than rank 0, a batch with
                                            per-query keys, degree-2 rows with no key on any rank, the folded ring with the fused
                                            drop, and a setting that changes between the two rounds with a fresh agreement
  test_ranks_with_different_settings        all see same = 0, every gather is refused locally, nothing is posted, everybody exits 0
  test_a_changed_setting_needs_a_new_agreement
  test_default_rows_need_no_agreement
  test_one_rank_over_rccl_keeps_one_limb    the real RCCL with one rank (it refuses two ranks on one device)
"""
import subprocess

import numpy as np
import pytest

from tests.slice_ranks_util import T16, T32, build_programs, rand_limbs, wait_all
from tests.test_chain_limbs import level_oracle, run_chain_limbs_exact
from tests.test_chain_schedule import last_level, run_chain_schedule_exact
from tests.test_result_limbs import mod_reduce_exact
from tests.test_result_relin import run_deg2_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    fake, exes = build_programs(tmp_path_factory.mktemp("rows_ranks"), ["rows_ranks_main"])
    return fake, exes["rows_ranks_main"]


def _parse(setting):
    keep, relin, sched = setting.split(":")
    return int(keep), bool(int(relin)), [int(v) for v in sched.split("-") if int(v)]


def exact_rows(ob, o, idx, minus, db, masks, evk, setting):
    """the definition of run() under a setting "keep:relin:schedule" -> [b][ncomp][rl][N]"""
    keep, relin, sched = _parse(setting)
    L, K = o.L, db.shape[0]
    if not sched:
        rows, at = (o.pie_run(idx, minus, db, masks, evk) if relin else run_deg2_exact(o, idx, minus, db, masks, evk)), L
    elif len(sched) == 1:
        rows, at = run_chain_limbs_exact(ob, o, idx, minus, db, masks, evk, sched[0], relin_last=relin), sched[0]
    else:
        rows, at = run_chain_schedule_exact(ob, o, idx, minus, db, masks, evk, sched, relin_last=relin), last_level(sched, K)
    if keep and keep < at:
        rows = mod_reduce_exact(o if at == L else level_oracle(ob, o, at), rows, keep)
    return np.ascontiguousarray(rows)


def _write_case(ob, d, N, L, t, K, E, b, nq, keys, seed):
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(seed)
    q = o.moduli[:L]
    db, masks = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N)
    evks = [rand_limbs(rng, q, (L, 2), N) for _ in range(nq if keys == "each" else 1)]
    queries = [(rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)) for _ in range(nq)]
    db.tofile(d / "db.bin")
    masks.tofile(d / "masks.bin")
    if keys != "none":
        for i, evk in enumerate(evks):
            evk.tofile(d / ("evk%d.bin" % i))
    for i, (idx, minus) in enumerate(queries):
        idx.tofile(d / ("idx%d.bin" % i))
        minus.tofile(d / ("minus%d.bin" % i))
    key_of = lambda slot: None if keys == "none" else evks[slot if keys == "each" else 0]
    return o, db, masks, queries, key_of


def _launch(built, G, root, N, L, t, K, E, b, nq, d, keys, set0, set1, mode=""):
    fake, exe = built
    procs = [subprocess.Popen([exe, fake, str(r), str(G), str(root), str(N), str(L), str(t), str(K), str(E), str(b), str(nq), str(d), keys,
                               set0, set1] + ([mode] if mode else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(G)]
    return wait_all(procs)


def _check_rounds(ob, case, d, settings):
    o, db, masks, queries, key_of = case
    b, nq, N = db.shape[1], len(queries), o.N
    for rnd, setting in enumerate(settings):
        ncomp, rl = (int(v) for v in (d / ("shape%d.txt" % rnd)).read_text().split())
        got = np.fromfile(d / ("out%d.bin" % rnd), dtype=np.uint64)
        assert got.size == b * nq * ncomp * rl * N, "round %d: %d words for rows [%d][%d][%d][%d][%d]" % (rnd, got.size, b, nq, ncomp, rl, N)
        got = got.reshape(b, nq, ncomp, rl, N)
        for i in range(nq):
            idx, minus = queries[(i + rnd) % nq]     # round 1 staged query (i + 1) % nq in place i, under place i's key
            want = exact_rows(ob, o, idx, minus, db, masks, key_of(i), setting)
            assert want.shape == (b, ncomp, rl, N), "round %d: rows %s, the definition's %s" % (rnd, got.shape, want.shape)
            assert (got[:, i] == want).all(), "round %d, query %d of the batch, setting %s" % (rnd, i, setting)


# (N, L, t, K, E, b, nq, G, root, keys, setting of round 0, setting of round 1); a setting: keep:relin:schedule, 0 = as ever
CASES = [
    (4096, 3, T16, 2, 3, 5, 1, 2, 0, "one", "1:1:0", "1:1:0"),         # keep = 1; 2 + 3 layers
    (4096, 3, T16, 2, 3, 5, 3, 2, 1, "one", "2:1:0", "2:1:0"),         # keep = 2, a batch of three, the root is rank 1
    (4096, 3, T16, 2, 3, 5, 1, 3, 0, "none", "0:0:0", "0:0:0"),        # degree-2 rows [3][L][N], 1 + 2 + 2 layers, NO key on any rank
    (4096, 3, T16, 2, 3, 5, 1, 3, 0, "none", "1:0:0", "1:0:0"),        # ... reduced to one limb
    (4096, 3, T16, 2, 3, 4, 3, 2, 0, "each", "0:1:2", "0:1:2"),        # chain limbs 2, every query of the batch under its own key
    (4096, 4, T16, 3, 3, 3, 1, 3, 0, "one", "2:1:4-3", "2:1:4-3"),     # K = 3: the schedule (4, 3), then keep = 2
    (16384, 4, T32, 2, 3, 2, 1, 2, 0, "one", "0:1:3", "1:1:3"),        # the folded ring, the fused drop: chain limbs 3, then keep = 1 below it
    (4096, 3, T16, 2, 3, 5, 1, 2, 0, "one", "1:1:0", "0:0:2"),         # changed between the rounds: keep = 1, then degree 2 on two limbs
]


@pytest.mark.parametrize("N,L,t,K,E,b,nq,G,root,keys,set0,set1", CASES)
def test_rows_of_every_setting_are_gathered(ob, built, tmp_path, N, L, t, K, E, b, nq, G, root, keys, set0, set1):
    case = _write_case(ob, tmp_path, N, L, t, K, E, b, nq, keys, 1000 * G + 10 * b + nq)
    outs = _launch(built, G, root, N, L, t, K, E, b, nq, tmp_path, keys, set0, set1)
    for r, (rc, so, se) in enumerate(outs):
        assert rc == 0, "rank %d: %s %s" % (r, so, se)
        assert "agree_rows -> 1" in so
    _check_rounds(ob, case, tmp_path, (set0, set1))


def test_ranks_with_different_settings(ob, built, tmp_path):
    """rank 2 of 3 keeps two limbs, the others one: nobody's rows are the agreed ones, because there are none"""
    N, L, t, K, E, b, nq = 4096, 3, T16, 2, 3, 5, 1
    _write_case(ob, tmp_path, N, L, t, K, E, b, nq, "one", 5)
    outs = _launch(built, 3, 0, N, L, t, K, E, b, nq, tmp_path, "one", "1:1:0", "2:1:0", "differ")
    for r, (rc, so, se) in enumerate(outs):
        assert rc == 0, "rank %d: %s %s" % (r, so, se)
        assert "agree_rows -> 0" in so and "gather -> -2" in so and "wait returned at once" in so, (r, so)   # -2: PIEHIP_ESTATE
    assert not (tmp_path / "out0.bin").exists()


def test_a_changed_setting_needs_a_new_agreement(ob, built, tmp_path):
    """a rank that touched a setting after agreeing -- even back to the agreed value -- is refused until the ranks agree again"""
    N, L, t, K, E, b, nq = 4096, 3, T16, 2, 3, 4, 1
    case = _write_case(ob, tmp_path, N, L, t, K, E, b, nq, "one", 6)
    outs = _launch(built, 2, 1, N, L, t, K, E, b, nq, tmp_path, "one", "1:1:0", "1:1:0", "stale")
    for r, (rc, so, se) in enumerate(outs):
        assert rc == 0, "rank %d: %s %s" % (r, so, se)
    _check_rounds(ob, case, tmp_path, ("1:1:0", "1:1:0"))


def test_default_rows_need_no_agreement(ob, built, tmp_path):
    N, L, t, K, E, b, nq = 4096, 3, T16, 2, 3, 5, 3
    case = _write_case(ob, tmp_path, N, L, t, K, E, b, nq, "one", 7)
    outs = _launch(built, 3, 2, N, L, t, K, E, b, nq, tmp_path, "one", "0:1:0", "0:1:0", "default")
    for r, (rc, so, se) in enumerate(outs):
        assert rc == 0, "rank %d: %s %s" % (r, so, se)
        assert "agree_rows" not in so
    assert (tmp_path / "shape0.txt").read_text().split() == ["2", str(L)]
    _check_rounds(ob, case, tmp_path, ("0:1:0", "0:1:0"))     # o.pie_run


def test_one_rank_over_rccl_keeps_one_limb(ob, pie_mod):
    """piehip_rccl_init / piehip_rccl_agree_rows / piehip_gather_results_host over the real RCCL with one rank, keep = 1: the form of
    tests/test_sharding_gpu.py::test_native_rccl_gather_one_rank"""
    pie = pie_mod
    N, L, t, K, E, b = 4096, 2, T16, 2, 4, 5
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(98)
    q = o.moduli[:L]
    db, masks, evk = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (L, 2), N)
    try:
        uid = pie.rccl_unique_id()
    except RuntimeError as e:
        if "RCCL" not in str(e):
            raise
        pytest.skip("RCCL does not load here: %s" % e)
    cc = pie.PieContext(N, L, t)
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    cc.rccl_init(uid, 1, 0)
    op.setResultLimbs(1)
    for nq in (1, 3):
        op.setQueryBatch(nq)
        with pytest.raises(RuntimeError, match="piehip_rccl_agree_rows"):
            op.gatherResultsHost(b)
        assert op.agreeRows(4000) is True
        queries = [(rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)) for _ in range(nq)]
        bufs = [op.hostBuffers(query=i) for i in range(nq)]
        for i, (idx, minus) in enumerate(queries):
            bufs[i][0][...] = idx
            bufs[i][1][...] = minus
            op.stageMinus(bufs[i][1], query=i)
            for h in range(K):
                op.stageIndexRow(h, bufs[i][0][h], query=i)
        op.broadcastQuery(0)
        op.run(sync=False)
        got = op.gatherResultsHost(b, root=0)
        op.sync()
        assert got.shape == ((b, 2, 1, N) if nq == 1 else (b, nq, 2, 1, N))
        for i, (idx, minus) in enumerate(queries):
            want = mod_reduce_exact(o, o.pie_run(idx, minus, db, masks, evk), 1)
            assert ((got if nq == 1 else got[:, i]) == want).all(), "query %d of %d" % (i, nq)
    op.setResultLimbs(L)      # back at the default shape: no agreement needed
    op.setQueryBatch(1)
    cc.rccl_destroy()
    cc.close()
