"""Stage A of a query batch with the index words resident in registers (stage_a_resident_kernel of kernels_stage_a.hip).

launch_stage_a_batch sends a group of three queries to that kernel where stage_a_resident_lpp (stage_a_common.h) says so: E = 14 or
E = 12 (the two instantiations), more layers than one tiled group holds (b > 3), and at least STAGE_A_RESIDENT_MIN_THREADS = 65 536
coefficients N L K in the launch.  Every other launch stays on the tiled kernel (stage_a_tiled_kernel), so the cases sit on both
sides of each condition and mix the two kernels in one run():
  E       1, 7, 8, 9 and 15 are tiled (no instantiation; 15 is past what a thread's registers hold), 12 and 14 resident -- both
          cross the kernel's one carry sweep (after term 8), and every word q - 1 overflows column 1 at once if the sweep is lost
  b       4 and 5: the smallest launches above one tiled group; 9 and 14 split 5 + 4 and 8 + 6 over two queues (run_streams 0)
  nq      5 = resident(3) + tiled(2), 6 = resident + resident, 7 = tiled(4) + resident(3): rows [layer][query] with q0 > 0
  N       L = 3 throughout.  1024 and 8192 with K = 2 are 6 144 and 49 152 coefficients: under the threshold the microbenchmark
          set, these run the tiled kernel and pin the rule's other side.  16384 (98 304), 8192 with K = 3 (73 728) and 32768 with
          K = 1 (98 304) are the smallest rings of the suite that reach the resident kernel; from 8192 on the plan lets stage A
          write operand X lane-ordered (plan.x_direct), the only place the lane-ordered stores of either kernel run
  K       1: the accumulators go straight into the mask multiply; 3: h = 1, 2 to acc and h = 0 to X
Words are `near` (distinct, uniform in [q - 2^24, q): tells lanes, layers and queries apart with the columns nearly full) or `max`
(every word q - 1).  Every result is compared bit for bit with the oracle's run(), as in tests/test_gpu_long_sums.py.
"""
import numpy as np
import pytest

from tests.test_gpu_long_sums import contexts, words  # noqa: F401  (contexts is the module's fixture)
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu


def _cases():
    out = []
    for chain in ("d60", "barrett_edges"):
        for E in (1, 7, 8, 9, 12, 14, 15):
            for b in (4, 5, 9, 14):
                out.append((chain, 1024, 2, E, b, 3, "near"))
        for E in (8, 12, 14):
            for b in (5, 14):
                out.append((chain, 1024, 2, E, b, 3, "max"))
    for nq in (5, 6, 7):
        out.append(("d60", 1024, 2, 14, 5, nq, "near"))
    out.append(("barrett_edges", 1024, 2, 14, 5, 7, "max"))
    for b in (5, 9):
        out.append(("d60", 8192, 2, 14, b, 3, "near"))
    for K in (1, 3):
        out.append(("d60", 1024, K, 14, 5, 3, "near"))
    # at and above the thread threshold: the resident kernel
    for E in (12, 14):
        for b in (4, 5, 9, 14):
            out.append(("d60", 16384, 2, E, b, 3, "near"))
        for chain in ("d60", "barrett_edges"):
            out.append((chain, 16384, 2, E, 5, 3, "max"))
        out.append(("barrett_edges", 16384, 2, E, 9, 3, "near"))
    for nq in (5, 6, 7):
        out.append(("d60", 16384, 2, 14, 5, nq, "near"))
    out.append(("barrett_edges", 16384, 2, 14, 4, 7, "max"))
    out.append(("d60", 8192, 3, 14, 5, 3, "near"))
    out.append(("barrett_edges", 8192, 3, 12, 9, 3, "near"))
    out.append(("d60", 32768, 1, 14, 5, 3, "near"))
    return out


CASES = _cases()


@pytest.mark.parametrize("chain,N,K,E,b,nq,pattern", CASES, ids=["%s-N%d-K%d-E%d-b%d-nq%d-%s" % c for c in CASES])
def test_stage_a_resident(contexts, chain, N, K, E, b, nq, pattern):  # noqa: F811
    pie, get = contexts
    o, cc = get(chain, N)
    q = o.q
    assert all((int(m) >> 59) == 1 for m in o.moduli[:2 * 3 + 1]), "the chain does not reach the column-accumulator kernels"
    rng = np.random.default_rng(((N * 4 + K) * 16 + E) * 64 + b * 8 + nq)
    db, masks, evk = words(rng, q, (K, b, E), N, pattern), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (3, 2), N)
    queries = [(words(rng, q, (K, E, 2), N, pattern), rand_limbs(rng, q, (2,), N)) for _ in range(nq)]
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    op.setQueryBatch(nq)
    try:
        for i, (idx, minus) in enumerate(queries):
            op.setIndex(idx, query=i)
            op.setMinusCompareElement(minus, query=i)
        want = [o.pie_run(idx, minus, db, masks, evk) for idx, minus in queries]
        for s in (1, 0):
            cc.set_run_streams(s)
            op.run()
            got = op.getResultList()
            assert got.shape == (nq, b, 2, 3, N)
            for i in range(nq):
                bad = [bn for bn in range(b) if not (got[i, bn] == want[i][bn]).all()]
                assert not bad, "run_streams %d, query %d: bin layers %s differ from the oracle" % (s, i, bad)
    finally:
        op.setQueryBatch(1)
        cc.set_run_streams(0)
