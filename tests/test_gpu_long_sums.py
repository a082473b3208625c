"""Stage A over long index sums (reference BatchedFHEHIPPIE.cpp:101-116): sum_j idx[h][j] * db[h][bin][j] + minus.

Stage A of a whole query on one handle (kernels_stage_a.hip): a batch goes through stage_a_tiled_kernel<BPT, Q, DEPTH, MAD> in groups of
Q = 2..4 queries (BPT bin layers per thread, DEPTH terms in flight; three queries on a ring that fills the chip through the resident
kernel: tests/test_gpu_stage_a_resident.py), one query through stage_a_mad_kernel<BPT> (four terms in flight) or, on the wide
arithmetic, stage_a_kernel<BPT> (none), with a divisor of b layers per thread or groups of seven / eight and a remainder launch
(launch_stage_a_one).  The tiled kernel's term loop is stage_a_terms of stage_a_common.h, which the sliced kernel shares
(tests/test_gpu_query_slices.py runs that one at the periods).  All accumulate lazily and reduce on a fixed period, in one of two
arithmetics, each bound resting on a hand proof (stage_a_common.h, madasm.h):
  mad    every modulus in (2^59, 2^60): 30-bit column accumulators, a carry sweep after every COLACC_MAX_TERMS = 8 terms (16
         products < 2^60 in column 1), a mid-sum reduction after every COLACC_MAX_TOTAL = 15 (the top column: 15 products, a value
         below 2^124), colacc_reduce<true> in the epilogue
  wide   every other chain: 128-bit accumulators reduced after every 32 terms (32 * 2^122 + 2^61 < 2^128 for q < 2^61)
Random residues cannot reach these bounds (a random 60-bit word has a high half near 2^29: a window twice as long as the
proof allows still does not wrap), so the index and database words here are every one q - 1, or distinct and uniform in
[q - 2^24, q): the columns as full as the moduli allow, data that still tells lanes, layers and queries apart.  E runs
across the periods (31..33, 63..65, 119..121 where both MAD periods line up and E = 120 hands the epilogue 8 uncarried and
15 unreduced terms at once, 148, 240, 581; 1 and 2, sums shorter than the ring of terms in flight) and b / nq pick every template
instantiation (the `kernels` column, from the launcher rules: launch_stage_a_one in kernels_stage_a.hip; for batches, stage_a_query_group / stage_a_layers / stage_a_depth in
stage_a_common.h).  Every result is compared bit for bit with the oracle's run() (oracle/pie_oracle.c: one mulmod + addmod per
term, independent of the GPU's lazy scheme); K = 2, so stage A feeds the whole product chain.

test_reference_long_rows runs rows of the reference's parameter table with E > 56 (Performance-Evaluation/Parameters1.txt)
end to end through the hashing harness: device offline phase, encryption, run(), decryption, scan.
"""
import numpy as np
import pytest

from tests.param_chains import T32, named_chain, uniform_chain
from tests.test_gpu_fullsize import run_case
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu

L = 3
CHAINS = {
    "d60": None,                 # the default chain: the largest primes below 2^60, q - 1 has both 30-bit halves near 2^30 - 1
    "barrett_edges": "barrett_edges",   # Q_0 just above 2^59 (mu = floor(2^123 / q) near 2^64), the rest below 2^60
    "u61": 1 << 61,              # 61-bit: the wide arithmetic, 32 (q - 1)^2 near 2^127
    "u50": 1 << 50,              # 50-bit: the wide arithmetic far from its bound
}

# (chain, N, E, b, nq, pattern, queue counts, instantiations reached).  Patterns: rand (uniform), max (every word q - 1), near
# (uniform in [q - 2^24, q)) for the index and database words; minus, masks and key are random.  One queue keeps all b layers in
# one launcher call; with 0 (the default: two queues from b = 8) the layers split 4/7 : 3/7 (run_group_size).
# Instantiations of the tiled kernel are written <arithmetic> <BPT, Q, DEPTH>; "ragged" = a last layer group shorter than BPT.
CASES = [
    # 128-bit accumulator, 61-bit chain: overflows after 65 unreduced near-max terms
    ("u61", 1024, 31, 1, 1, "near", (1,), "wide stage_a_kernel<1>"),
    ("u61", 1024, 32, 2, 1, "max", (1,), "wide stage_a_kernel<2>"),
    ("u61", 1024, 33, 3, 1, "near", (1,), "wide stage_a_kernel<3>"),
    ("u61", 1024, 63, 4, 1, "rand", (1,), "wide stage_a_kernel<4>"),
    ("u61", 1024, 64, 5, 1, "near", (1,), "wide stage_a_kernel<5>"),
    ("u61", 2048, 65, 6, 1, "near", (1,), "wide stage_a_kernel<6>"),
    ("u61", 1024, 119, 7, 1, "max", (1,), "wide stage_a_kernel<7>"),
    ("u61", 1024, 120, 8, 1, "near", (1, 0), "wide stage_a_kernel<8>; two queues: <5> + <3>"),
    ("u61", 1024, 121, 17, 1, "near", (1,), "wide stage_a_kernel<8> + <1> (16 + 1)"),
    ("u61", 1024, 148, 3, 2, "near", (1, 0), "wide <3, 2, 3>"),
    ("u61", 1024, 240, 17, 3, "near", (1, 0), "wide <3, 3, 2> ragged (5 x 3 + 2); two queues: 10 and 7 layers, <3, 3, 2> ragged both"),
    ("u61", 1024, 581, 2, 1, "near", (1,), "wide stage_a_kernel<2>"),
    ("u61", 1024, 581, 1, 1, "max", (1,), "wide stage_a_kernel<1>"),
    # 128-bit accumulator, 50-bit chain
    ("u50", 1024, 64, 8, 1, "near", (1,), "wide stage_a_kernel<8>"),
    ("u50", 1024, 121, 17, 1, "near", (1,), "wide stage_a_kernel<8> + <1>"),
    ("u50", 1024, 240, 5, 2, "near", (1, 0), "wide <3, 2, 3> ragged (3 + 2)"),
    ("u50", 1024, 581, 2, 1, "near", (1,), "wide stage_a_kernel<2>"),
    # 128-bit accumulator, query groups: two reductions (terms 32 and 64) and one more term; q0 > 0 in the row index
    ("u61", 1024, 65, 5, 4, "near", (1, 0), "wide <3, 4, 2> ragged (3 + 2)"),
    ("u61", 1024, 32, 7, 5, "max", (1,), "wide queries 3 + 2: <3, 3, 2> ragged (3 + 3 + 1), <4, 2, 3> ragged (4 + 3)"),
    ("u50", 1024, 33, 2, 7, "near", (1,), "wide queries 4 + 3: <2, 4, 2>, <2, 3, 3>"),
    # column accumulators, one query
    ("d60", 1024, 31, 1, 1, "near", (1,), "mad stage_a_mad_kernel<1>"),
    ("d60", 1024, 32, 2, 1, "max", (1,), "mad stage_a_mad_kernel<2>"),
    ("d60", 1024, 33, 3, 1, "near", (1,), "mad stage_a_mad_kernel<3>"),
    ("d60", 1024, 63, 4, 1, "near", (1,), "mad stage_a_mad_kernel<4>"),
    ("d60", 1024, 64, 5, 1, "rand", (1,), "mad stage_a_mad_kernel<5>"),
    ("d60", 2048, 65, 6, 1, "near", (1,), "mad stage_a_mad_kernel<6>"),
    ("d60", 1024, 119, 7, 1, "near", (1,), "mad stage_a_mad_kernel<7>"),
    ("d60", 1024, 120, 9, 1, "near", (1, 0), "mad stage_a_mad_kernel<7> + <2> (7 + 2); two queues: <5> and <4>"),
    ("d60", 1024, 121, 17, 1, "near", (1,), "mad stage_a_mad_kernel<7> + <3> (14 + 3)"),
    ("d60", 1024, 148, 8, 1, "max", (1, 0), "mad stage_a_mad_kernel<4> (b = 8); two queues: <5> and <3>"),
    ("d60", 1024, 240, 3, 1, "near", (1,), "mad stage_a_mad_kernel<3>"),
    ("d60", 1024, 581, 2, 1, "near", (1,), "mad stage_a_mad_kernel<2>"),
    # a sum shorter than the ring of terms in flight: the prologue's d < E guards, the j + d < E guards of the first unrolled round
    ("d60", 1024, 1, 7, 1, "near", (1,), "mad stage_a_mad_kernel<7>"),
    ("d60", 1024, 2, 4, 1, "near", (1,), "mad stage_a_mad_kernel<4>"),
    ("u61", 1024, 1, 5, 1, "near", (1,), "wide stage_a_kernel<5> (no ring there: one term)"),
    ("u61", 1024, 1, 5, 2, "near", (1,), "wide <3, 2, 3> ragged (3 + 2)"),
    ("d60", 1024, 2, 5, 2, "near", (1,), "mad <3, 2, 3> ragged (3 + 2)"),
    # column accumulators, query batches (one launch per group of 2..4 queries)
    ("d60", 1024, 120, 4, 2, "near", (1, 0), "mad <4, 2, 3>"),
    ("d60", 1024, 121, 5, 2, "near", (1, 0), "mad <3, 2, 3> ragged (3 + 2)"),
    ("d60", 1024, 119, 3, 3, "near", (1, 0), "mad <3, 3, 2>"),
    ("d60", 1024, 65, 2, 3, "near", (1, 0), "mad <2, 3, 3>"),
    ("d60", 1024, 148, 5, 4, "near", (1, 0), "mad <3, 4, 2> ragged (3 + 2)"),
    ("d60", 1024, 240, 7, 5, "near", (1, 0), "mad queries 3 + 2: <3, 3, 2> ragged (3 + 3 + 1), <4, 2, 3> ragged (4 + 3)"),
    ("d60", 1024, 63, 9, 3, "near", (1, 0), "mad <3, 3, 2>; two queues: 5 layers <3, 3, 2> ragged, 4 layers <2, 3, 3>"),
    ("d60", 1024, 581, 1, 2, "near", (1, 0), "mad <1, 2, 3>"),
    ("d60", 1024, 64, 3, 4, "max", (1, 0), "mad <3, 4, 2>"),
    # column accumulators at the edges of the one-word Barrett
    ("barrett_edges", 1024, 120, 7, 1, "near", (1,), "mad stage_a_mad_kernel<7>"),
    ("barrett_edges", 1024, 33, 17, 1, "max", (1, 0), "mad stage_a_mad_kernel<7> + <3>; two queues: <5> and <7>"),
    ("barrett_edges", 1024, 240, 9, 3, "near", (1, 0), "mad <3, 3, 2>; two queues: <3, 3, 2> ragged, <2, 3, 3>"),
    ("barrett_edges", 1024, 64, 3, 4, "near", (1, 0), "mad <3, 4, 2>"),
    ("barrett_edges", 1024, 581, 1, 1, "near", (1,), "mad stage_a_mad_kernel<1>"),
]


def _case_id(c):
    chain, N, E, b, nq, pattern = c[:6]
    return "%s-N%d-E%d-b%d-nq%d-%s" % (chain, N, E, b, nq, pattern)


@pytest.fixture(scope="module")
def contexts(ob):
    """one (oracle, GPU context) pair per (chain, N), shared by the cases of the module"""
    from nested_hashing_psi_amd import pie
    made = {}

    def get(chain, N):
        if (chain, N) not in made:
            spec = CHAINS[chain]
            q, p = (None, None) if spec is None else (uniform_chain(N, L, spec) if isinstance(spec, int) else named_chain(N, L, spec))
            o = ob.Oracle(N, L, T32, q, p)
            cc = pie.PieContext(N, L, T32, q, p)
            assert (cc.moduli == o.moduli).all()
            made[(chain, N)] = (o, cc)
        return made[(chain, N)]
    yield pie, get
    for _, cc in made.values():
        cc.close()


def words(rng, q, shape, N, pattern):
    """index / database words [*shape][L][N] of one residue pattern"""
    if pattern == "rand":
        return rand_limbs(rng, q, shape, N)
    out = np.empty(tuple(shape) + (len(q), N), dtype=np.uint64)
    for i, m in enumerate(q):
        top = np.uint64(int(m) - 1)
        out[..., i, :] = top if pattern == "max" else top - rng.integers(0, 1 << 24, tuple(shape) + (N,), dtype=np.uint64)
    return out


@pytest.mark.parametrize("chain,N,E,b,nq,pattern,streams,kernels", CASES, ids=[_case_id(c) for c in CASES])
def test_stage_a_long_sum(contexts, chain, N, E, b, nq, pattern, streams, kernels):
    pie, get = contexts
    o, cc = get(chain, N)
    K, q = 2, o.q
    small = all((int(m) >> 59) == 1 for m in o.moduli[:2 * L + 1])
    assert small == kernels.startswith("mad"), "the chain does not reach the kernels named"
    rng = np.random.default_rng(E * 1000 + b * 10 + nq)
    db, masks, evk = words(rng, q, (K, b, E), N, pattern), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (L, 2), N)
    queries = [(words(rng, q, (K, E, 2), N, pattern), rand_limbs(rng, q, (2,), N)) for _ in range(nq)]
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    op.setQueryBatch(nq)
    try:
        for i, (idx, minus) in enumerate(queries):
            op.setIndex(idx, query=i)
            op.setMinusCompareElement(minus, query=i)
        want = [o.pie_run(idx, minus, db, masks, evk) for idx, minus in queries]
        for s in streams:
            cc.set_run_streams(s)
            op.run()
            got = op.getResultList()
            if nq == 1:
                got = got[None]
            assert got.shape == (nq, b, 2, L, N)
            for i in range(nq):
                bad = [bn for bn in range(b) if not (got[i, bn] == want[i][bn]).all()]
                assert not bad, "%s, run_streams %d, query %d: bin layers %s differ from the oracle" % (kernels, s, i, bad)
    finally:
        op.setQueryBatch(1)
        cc.set_run_streams(0)


# Rows of Parameters1.txt with E > 56 (|C|, |S|, k, e, b, E), at the depth client.select_parameters picks (3 below E = 500: L = 4;
# 5 from there: L = 6) and the smallest ring the row's batch k e fits into, except row 41 at its full shape.
@pytest.mark.parametrize("N,L_,nS,nC,k,e,E,b,layers,what", [
    (16384, 4, 1 << 24, 1 << 10, 2, 4949, 66, 33, range(0, 33, 4),
     "Parameters1.txt:41 at full shape: 4 356 plaintexts (2.3 GB) hashed and encoded on the device; 9 of 33 layers compared"),
    (1024, 4, 1 << 24, 32, 2, 442, 148, 148, range(148),
     "Parameters1.txt:14: K b E = 43 808 words per table row, beyond the LDS table: the global cuckoo_build_kernel with b > 64"),
    (64, 4, 1 << 20, 32, 3, 14, 206, 206, range(206),
     "Parameters1.txt:56: K b E = 84 872 plaintexts, gather_slots_kernel with grid.y above 65 535"),
    (1024, 6, 1 << 16, 32, 2, 442, 581, 5, range(5),
     "Parameters1.txt:20 (k, e, E) with b = 5 and |S| = 2^16 instead of 2^28: E = 581 through the whole pipeline"),
], ids=["row41-E66", "row14-E148", "row56-E206", "row20-E581"])
def test_reference_long_rows(ob, pie_mod, N, L_, nS, nC, k, e, E, b, layers, what):
    """device offline phase, client encryption, run(), decryption, scan: bit for bit with the oracle on the compared layers, a
    positive noise budget in every result and exactly the intersection (run_case of test_gpu_fullsize.py)"""
    assert run_case(ob, pie_mod, N, L_, T32, nS, nC, k, e, 2, E, b, E * 7 + b, layers) > 0
