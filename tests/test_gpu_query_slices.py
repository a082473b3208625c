"""Query slices on the GPU (include/piehip.h "Query slices"): stage A sharded by inner hash function and limb over G handles of one
process -- all on the one device the tests see -- against the oracle and against one unsliced handle, bit for bit.

Every case builds a database, G sliced handles (unit ranges and bin ranges tile the units and the bin layers) and one unsliced
handle with the same arrays, and checks
  * each handle's acc_slice against the same limbs of the accumulators composed from the oracle's ct x pt and add;
  * the sliced results against o.pie_run on every word, and against piehip_run on the unsliced handle.
Shapes stay small; the sizes are the ones at which the code takes another path: N = 4096 (no lane order), 8192 (the 16-coefficient
transform: a batch's operand X is placed lane-ordered inside the QP operand array), 16384 (folded outer stage); E past one carry
sweep (COLACC_MAX_TERMS = 8) and past one full reduction (COLACC_MAX_TOTAL = 15; 40 passes two); odd bin counts on two queues; one
to five queries per run (query groups 1, 2, 3, 3 + 2); partitions with one unit each, a slice across two hash functions, empty unit
slices and empty bin slices; every instance of the sliced kernel at its reduction periods with worst-case residues (N = 1024).  At most
ten handles per process."""
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T16, T32, uniform_chain
from tests.test_gpu_parity import rand_limbs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _lib():
    from nested_hashing_psi_amd import _lib as l
    return l.lib()


def _acc_oracle(o, idx, minus, db):
    """acc[b][K][2][L][N] = sum_j idx[h][j] (.) db[h][beta][j] + minus (BatchedFHEHIPPIE.cpp:101-116) from the oracle's primitives"""
    K, b, E = db.shape[:3]
    out = np.zeros((b, K, 2, o.L, o.N), dtype=np.uint64)
    for beta in range(b):
        for h in range(K):
            s = o.mul_plain(idx[h, 0], db[h, beta, 0])
            for j in range(1, E):
                s = o.add(s, o.mul_plain(idx[h, j], db[h, beta, j]))
            out[beta, h] = o.add(s, minus)
    return out


def _case(ob, pie, N=4096, L=2, K=2, E=3, b=3, nq=1, G=2, unit_slices=None, bin_slices=None, streams=0, below=None, t=T32,
          extreme=False, keep=None, own_keys=False, rounds=1, put_order=None, set_order=None, seed=0):
    q, p = uniform_chain(N, L, below) if below else (None, None)
    o = ob.Oracle(N, L, t, q, p)
    rng = np.random.default_rng(1000 * N + 100 * L + 10 * K + E + b + nq + G + seed)
    db, masks = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N)
    keys = [rand_limbs(rng, o.q, (L, 2), N) for _ in range(nq if own_keys else 1)]
    if extreme:   # every residue at q - 1: the largest accumulators and products
        db[...] = (o.q - np.uint64(1))[:, None]
    ccs = [pie.PieContext(N, L, t, q, p) for _ in range(G)]
    ref_cc = pie.PieContext(N, L, t, q, p)
    assert G + 1 <= 10
    try:
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=db, preCalcRandomMask=masks, unitSlices=unit_slices, binSlices=bin_slices)
        ref = pie.BatchedFHEHIPPIE(ref_cc, vectorizedHCT=db, preCalcRandomMask=masks)
        if nq > 1:
            op.setQueryBatch(nq)
            ref.setQueryBatch(nq)
        for cc in ccs + [ref_cc]:
            if K > 1:
                cc.load_relin_key(keys[0])
                for i in range(nq if own_keys else 0):
                    cc.load_relin_key(keys[i], query=i)
            cc.set_run_streams(streams)
        if keep is not None:
            op.setResultLimbs(keep)
            ref.setResultLimbs(keep)
        for rnd in range(rounds):
            queries = [(rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)) for _ in range(nq)]
            if extreme:
                queries[0][0][...] = (o.q - np.uint64(1))[:, None]
                queries[0][1][...] = (o.q - np.uint64(1))[:, None]
            for i in (set_order if set_order is not None else range(nq)):
                op.setIndex(queries[i][0], query=i)
                op.setMinusCompareElement(queries[i][1], query=i)
                ref.setMinusCompareElement(queries[i][1], query=i)
                ref.setIndex(queries[i][0], query=i)
            # the facade's upload accounting, exact: a unit is limb l of the E index ciphertexts of one inner hash function -- 1 / (K L)
            # of the index matrix -- and limb l of the minus element, 1 / L of it (every inner hash function's sum ends with the
            # minus word, so that limb goes to each of the K units that share l: the minus element is 1 / (K E + 1) of a query)
            for g, (ul, uh) in enumerate(op.unitSlices):
                assert op.uploadedBytes()[g] * K * L == (uh - ul) * (K * E * 2 * L * N * 8 + K * 2 * L * N * 8)
                assert op.uploadedBytes()[g] == (uh - ul) * (E * 2 + 2) * N * 8
            op.run(putOrder=put_order)
            ref.run()
            got, unsliced = op.getResultList(), ref.getResultList()
            assert got.shape == unsliced.shape
            assert (got == unsliced).all(), "sliced evaluation differs from piehip_run on an unsliced handle"
            for i, (idx, minus) in enumerate(queries):
                acc = _acc_oracle(o, idx, minus, db)
                for g, (ul, uh) in enumerate(op.unitSlices):
                    sl = op.sliceAccumulators(g)    # [b][nq][u_n][2][N]
                    for u in range(ul, uh):
                        assert (sl[:, i, u - ul] == acc[:, u // L, :, u % L]).all(), (g, u, i)
                if keep is None:
                    want = o.pie_run(idx, minus, db, masks, keys[i if own_keys else 0])
                    assert ((got if nq == 1 else got[i]) == want).all(), (rnd, i)
        return op
    finally:
        for cc in ccs + [ref_cc]:
            cc.close()


# ---- rings --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,K,E,b,nq,G", [
    (4096, 2, 2, 3, 3, 1, 2),     # no lane order
    (4096, 2, 2, 3, 3, 3, 2),
    (8192, 2, 2, 3, 3, 3, 2),     # the smallest ring with the 16-coefficient transform: X placed lane-ordered (a batch)
    (8192, 2, 2, 3, 3, 1, 4),     # ... one query: X through the inverse transform's copy
    (8192, 3, 3, 2, 2, 2, 3),     # ... K = 3: only inner hash function 0 is placed there
    (16384, 2, 2, 3, 2, 2, 2),    # folded outer stage
    (16384, 2, 2, 3, 2, 1, 3),
])
def test_rings(ob, pie, N, L, K, E, b, nq, G):
    _case(ob, pie, N=N, L=L, K=K, E=E, b=b, nq=nq, G=G)


# ---- shapes at N = 4096 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 4])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_limbs_and_hash_functions(ob, pie, L, K):
    """K = 1 goes through piehip_load_db_sliced (the hashing variants refuse it) and needs no key"""
    _case(ob, pie, L=L, K=K, E=3, b=2, nq=2 if K == 2 else 1, G=3)


@pytest.mark.parametrize("E", [1, 3, 17, 40])
def test_sum_lengths(ob, pie, E):
    """past one carry sweep (8 terms) and past one full reduction (15; 40 is past two), for one query and for a group of two"""
    _case(ob, pie, E=E, b=2, nq=1, G=2)
    _case(ob, pie, E=E, b=2, nq=2, G=2, seed=1)


@pytest.mark.parametrize("b", [1, 5, 9])
@pytest.mark.parametrize("streams", [1, 2])
def test_bin_counts_on_one_and_two_queues(ob, pie, b, streams):
    """odd shares on two queues; ragged layer groups of the sliced stage A (five layers: 3 + 2 for three queries)"""
    _case(ob, pie, E=3, b=b, nq=3, G=1, streams=streams)
    _case(ob, pie, E=3, b=b, nq=1, G=2, streams=streams, seed=2)


@pytest.mark.parametrize("nq", [1, 2, 3, 5])
def test_batch_sizes(ob, pie, nq):
    """query groups of one, two, three, and three + two"""
    _case(ob, pie, E=3, b=4, nq=nq, G=2)


def test_61_bit_chain(ob, pie):
    """a caller-supplied chain of 61-bit primes: not small_moduli, the 128-bit accumulators; E = 40 passes their 32-term reduction"""
    _case(ob, pie, E=40, b=2, nq=1, G=2, below=1 << 61)
    _case(ob, pie, E=3, b=3, nq=3, G=3, below=1 << 61, seed=3)


@pytest.mark.parametrize("N,nq", [(4096, 1), (8192, 2)])
def test_worst_case_residues(ob, pie, N, nq):
    """q - 1 everywhere in the database and in the first query, over 17 terms"""
    _case(ob, pie, N=N, E=17, b=2, nq=nq, G=2, extreme=True)


# ---- the reduction periods, in every instance of the sliced kernel ---------------------------------------------------------------
# (arithmetic, E, nq, b, instance reached).  The sliced launcher takes one query group per run (nq <= 4: one group of nq) and, by
# the layer rule (stage_a_common.h: stage_a_layers under stage_a_layer_cap), exactly b layers per thread for every b up to the cap
# of (nq, arithmetic): each case launches stage_a_slice_kernel<BPT = b, Q = nq, DEPTH, MAD> and no other instance, 17 with column
# accumulators and 15 with 128-bit ones.  E = 120: both column-accumulator periods line up, the epilogue gets 8 uncarried and 15
# unreduced terms; E = 65: past two 32-term reductions of the 128-bit accumulators.  Every database and first-query word is q - 1.
PERIOD_CASES = ([("mad", 120, nq, b, "slice<%d, %d, %d, mad>" % (b, nq, depth))
                 for nq, cap in ((1, 7), (2, 4), (3, 3), (4, 3)) for b in range(1, cap + 1)
                 for depth in [(3 if b == 7 else 4) if nq == 1 else 2 if nq == 4 or nq * b >= 9 else 3]] +
                [("u128", 65, nq, b, "slice<%d, %d, %d, 128-bit>" % (b, nq, depth))
                 for nq, cap in ((1, 5), (2, 4), (3, 3), (4, 3)) for b in range(1, cap + 1)
                 for depth in [4 if nq == 1 else 2 if nq == 4 or nq * b >= 9 else 3]])
assert len(PERIOD_CASES) == 17 + 15


@pytest.mark.parametrize("arith,E,nq,b,kernel", PERIOD_CASES, ids=["%s-E%d-nq%d-b%d" % c[:4] for c in PERIOD_CASES])
def test_periods_in_every_slice_instance(ob, pie, arith, E, nq, b, kernel):
    _case(ob, pie, N=1024, L=2, K=2, E=E, b=b, nq=nq, G=2, extreme=True, below=None if arith == "mad" else 1 << 61)


# ---- partitions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,L,G,b,nq", [
    (2, 2, 1, 3, 2),     # one handle: both sides whole
    (2, 2, 4, 5, 2),     # G = K L: one unit each; five layers over four handles
    (2, 4, 3, 4, 1),     # K L = 8 over three: 2 + 3 + 3, the middle slice spans two hash functions
    (2, 2, 6, 3, 2),     # G = K L + 2: empty unit slices, and b < G: handles without a chain side
    (3, 2, 8, 2, 1),     # both kinds of empty handle at once
])
def test_partitions(ob, pie, K, L, G, b, nq):
    op = _case(ob, pie, K=K, L=L, E=3, b=b, nq=nq, G=G)
    assert [hi - lo for lo, hi in op.unitSlices].count(0) == max(0, G - K * L)


def test_uneven_slices_of_the_callers_choice(ob, pie):
    """unit slices and bin slices that do not line up: a handle with units and no bins, one with bins and no units"""
    _case(ob, pie, N=8192, K=2, L=2, E=3, b=5, nq=2, G=3, unit_slices=[(0, 3), (3, 4), (4, 4)], bin_slices=[(0, 0), (0, 1), (1, 5)])


# ---- what the chain carries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nq", [(4096, 1), (8192, 3)])
def test_result_limbs_through_run_chain(ob, pie, N, nq):
    """piehip_set_result_limbs(1): run_chain hands out the unsliced handle's reduced rows"""
    _case(ob, pie, N=N, E=3, b=3, nq=nq, G=2, keep=1)


@pytest.mark.parametrize("streams", [1, 2])
def test_per_query_keys(ob, pie, streams):
    _case(ob, pie, N=8192, E=3, b=3, nq=3, G=2, own_keys=True, streams=streams)


# ---- order independence ---------------------------------------------------------------------------------------------------------
def test_puts_and_queries_in_any_order_and_two_rounds(ob, pie):
    G = 3
    order = [(d, s) for s in reversed(range(G)) for d in (1, 0, 2)]
    _case(ob, pie, N=8192, K=2, L=2, E=3, b=4, nq=3, G=G, put_order=order, set_order=[2, 0, 1], rounds=2)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ob, pie):
    """every refusal returns its code and a message and leaves the handle usable: the round completes afterwards"""
    EINVAL, ESTATE = -1, -2
    N, L, K, E, b, t = 4096, 2, 2, 2, 2, T32
    lib = _lib()
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(5)
    db, masks, evk = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
    idx, minus = rand_limbs(rng, o.q, (K, E, 2), N), rand_limbs(rng, o.q, (2,), N)
    ccs = [pie.PieContext(N, L, t) for _ in range(2)]
    plain = pie.PieContext(N, L, t)
    u64p = C.POINTER(C.c_uint64)

    def refused(rc, code):
        assert rc == code and lib.piehip_last_error().decode()

    try:
        h0, h1 = ccs[0]._h, ccs[1]._h
        pts = np.ascontiguousarray(np.stack([db[u // L, :, :, u % L] for u in range(K * L)]))
        pp, mp = pts.ctypes.data_as(u64p), masks.ctypes.data_as(u64p)
        # ranges outside K L or b, and reversed ones
        refused(lib.piehip_load_db_sliced(h0, K, b, E, 0, K * L + 1, pp, 0, b, mp), EINVAL)
        refused(lib.piehip_load_db_sliced(h0, K, b, E, 3, 2, pp, 0, b, mp), EINVAL)
        refused(lib.piehip_load_db_sliced(h0, K, b, E, 0, 2, pp, 0, b + 1, mp), EINVAL)
        refused(lib.piehip_load_db_sliced(h0, K, b, E, 0, 2, pp, 2, 1, mp), EINVAL)
        # the hashing variant refuses one inner hash function
        tbl = np.ones((2, 2, 1, b, E), dtype=np.uint64)
        refused(lib.piehip_load_db_table_sliced(h0, tbl.ctypes.data_as(u64p), 2, 2, 1, b, E, 1, 2, 0, 1, 0, b), EINVAL)
        # the slice calls on an unsliced handle
        refused(lib.piehip_run_slice(plain._h), ESTATE)
        refused(lib.piehip_run_chain(plain._h), ESTATE)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=db, preCalcRandomMask=masks)
        for cc in ccs:
            cc.load_relin_key(evk)
        refused(lib.piehip_run_slice(h0), ESTATE)                 # no slice inputs yet
        refused(lib.piehip_run(h0), ESTATE)                       # a handle that holds only a slice
        refused(lib.piehip_set_graph(h0, 1), ESTATE)
        ref = pie.BatchedFHEHIPPIE(plain, vectorizedHCT=db, preCalcRandomMask=masks)
        refused(lib.piehip_attach_database(h0, plain._h), ESTATE)
        refused(lib.piehip_attach_database(plain._h, h0), ESTATE)
        op.setIndex(idx)
        op.setMinusCompareElement(minus)
        for cc in ccs:
            assert lib.piehip_run_slice(cc._h) == 0
        refused(lib.piehip_run_chain(h0), ESTATE)                 # nothing put
        assert lib.piehip_put_accumulators_from(h0, h0) == 0
        refused(lib.piehip_put_accumulators_from(h0, h0), ESTATE)  # the same units twice in one round
        refused(lib.piehip_run_chain(h0), ESTATE)                 # half of the units put
        src = C.c_void_p()
        assert lib.piehip_slice_accumulators_device(h1, C.byref(src)) == 0 and src.value
        refused(lib.piehip_put_accumulators(h0, 1, 3, src), ESTATE)   # overlaps what has been put
        refused(lib.piehip_put_accumulators(h0, 3, 2, src), EINVAL)
        refused(lib.piehip_put_accumulators(h0, 2, K * L + 1, src), EINVAL)
        assert lib.piehip_sync(h1) == 0                            # piehip_put_accumulators: the caller orders the writer
        assert lib.piehip_put_accumulators(h0, 2, 4, src) == 0
        for s in (0, 1):
            assert lib.piehip_put_accumulators_from(h1, ccs[s]._h) == 0
        for cc in ccs:
            assert lib.piehip_run_chain(cc._h) == 0
        refused(lib.piehip_run_chain(h0), ESTATE)                 # a new round: nothing put since the last run_chain
        want = o.pie_run(idx, minus, db, masks, evk)
        assert (op.getResultList() == want).all()
        # a change of the batch size starts a new round as well
        assert lib.piehip_put_accumulators_from(h0, h0) == 0
        op.setQueryBatch(2)
        refused(lib.piehip_run_slice(h0), ESTATE)                 # query 1 has no inputs
        for i in range(2):
            op.setIndex(idx, query=i)
            op.setMinusCompareElement(minus, query=i)
        op.run()
        got = op.getResultList()
        assert (got[0] == want).all() and (got[1] == want).all()
        # loading a whole database makes the handle an unsliced one again
        ref2 = pie.BatchedFHEHIPPIE(ccs[0], vectorizedHCT=db, preCalcRandomMask=masks)
        refused(lib.piehip_run_slice(h0), ESTATE)
        ref2.setQueryBatch(1)
        ref2.setIndex(idx)
        ref2.setMinusCompareElement(minus)
        ref2.run()
        assert (ref2.getResultList() == want).all()
        del ref
    finally:
        for cc in ccs + [plain]:
            cc.close()


# ---- decrypted semantics, through the table form ------------------------------------------------------------------------------
def test_kat0_shape_decrypts_to_the_intersection(ob, pie):
    """the KAT-0 shape (TestBatchedFHEPIE.cpp:89-94) through piehip_load_db_table_sliced on three handles: the table is shuffled whole,
    every handle encodes its units only -- the ciphertexts equal the oracle's on the table it shuffles with the same seed and those of
    an unsliced piehip_load_db_table handle, and they decrypt to exactly the expected match, and to none for an absent element"""
    N, L, t, k, e, K, E, b = 4096, 2, T16, 2, 1, 2, 10, 20
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(77)
    sk = o.keygen(11)
    evk = o.relin_keygen(sk, 12)
    from tests.test_oracle_pie import distinct_items
    universe = distinct_items(rng, o.t, 101)
    server, absent = universe[:100].copy(), universe[100:]
    tab = ob.Tabulation(987654321, k + K)
    tbl = ob.hct_build(tab, server, k, e, K, b, E, evict_seed=1)
    ccs = [pie.PieContext(N, L, t) for _ in range(3)]
    ref_cc = pie.PieContext(N, L, t)
    try:
        for cc in ccs + [ref_cc]:
            cc.load_relin_key(evk)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, hashTable=tbl, shuffle_seed=2, mask_seed=3)
        ref = pie.BatchedFHEHIPPIE(ref_cc, hashTable=tbl, shuffle_seed=2, mask_seed=3)
        shuffled = tbl.copy()
        ob.hct_shuffle_bins(shuffled, 2)
        slots, mk = ob.pack_db(shuffled), ob.masks(t, b, k * e, 3)
        db = np.stack([o.encode_eval(slots[h, bn, j]) for h in range(K) for bn in range(b) for j in range(E)]).reshape(K, b, E, L, N)
        masks = np.stack([o.encode_eval(mk[bn]) for bn in range(b)])
        for client, expect in ((server[:1], [int(server[0])]), (absent, [])):
            ctab = ob.client_build(tab, client, k, e, evict_seed=4)
            index, minus_v = ob.client_vectors(tab, ctab, K, E)
            idx = np.stack([o.encrypt_slots(sk, index[h, j], 100 + h * E + j) for h in range(K) for j in range(E)]).reshape(K, E, 2, L, N)
            minus = o.encrypt_slots(sk, minus_v, 99)
            op.setIndex(idx)
            op.setMinusCompareElement(minus)
            op.run()
            got = op.getResultList()
            ref.setIndex(idx)
            ref.setMinusCompareElement(minus)
            ref.run()
            assert (got == ref.getResultList()).all()
            assert (got == o.pie_run(idx, minus, db, masks, evk)).all()
            dec = np.stack([o.decrypt_slots(sk, got[bn], k * e)[0] for bn in range(b)])
            assert sorted(int(v) for v in ob.client_scan(ctab, dec)) == expect
    finally:
        for cc in ccs + [ref_cc]:
            cc.close()
