"""Seeded query slices on the GPU (include/piehip.h "Query slices", the piehip_set_*_slice_seeded*_q calls): a sliced handle is sent the
c0 limbs of its units and the query's 32-byte seeds, and expands the c1 limbs itself, one limb-selective launch in front of stage A.

The expansion is a wire format: the c1 rows must equal limb u % L of the hashlib statement (tests/test_seeded_queries.py) bit for bit,
and nothing but those rows may be written -- in a slice the row behind a c1 row is the c0 row of the NEXT ciphertext.  Everything
else is an equivalence: a seeded sliced query gives, word for word, the accumulators and results of the same query sent in full.

An operator whose handles have never held a query runs the SEEDED form first wherever one operator carries both forms: the c1 rows
of an earlier unseeded query would otherwise still be in place and hide an expansion that does nothing.  At most ten handles per
process, all on the one device the tests see."""
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T16, T32, uniform_chain
from tests.test_gpu_parity import rand_limbs
from tests.test_seeded_queries import expand_ref, rand_seeds

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -2
u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _lib():
    from nested_hashing_psi_amd import _lib as l
    return l.lib()


def _P(a):
    return a.ctypes.data_as(u64p)


def _S(a):
    return a.ctypes.data_as(u8p)


def _seeded_query(rng, cc, K, E, expand):
    """random c0 halves and seeds, and the same query in full: c1 = expand(seeds) [K E + 1][L][N], the minus element last"""
    N = cc.N
    c0i, si = rand_limbs(rng, cc.q, (K, E), N), rand_seeds(rng, K, E)
    c0m, sm = rand_limbs(rng, cc.q, (), N), rand_seeds(rng)
    c1 = expand(np.concatenate([si.reshape(K * E, 32), sm.reshape(1, 32)]))
    idx = np.ascontiguousarray(np.stack([c0i, c1[:K * E].reshape(K, E, cc.L, N)], axis=2))
    return dict(c0i=c0i, si=si, c0m=c0m, sm=sm, idx=idx, minus=np.ascontiguousarray(np.stack([c0m, c1[K * E]])))


def _set_seeded(op, x, i):
    op.setIndexSeeded(x["c0i"], x["si"], query=i)
    op.setMinusCompareElementSeeded(x["c0m"], x["sm"], query=i)


def _set_full(op, x, i):
    op.setIndex(x["idx"], query=i)
    op.setMinusCompareElement(x["minus"], query=i)


def _run(op):
    op.run()
    return [op.sliceAccumulators(g).copy() for g in range(len(op.ccs))], op.getResultList().copy()


def _same(a, b, what):
    for g, (x, y) in enumerate(zip(a[0], b[0])):
        assert (x == y).all(), "%s: accumulators of handle %d differ" % (what, g)
    assert a[1].shape == b[1].shape and (a[1] == b[1]).all(), "%s: result lists differ" % what


# ---- the kernel against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 8192])
def test_c1_rows_are_the_stated_expansion_and_c0_rows_stay(ob, pie, N):
    """L = 3, K = 2 on two handles: three units each, limb indices 0, 1, 2.  The database makes stage A read the slice back: layer
    beta < E holds the plaintext 1 (all-ones in EVALUATION format) at column beta and 0 elsewhere, layer E holds 0 everywhere, so
        acc[E][u] = minus[u]                         and  acc[beta][u] = idx[u][beta] + minus[u] (mod q_l),
    each with its c0 row and its c1 row.  Expected: c0 as uploaded, c1 = limb u % L of the hashlib statement.  N = 4096: 410 chunks,
    the last one of 6 coefficients -- four words further is the c0 row of the next ciphertext, which the same comparison reads."""
    L, K, E, G, t = 3, 2, 2, 2, T32
    lib = _lib()
    ccs = [pie.PieContext(N, L, t) for _ in range(G)]
    try:
        q = ccs[0].q
        rng = np.random.default_rng(N)
        db = np.zeros((K, E + 1, E, L, N), dtype=np.uint64)
        for j in range(E):
            db[:, j, j] = 1
        masks = rand_limbs(rng, q, (E + 1,), N)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=db, preCalcRandomMask=masks)
        c0i, si = rand_limbs(rng, q, (K, E), N), rand_seeds(rng, K, E)
        c0m, sm = rand_limbs(rng, q, (), N), rand_seeds(rng)
        op.setIndexSeeded(c0i, si)
        op.setMinusCompareElementSeeded(c0m, sm)
        for cc in ccs:
            assert lib.piehip_run_slice(cc._h) == 0
        want_m = np.stack([c0m, expand_ref(sm, q, N)])                                      # [2][L][N]
        want_i = np.stack([np.stack([np.stack([c0i[h, j], expand_ref(si[h, j], q, N)]) for j in range(E)]) for h in range(K)])
        limbs = set()
        for g, (ul, uh) in enumerate(op.unitSlices):
            acc = op.sliceAccumulators(g)      # [E + 1][1][u_n][2][N]
            for u in range(ul, uh):
                h, l = divmod(u, L)
                limbs.add(l)
                assert (acc[E, 0, u - ul] == want_m[:, l]).all(), ("minus", u)
                for j in range(E):
                    s = want_i[h, j, :, l] + want_m[:, l]
                    s = np.where(s >= q[l], s - q[l], s)
                    assert (acc[j, 0, u - ul, 0] == s[0]).all(), ("c0 row", u, j)
                    assert (acc[j, 0, u - ul, 1] == s[1]).all(), ("c1 row", u, j)
        assert limbs == {0, 1, 2}
    finally:
        for cc in ccs:
            cc.close()


# ---- equivalence through the whole run --------------------------------------------------------------------------------------------
def _case(ob, pie, N, L, K, E, b, nq, G, below=None, t=T32):
    """seeded first on fresh handles, then the same queries in full on the same operator, then the oracle.  Bytes (the facade's
    rule, per handle and per query set): the c0 rows, u_n (E + 1) N 8 bytes, plus the seed tables every handle with units is handed
    whole, 32 K E + 32 bytes; over the batch that is nq times as much, and the c0 part is exactly half of the unseeded count."""
    q, p = uniform_chain(N, L, below) if below else (None, None)
    o = ob.Oracle(N, L, t, q, p)
    rng = np.random.default_rng(7000 * N + 100 * L + 10 * K + E + b + nq + G)
    db, masks = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N)
    evk = rand_limbs(rng, o.q, (L, 2), N)
    ccs = [pie.PieContext(N, L, t, q, p) for _ in range(G)]
    assert G <= 10
    try:
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=db, preCalcRandomMask=masks)
        op.setQueryBatch(nq)
        for cc in ccs:
            cc.load_relin_key(evk)
        assert (ccs[0].q == o.q).all()
        queries = [_seeded_query(rng, ccs[0], K, E, ccs[0].expand_uniform) for _ in range(nq)]
        assert (queries[0]["minus"][1] == expand_ref(queries[0]["sm"], o.q, N)).all()   # the reference's c1 is the format's
        un = [uh - ul for ul, uh in op.unitSlices]
        seed_bytes = [(32 * K * E + 32) if n else 0 for n in un]
        total = [0] * G
        for i, x in enumerate(queries):
            _set_seeded(op, x, i)
            for g in range(G):
                assert op.uploadedBytes()[g] == un[g] * (E + 1) * N * 8 + seed_bytes[g]
                total[g] += op.uploadedBytes()[g]
        for g in range(G):
            assert total[g] == un[g] * (E + 1) * N * 8 * nq + seed_bytes[g] * nq
        seeded = _run(op)
        for i, x in enumerate(queries):
            _set_full(op, x, i)
        for g in range(G):
            assert op.uploadedBytes()[g] == 2 * (un[g] * (E + 1) * N * 8)
        full = _run(op)
        _same(seeded, full, "seeded against unseeded slices")
        for i, x in enumerate(queries):
            want = o.pie_run(x["idx"], x["minus"], db, masks, evk)
            assert ((seeded[1] if nq == 1 else seeded[1][i]) == want).all(), i
        return op
    finally:
        for cc in ccs:
            cc.close()


@pytest.mark.parametrize("N,L,K,E,b,nq,G", [
    (4096, 2, 2, 3, 3, 1, 2),
    (4096, 2, 2, 3, 5, 3, 4),     # one unit each
    (4096, 4, 2, 3, 4, 1, 3),     # units split 2 + 3 + 3, the middle slice spans two inner hash functions
    (8192, 3, 3, 2, 2, 2, 3),     # K = 3
    (16384, 2, 2, 3, 2, 2, 2),    # folded ring
    (4096, 2, 2, 3, 3, 2, 6),     # handles without units or without bins
    (4096, 2, 2, 17, 2, 1, 2),    # E = 17
])
def test_seeded_slices_equal_unseeded_slices_and_the_oracle(ob, pie, N, L, K, E, b, nq, G):
    op = _case(ob, pie, N, L, K, E, b, nq, G)
    if (L, G) == (4, 3):
        assert [hi - lo for lo, hi in op.unitSlices] == [2, 3, 3]
    if G == 6:
        assert [hi - lo for lo, hi in op.unitSlices].count(0) == 2 and [hi - lo for lo, hi in op.binSlices].count(0) == 3


def test_caller_supplied_61_bit_chain(ob, pie):
    """tests/param_chains.py: the expansion reduces modulo the caller's primes (the generic 128-bit reduction)"""
    _case(ob, pie, 4096, 2, 2, 3, 3, 1, 2, below=1 << 61)


# ---- both setter forms ------------------------------------------------------------------------------------------------------------
def test_slice_form_equals_whole_query_form(ob, pie):
    """piehip_set_*_slice_seeded_q fed with hand-cut c0 slices [u_n][E][N] and [u_n][N] (and the whole seed tables) against
    piehip_set_*_slice_seeded_from_q, on fresh handles each: the same accumulators"""
    N, L, K, E, b, G, t = 4096, 2, 2, 3, 2, 2, T32
    lib = _lib()
    ccs = [pie.PieContext(N, L, t) for _ in range(2 * G)]
    try:
        rng = np.random.default_rng(31)
        q = ccs[0].q
        db, masks = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N)
        ops = [pie.QuerySlicedBatchedFHEHIPPIE(ccs[i * G:(i + 1) * G], vectorizedHCT=db, preCalcRandomMask=masks) for i in range(2)]
        x = _seeded_query(rng, ccs[0], K, E, ccs[0].expand_uniform)
        _set_seeded(ops[0], x, 0)
        for g, (ul, uh) in enumerate(ops[1].unitSlices):
            ci = np.ascontiguousarray(np.stack([x["c0i"][u // L, :, u % L] for u in range(ul, uh)]))
            cm = np.ascontiguousarray(np.stack([x["c0m"][u % L] for u in range(ul, uh)]))
            assert ci.shape == (uh - ul, E, N) and cm.shape == (uh - ul, N)
            h = ops[1].ccs[g]._h
            assert lib.piehip_set_index_slice_seeded_q(h, 0, _P(ci), _S(x["si"])) == 0
            assert lib.piehip_set_minus_slice_seeded_q(h, 0, _P(cm), _S(x["sm"])) == 0
        accs = []
        for op in ops:
            for cc in op.ccs:
                assert lib.piehip_run_slice(cc._h) == 0
            accs.append([op.sliceAccumulators(g) for g in range(G)])
        for g in range(G):
            assert (accs[0][g] == accs[1][g]).all(), g
        # ... and they are the accumulators of the full query
        _set_full(ops[0], x, 0)
        for cc in ops[0].ccs:
            assert lib.piehip_run_slice(cc._h) == 0
        for g in range(G):
            assert (ops[0].sliceAccumulators(g) == accs[1][g]).all(), g
    finally:
        for cc in ccs:
            cc.close()


# ---- mixing and order -------------------------------------------------------------------------------------------------------------
def test_seeded_and_unseeded_pieces_mixed_over_three_rounds(ob, pie):
    """a batch of three on two handles against an unseeded sliced operator on two more and the oracle, bit for bit in every round.
    Round 0: query 0 seeded, query 1 in full, query 2 seeded with a wrong c0 and wrong seeds and then set again in full -- the
    pending expansion must not write over the full one.  Round 1: only query 1 is set again, seeded; the others keep their inputs
    (their c1 rows are still there and are not expanded again).  Round 2: query 0 seeded with wrong inputs, then handed device
    arrays (piehip_set_*_slice_device_q)."""
    import torch
    N, L, K, E, b, nq, G, t = 4096, 2, 2, 3, 3, 3, 2, T32
    lib = _lib()
    o = ob.Oracle(N, L, t)
    ccs = [pie.PieContext(N, L, t) for _ in range(2 * G)]
    try:
        rng = np.random.default_rng(32)
        db, masks = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N)
        evk = rand_limbs(rng, o.q, (L, 2), N)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs[:G], vectorizedHCT=db, preCalcRandomMask=masks)
        ref = pie.QuerySlicedBatchedFHEHIPPIE(ccs[G:], vectorizedHCT=db, preCalcRandomMask=masks)
        for x in (op, ref):
            x.setQueryBatch(nq)
        for cc in ccs:
            cc.load_relin_key(evk)
        new = lambda: _seeded_query(rng, ccs[0], K, E, ccs[0].expand_uniform)
        plain = lambda: dict(idx=rand_limbs(rng, o.q, (K, E, 2), N), minus=rand_limbs(rng, o.q, (2,), N))

        def check(cur, rnd):
            for i, x in enumerate(cur):
                _set_full(ref, x, i)
            got, want = _run(op), _run(ref)
            _same(got, want, "round %d" % rnd)
            for i, x in enumerate(cur):
                assert (got[1][i] == o.pie_run(x["idx"], x["minus"], db, masks, evk)).all(), (rnd, i)

        # round 0
        cur = [new(), plain(), plain()]
        junk = new()
        _set_seeded(op, cur[0], 0)
        _set_full(op, cur[1], 1)
        _set_seeded(op, junk, 2)
        _set_full(op, cur[2], 2)
        check(cur, 0)
        # round 1: only query 1, now seeded
        cur[1] = new()
        _set_seeded(op, cur[1], 1)
        check(cur, 1)
        # round 2: device arrays after a seeded set of the same pieces
        cur[0] = plain()
        _set_seeded(op, junk, 0)
        keep = []
        for g, (ul, uh) in enumerate(op.unitSlices):
            si = np.ascontiguousarray(np.stack([cur[0]["idx"][u // L, :, :, u % L] for u in range(ul, uh)]))      # [u_n][E][2][N]
            sm = np.ascontiguousarray(np.stack([cur[0]["minus"][:, u % L] for u in range(ul, uh)]))              # [u_n][2][N]
            di, dm = torch.from_numpy(si.view(np.int64)).cuda(), torch.from_numpy(sm.view(np.int64)).cuda()
            keep += [di, dm]
            assert lib.piehip_set_index_slice_device_q(op.ccs[g]._h, 0, C.c_void_p(di.data_ptr())) == 0
            assert lib.piehip_set_minus_slice_device_q(op.ccs[g]._h, 0, C.c_void_p(dm.data_ptr())) == 0
        torch.cuda.synchronize()
        check(cur, 2)
        # ... and a seeded set after the device arrays takes the owned copy again
        cur[0] = new()
        _set_seeded(op, cur[0], 0)
        check(cur, 3)
    finally:
        for cc in ccs:
            cc.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ob, pie):
    """null c0 or seeds and q >= nq: PIEHIP_EINVAL; a handle that is not query-sliced: PIEHIP_ESTATE; each with a message.  A handle
    without units returns PIEHIP_OK and does nothing.  Nothing of a refused call reaches the handle: the round completes afterwards
    with the inputs set before."""
    N, L, K, E, b, t = 4096, 2, 2, 2, 2, T32
    lib = _lib()
    o = ob.Oracle(N, L, t)
    ccs = [pie.PieContext(N, L, t) for _ in range(2)]
    plain = pie.PieContext(N, L, t)

    def refused(rc, code):
        assert rc == code and lib.piehip_last_error().decode()

    try:
        rng = np.random.default_rng(33)
        db, masks, evk = rand_limbs(rng, o.q, (K, b, E), N), rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, vectorizedHCT=db, preCalcRandomMask=masks, unitSlices=[(0, 4), (4, 4)])
        for cc in ccs:
            cc.load_relin_key(evk)
        x, junk = (_seeded_query(rng, ccs[0], K, E, ccs[0].expand_uniform) for _ in range(2))
        _set_seeded(op, x, 0)
        h0, h1 = ccs[0]._h, ccs[1]._h
        ci, si, cm, sm = _P(junk["c0i"]), _S(junk["si"]), _P(junk["c0m"]), _S(junk["sm"])
        setters = [(lib.piehip_set_index_slice_seeded_q, ci, si), (lib.piehip_set_minus_slice_seeded_q, cm, sm),
                   (lib.piehip_set_index_slice_seeded_from_q, ci, si), (lib.piehip_set_minus_slice_seeded_from_q, cm, sm)]
        for h in (h0, h1):    # a handle with units and one without: the arguments are checked on both
            for f, c0, sd in setters:
                refused(f(h, 0, None, sd), EINVAL)
                refused(f(h, 0, c0, None), EINVAL)
                refused(f(h, 1, c0, sd), EINVAL)
        for f, c0, sd in setters:
            refused(f(plain._h, 0, c0, sd), ESTATE)
            refused(f(None, 0, c0, sd), EINVAL)
            assert f(h1, 0, c0, sd) == 0          # no units: PIEHIP_OK, nothing happens
        assert op.uploadedBytes()[1] == 0
        op.run()
        assert (op.getResultList() == o.pie_run(x["idx"], x["minus"], db, masks, evk)).all()
        # the facade's own argument checks
        with pytest.raises(ValueError):
            op.setIndexSeeded(x["c0i"], x["si"][:1])
        with pytest.raises(ValueError):
            op.setMinusCompareElementSeeded(x["minus"], x["sm"])
        with pytest.raises(ValueError):
            op.setIndexSeeded(x["c0i"], x["si"], query=1)
    finally:
        for cc in ccs + [plain]:
            cc.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_end_to_end_psi_with_seeded_slices(ob, pie):
    """keys and the query from the device client harness (piehip_client_encrypt_seeded through BatchedFHEPSIClient), the database
    through piehip_load_db_table_sliced on two handles, seeded slices up, results decrypted: the intersection is the true one"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    N, L, t = 4096, 2, T16
    k, e, K, E, b = 2, 16, 2, 5, 4
    rng = np.random.default_rng(7)
    items = np.unique(rng.integers(1, t, 400, dtype=np.uint64))[:150]
    rng.shuffle(items)
    server, clientset = items[:140].copy(), np.concatenate([items[:5], items[140:150]])
    tbl = ob.hct_build(ob.Tabulation(987654321, k + K), server, k, e, K, b, E, evict_seed=1)
    ccs = [pie.PieContext(N, L, t) for _ in range(2)]
    try:
        cl = BatchedFHEPSIClient(ccs[0], k, e, K, E, b)
        evk = cl.runSetUpPhase()
        for cc in ccs:
            cc.load_relin_key(evk)
        op = pie.QuerySlicedBatchedFHEHIPPIE(ccs, hashTable=tbl, shuffle_seed=2, mask_seed=3)
        m0, ms, i0, isd = cl.runOfflinePhaseSeeded(clientset, aSeedBase=2)
        op.setIndexSeeded(i0, isd)
        op.setMinusCompareElementSeeded(m0, ms)
        op.run()
        found = cl.extractIntersection(op.getResultList())
        assert sorted(int(v) for v in found) == sorted(int(v) for v in items[:5])
    finally:
        for cc in ccs:
            cc.close()
