"""Result limbs on the GPU (include/piehip.h "Result limbs"): piehip_mod_reduce, run() with piehip_set_result_limbs, the host-memory
path, decryption on the shorter chain through the client harness, and the refusals.

Every comparison is bit for bit, on every word, against the exact definition in tests/test_result_limbs.py (mod_reduce_exact) applied
to the oracle's output: integer arithmetic only, so every schedule gives the same bits.
"""
import ctypes as C

import numpy as np
import pytest

from tests.param_chains import T16, T32, named_chain, uniform_chain
from tests.test_gpu_parity import rand_limbs
from tests.test_result_limbs import mod_reduce_exact, reduced_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def _chain(N, L, chain):
    if chain is None:
        return None, None
    if isinstance(chain, int):
        return uniform_chain(N, L, chain)
    return named_chain(N, L, chain)


def _contexts(ob, pie, N, L, t, chain=None):
    q, p = _chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    cc = pie.PieContext(N, L, t, q, p)
    assert (cc.moduli == o.moduli).all()
    return o, cc


# ---- 1. piehip_mod_reduce ---------------------------------------------------------------------------------------------------------
def _planted_ciphertexts(o, rng, nct=2):
    """random residues in COEFFICIENT format with planted coefficients at the edges of the centred rounding, transformed to
    EVALUATION format by the oracle.  Positions 0..7: limb 0 is 0 / q - 1 and every other limb 0, (q-1)/2, (q+1)/2, q-1;
    positions 8..15: only the last limb has the edge value, every other limb is 0 / q - 1."""
    N, L, q = o.N, o.L, [int(v) for v in o.q]
    coef = rand_limbs(rng, o.q, (nct, 2), N)
    edge = lambda m, e: (0, (m - 1) // 2, (m + 1) // 2, m - 1)[e]
    for e in range(4):
        for kept in range(2):
            p = 2 * e + kept
            for l in range(L):
                kv = 0 if kept == 0 else q[l] - 1
                coef[..., l, p] = kv if l == 0 else edge(q[l], e)
                coef[..., l, 8 + p] = edge(q[l], e) if l == L - 1 else kv
    ev = np.zeros_like(coef)
    for i in range(nct):
        for c in range(2):
            for l in range(L):
                ev[i, c, l] = o.ntt(l, coef[i, c, l])
    return ev


SMALL = [(64, L, None, "all") for L in range(2, 8)] + [
    (2048, 3, 1 << 50, "all"),            # 50-bit caller chain
    (2048, 7, None, "all"),
    (4096, 4, None, "all"),
    (4096, 3, "q0_wide", "all"),          # 60-bit q_0 over 45-bit limbs: the offsets of the kernel's difference span several q_i
    (4096, 5, 1 << 61, "all"),            # 61-bit caller chain
    (4096, 3, "q_narrow_p_wide", "all"),  # 36-bit Q
]
LARGE = [
    (8192, 3, 1 << 58, "ends"),           # 58-bit caller chain; the unfolded 16-coefficient transform's ring
    (16384, 4, None, "ends"),             # C3's ring
    (16384, 7, 1 << 50, "ends"),
    (32768, 6, None, "ends"),             # C5's ring
    (32768, 4, 1 << 61, "ends"),          # 61-bit: the generic transform with one global stage
    (65536, 2, 1 << 61, "ends"),          # ... with two
    (65536, 5, None, "ends"),             # the 32-coefficient kernel behind two global stages
]


@pytest.mark.parametrize("N,L,chain,which", SMALL + LARGE)
def test_mod_reduce_matches_the_definition(ob, pie, N, L, chain, which):
    t = T16 if N <= 4096 else T32
    if chain == "q_narrow_p_wide":
        t = T16
    o, cc = _contexts(ob, pie, N, L, t, chain)
    rng = np.random.default_rng(N + 31 * L)
    x = _planted_ciphertexts(o, rng)
    keeps = range(1, L) if which == "all" else sorted({1, L - 1})
    for keep in keeps:
        got = cc.mod_reduce(x, keep)
        assert got.shape == (2, 2, keep, N)
        assert (got == mod_reduce_exact(o, x, keep)).all(), "keep = %d" % keep
    assert (cc.mod_reduce(x, L) == x).all()       # keep == L: the input, unchanged
    assert (cc.mod_reduce(x[0], 1) == mod_reduce_exact(o, x[0], 1)).all()   # one ciphertext, no leading axis
    cc.close()


# ---- 2. run() ---------------------------------------------------------------------------------------------------------------------
def _random_database(pie, o, cc, rng, K, E, b, nq):
    """random limbs everywhere (any N); a different EvalMult key per query of a batch"""
    N, L, q = o.N, o.L, o.q
    db, masks = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N)
    evks = [rand_limbs(rng, q, (L, 2), N) for _ in range(nq)]
    cc.load_relin_key(evks[0])
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    if nq > 1:
        op.setQueryBatch(nq)
        for i in range(nq):
            cc.load_relin_key(evks[i], query=i)
    return op, db, masks, evks


def _random_queries(o, rng, K, E, nq):
    return [(rand_limbs(rng, o.q, (K, E, 2), o.N), rand_limbs(rng, o.q, (2,), o.N)) for _ in range(nq)]


def _oracle_results(o, queries, db, masks, evks, layers):
    """[nq][len(layers)][2][L][N]: the oracle's full-width result of every query on the bin layers `layers`, one task per layer"""
    import concurrent.futures
    layers = list(layers)

    def layer(bn):
        return [o.pie_run(idx, minus, np.ascontiguousarray(db[:, bn:bn + 1]), np.ascontiguousarray(masks[bn:bn + 1]), evks[i])[0]
                for i, (idx, minus) in enumerate(queries)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=12) as pool:
        per_layer = list(pool.map(layer, layers))
    return np.stack([np.stack([per_layer[j][i] for j in range(len(layers))]) for i in range(len(queries))])


def _set_queries(op, queries):
    for i, (idx, minus) in enumerate(queries):
        op.setMinusCompareElement(minus, query=i)
        op.setIndex(idx, query=i)


def _results_by_query(op, got):
    """getResultList's [nq][b] view, or a raw [b][nq] / [b] result array, as [nq][b][2][keep][N]"""
    return got[None] if op.nq == 1 else got


def check_run(o, op, queries, db, masks, evks, keeps, layers):
    layers = list(layers)
    full = _oracle_results(o, queries, db, masks, evks, layers)
    _set_queries(op, queries)
    for keep in keeps:
        op.setResultLimbs(keep)
        assert op.resultLimbs == keep
        op.run()
        got = _results_by_query(op, op.getResultList())
        assert got.shape == (len(queries), op.b, 2, keep, o.N)
        want = mod_reduce_exact(o, full, keep)
        assert (got[:, layers] == want).all(), "keep = %d" % keep
    return full


@pytest.mark.parametrize("K,b,nq", [(1, 3, 1), (1, 9, 3), (2, 3, 3), (2, 9, 1), (3, 9, 3), (3, 3, 1)])
def test_run_with_result_limbs(ob, pie, K, b, nq):
    """K = 1, 2, 3; one queue (b = 3) and two (b = 9: 5 + 4 bin layers); one query and a batch of three with a key per query; every
    keep, then back to L: the full result list again"""
    N, L, E = 4096, 3, 3
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(100 * K + 10 * b + nq)
    op, db, masks, evks = _random_database(pie, o, cc, rng, K, E, b, nq)
    queries = _random_queries(o, rng, K, E, nq)
    full = check_run(o, op, queries, db, masks, evks, (1, 2), range(b))
    op.setResultLimbs(L)
    op.run()
    assert (_results_by_query(op, op.getResultList()) == full).all()
    cc.close()


@pytest.mark.parametrize("N,L,K,E,b,nq,keeps,layers", [
    (16384, 4, 2, 14, 14, 3, (1, 2), (0, 1, 2, 7, 8, 9, 12, 13)),   # C3's shape, a batch of three: both queue groups (8 + 6 layers)
    (32768, 6, 2, 3, 8, 1, (1, 5), range(8)),                       # C5's ring, L = 6
])
def test_run_with_result_limbs_full_shapes(ob, pie, N, L, K, E, b, nq, keeps, layers):
    o, cc = _contexts(ob, pie, N, L, T32)
    rng = np.random.default_rng(N + b)
    op, db, masks, evks = _random_database(pie, o, cc, rng, K, E, b, nq)
    check_run(o, op, _random_queries(o, rng, K, E, nq), db, masks, evks, keeps, layers)
    cc.close()


def test_query_slot_has_its_own_setting(ob, pie):
    """a query slot attached to another handle's database reduces to one limb while its owner hands out two, then full results"""
    N, L, K, E, b = 4096, 3, 2, 3, 4
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(77)
    op, db, masks, evks = _random_database(pie, o, cc, rng, K, E, b, 1)
    cc2 = pie.PieContext(N, L, T16)
    slot = pie.BatchedFHEHIPPIE(cc2, attachTo=op)
    qa, qb = _random_queries(o, rng, K, E, 2)
    fa = _oracle_results(o, [qa], db, masks, evks, range(b))[0]
    fb = _oracle_results(o, [qb], db, masks, evks, range(b))[0]
    _set_queries(op, [qa])
    _set_queries(slot, [qb])
    op.setResultLimbs(2)
    slot.setResultLimbs(1)
    assert (op.resultLimbs, slot.resultLimbs) == (2, 1)
    op.run(sync=False)
    slot.run(sync=False)
    assert (slot.getResultList() == mod_reduce_exact(o, fb, 1)).all()
    assert (op.getResultList() == mod_reduce_exact(o, fa, 2)).all()
    op.setResultLimbs(L)
    op.run()
    slot.run()
    assert (op.getResultList() == fa).all()
    assert (slot.getResultList() == mod_reduce_exact(o, fb, 1)).all()
    cc2.close()
    cc.close()


# ---- 3. the host-memory path ------------------------------------------------------------------------------------------------------
def _free_device_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("nq", [1, 3])
def test_host_path_with_result_limbs(ob, pie, nq):
    """runStaged, runHost, runHostAsync and runHostSeeded with keep < L on two queues (b = 9: the second group starts behind the
    first group's hand-over, each group's download behind its reduction): the page-locked result array has the reduced shape and
    equals the device list; back at L the results and the page-locked size are those of a handle that never had the setting; going
    through the settings again allocates nothing"""
    N, L, K, E, b = 4096, 3, 2, 3, 9
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(900 + nq)
    op, db, masks, evks = _random_database(pie, o, cc, rng, K, E, b, nq)
    pre = () if nq == 1 else (nq,)
    by_query = lambda a: a[None] if nq == 1 else a.transpose(1, 0, 2, 3, 4)     # [b][nq] rows -> [nq][b]

    def arrays(queries):
        idx, minus = np.stack([q[0] for q in queries]), np.stack([q[1] for q in queries])
        return (idx[0], minus[0]) if nq == 1 else (idx, minus)

    full_shape = op.hostBuffers()[2].shape
    assert full_shape == (b,) + pre + (2, L, N)
    ptr = op.resultsDevicePtr()
    free0 = None
    for rnd, keep in enumerate((1, 2, 1)):
        op.setResultLimbs(keep)
        pr = op.hostBuffers()[2]
        assert pr.shape == (b,) + pre + (2, keep, N)
        # runStaged, piece by piece, into the page-locked array
        queries = _random_queries(o, rng, K, E, nq)
        want = mod_reduce_exact(o, _oracle_results(o, queries, db, masks, evks, range(b)), keep)
        for i, (idx, minus) in enumerate(queries):
            op.stageMinus(minus, query=i)
            for h in range(K):
                op.stageIndexRow(h, np.ascontiguousarray(idx[h]), query=i)
        pr[...] = 0
        op.runStaged(pr)
        op.waitHost()
        assert (by_query(pr) == want).all()
        assert (_results_by_query(op, op.getResultList()) == want).all()     # the device list
        # runHost into an array of the facade's own, runHostAsync into the page-locked one
        queries = _random_queries(o, rng, K, E, nq)
        want = mod_reduce_exact(o, _oracle_results(o, queries, db, masks, evks, range(b)), keep)
        idx, minus = arrays(queries)
        got = op.runHost(idx, minus)
        assert got.shape == pr.shape and (by_query(got) == want).all()
        pr[...] = 0
        op.runHostAsync(np.ascontiguousarray(idx), np.ascontiguousarray(minus), pr)
        op.waitHost()
        assert (by_query(pr) == want).all()
        # seeded: c0 halves + seeds, the c1 halves expanded on the device
        seeds = rng.integers(0, 256, (nq * (K * E + 1), 32), dtype=np.uint8)
        a = cc.expand_uniform(seeds).reshape(nq, K * E + 1, L, N)
        queries = _random_queries(o, rng, K, E, nq)
        for i, (idx, minus) in enumerate(queries):
            idx[:, :, 1] = a[i, :K * E].reshape(K, E, L, N)
            minus[1] = a[i, K * E]
        want = mod_reduce_exact(o, _oracle_results(o, queries, db, masks, evks, range(b)), keep)
        idx, minus = arrays(queries)
        sd = seeds.reshape(nq, K * E + 1, 32)
        idx_seeds, minus_seeds = sd[:, :K * E].reshape(pre + (K, E, 32)), sd[:, K * E].reshape(pre + (32,))
        c0i, c0m = np.ascontiguousarray(idx[..., 0, :, :]), np.ascontiguousarray(minus[..., 0, :, :])
        got = op.runHostSeeded(c0i, np.ascontiguousarray(idx_seeds), c0m, np.ascontiguousarray(minus_seeds))
        assert (by_query(got) == want).all()
        # everything a reduced host-memory query needs exists after the first round (the reduction's full-width rows from the
        # first setting below L on): from then on the settings come and go without an allocation
        if free0 is None:
            free0 = _free_device_bytes()
        assert _free_device_bytes() == free0, "changing the setting between runs allocated or freed device memory"
        assert op.resultsDevicePtr() == ptr
    # back to L: as a handle that never had the setting
    op.setResultLimbs(L)
    assert op.hostBuffers()[2].shape == full_shape
    queries = _random_queries(o, rng, K, E, nq)
    idx, minus = arrays(queries)
    got = by_query(op.runHost(idx, minus)).copy()
    assert op.resultsDevicePtr() == ptr and _free_device_bytes() == free0
    cc3 = pie.PieContext(N, L, T16)
    cc3.load_relin_key(evks[0])
    fresh = pie.BatchedFHEHIPPIE(cc3, vectorizedHCT=db, preCalcRandomMask=masks)
    if nq > 1:
        fresh.setQueryBatch(nq)
        for i in range(nq):
            cc3.load_relin_key(evks[i], query=i)
    assert fresh.hostBuffers()[2].shape == full_shape
    assert (by_query(fresh.runHost(idx, minus)) == got).all()
    assert (got == _oracle_results(o, queries, db, masks, evks, range(b))).all()
    cc3.close()
    cc.close()


# ---- 4. semantics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equals", [True, False])
def test_kat0_decrypts_on_one_limb(ob, pie, equals):
    """KAT-0 (tests/TestBatchedFHEPIE.cpp: k=2, e=1, K=2, E=10, b=20, 100 items) at N = 16384 with the 33-bit plaintext modulus,
    results reduced to ONE 60-bit limb and decrypted on the reduced context through the client harness: exactly two matches, none when
    the element is absent, noise budget left.  Derivable worst case: log2(q_0) - log2(t) - log2(N + 1) - 1, about 12 bits.
    The observed budgets are printed (DESIGN.md section 4c has them)."""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    from tests.test_oracle_pie import distinct_items
    N, L, t = 16384, 4, T32
    o, cc = _contexts(ob, pie, N, L, t)
    rng = np.random.default_rng(122333444455555 % (1 << 32))
    items = distinct_items(rng, t, 100)
    k, e, K, E, b = 2, 1, 2, 10, 20
    present = set(int(x) for x in items)
    elem = int(items[50]) if equals else next(v for v in range(1, t) if v not in present)
    sk = o.keygen(1)
    evk = o.relin_keygen(sk, 2)
    tab = ob.Tabulation(12223222, k + K)
    tbl = ob.hct_build(tab, items, k, e, K, b, E, evict_seed=5)
    idx = np.zeros((K, E, 2, L, N), dtype=np.uint64)
    for h in range(K):
        hi = tab.hash(elem, k + h) % E
        for j in range(E):
            idx[h, j] = o.encrypt_slots(sk, [1, 1] if j == hi else [0, 0], 10 + h * E + j)
    minus = o.encrypt_slots(sk, [-elem, -elem], 9)
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, hashTable=tbl, shuffle_seed=6, mask_seed=7)
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    full = op.getResultList().copy()
    op.setResultLimbs(1)
    op.run()
    red = op.getResultList().copy()
    assert red.shape == (b, 2, 1, N)
    assert (red == mod_reduce_exact(o, full, 1)).all()
    cl = BatchedFHEPSIClient(cc, k, e, K, E, b)
    cl.sk = sk
    dec = cl.decrypt(red, nslots=2, limbs=1)
    assert cl._reduced_context(1) is cl._reduced_context(1)          # made once, reused
    assert (dec == cl.decrypt(full, nslots=2)).all()                 # the slots of the full ciphertexts
    assert int((dec == 0).sum()) == (2 if equals else 0)
    o1 = reduced_oracle(ob, o, 1)
    budgets = [o1.decrypt_slots(np.ascontiguousarray(sk[:1]), red[bn], 2)[1] for bn in range(b)]
    full_budgets = [o.decrypt_slots(sk, full[bn], 2)[1] for bn in range(b)]
    print("KAT-0 N=16384 t=%d keep=1 equals=%s: noise budget min %d max %d bits (full ciphertexts: min %d)"
          % (t, equals, min(budgets), max(budgets), min(full_budgets)))
    assert min(budgets) >= 1
    cc.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(ob, pie):
    from nested_hashing_psi_amd._lib import lib, u64p
    N, L, K, E, b = 4096, 3, 2, 3, 3
    o, cc = _contexts(ob, pie, N, L, T16)
    rng = np.random.default_rng(5)
    op, db, masks, evks = _random_database(pie, o, cc, rng, K, E, b, 1)
    queries = _random_queries(o, rng, K, E, 1)
    full = _oracle_results(o, queries, db, masks, evks, range(b))[0]
    _set_queries(op, queries)
    x = rand_limbs(rng, o.q, (1, 2), N)
    out = np.zeros((1, 2, L, N), dtype=np.uint64)
    for keep in (0, L + 1):
        assert lib().piehip_set_result_limbs(cc._h, keep) == pie.EINVAL
        assert b"keep" in lib().piehip_last_error()
        assert lib().piehip_mod_reduce(cc._h, x.ctypes.data_as(u64p), 1, keep, out.ctypes.data_as(u64p)) == pie.EINVAL
        assert b"keep" in lib().piehip_last_error()
        with pytest.raises(ValueError):
            op.setResultLimbs(keep)
        with pytest.raises(ValueError):
            cc.mod_reduce(x, keep)
    assert lib().piehip_get_result_limbs(cc._h, None) == pie.EINVAL
    assert op.resultLimbs == L
    # the captured graph and fewer limbs exclude each other, whichever comes second
    cc.set_graph(True)
    assert lib().piehip_set_result_limbs(cc._h, 1) == pie.ESTATE
    assert b"graph" in lib().piehip_last_error()
    assert op.resultLimbs == L
    op.setResultLimbs(L)                       # L is what the graph hands out: accepted
    op.run()
    assert (op.getResultList() == full).all()
    cc.set_graph(False)
    op.setResultLimbs(2)
    assert lib().piehip_set_graph(cc._h, 1) == pie.ESTATE
    assert b"set_result_limbs" in lib().piehip_last_error()
    op.run()
    assert (op.getResultList() == mod_reduce_exact(o, full, 2)).all()
    # the gather of a sharded server refuses reduced results, before it looks at its communicator
    p = u64p()
    assert lib().piehip_gather_results_host(cc._h, b, 0, C.byref(p)) == pie.ESTATE
    assert b"piehip_set_result_limbs" in lib().piehip_last_error()
    assert lib().piehip_gather_results(cc._h, b, 0, C.c_void_p(op.resultsDevicePtr())) == pie.ESTATE
    assert b"piehip_set_result_limbs" in lib().piehip_last_error()
    op.setResultLimbs(L)
    op.run()
    assert (op.getResultList() == full).all()
    cc.close()
