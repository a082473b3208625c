"""Layer tiling on the GPU (include/piehip.h "Layer tiling"): databases tiled on the device by piehip_load_db_table(_bins) and
piehip_build_db(_bins) under piehip_set_layer_tiling, compared with the definition of tests/layer_tiling.py.

Every result row is compared bit for bit with o.pie_run on the tiled arrays -- the oracle's shuffled table packed by ob.pack_db and
re-arranged by tile_db_slots, the oracle's mask draw re-arranged by tile_masks, the client's vectors repeated by tile_vectors --
which is how tests/test_gpu_fullsize.py checks an untiled database.  One shape's table, query and reference are computed once
(_shape, _reference) and shared.  The K = 1 case: every entry point that builds from a table refuses K = 1 (a Cuckoo table has more
than one hash function), so that case loads the hand-tiled arrays through piehip_load_db_slots, which ignores the setting.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.layer_tiling import tile_db_slots, tile_masks, tile_vectors, tiled_layers, untile
from tests.test_oracle_pie import distinct_items

pytestmark = pytest.mark.gpu
T16 = 65537
T32 = 4296540161
SEEDS = dict(hash_seed=987654321, evict_seed=1, shuffle_seed=2, mask_seed=3)
#         N     L  t    k  e    K  b  E  |S|
C1 = (4096, 2, T16, 3, 110, 2, 7, 3, 1500)      # BASELINE.md C1's packing, a smaller table
FULL = (4096, 2, T16, 2, 512, 2, 5, 3, 4000)    # R = 4 fills the ring: R*B = N
C2 = (8192, 3, T32, 3, 443, 2, 5, 4, 6000)      # C2's packing
K3 = (4096, 3, T16, 3, 110, 3, 4, 3, 1200)


@pytest.fixture(scope="module")
def pie(pie_mod):
    return pie_mod


@functools.lru_cache(maxsize=None)
def _shape_cached(ob, shape):
    N, L, t, k, e, K, b, E, nS = shape
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(N + e + K)
    items = distinct_items(rng, t, nS + 40)
    server, client = items[:nS].copy(), np.concatenate([items[:9], items[nS:nS + 31]])
    rng.shuffle(client)
    tab = ob.Tabulation(SEEDS["hash_seed"], k + K)
    tbl0 = ob.hct_build(tab, server, k, e, K, b, E, evict_seed=SEEDS["evict_seed"])   # before the shuffle: what a server hands in
    tbl = tbl0.copy()
    ob.hct_shuffle_bins(tbl, SEEDS["shuffle_seed"])
    ctab = ob.client_build(tab, client, k, e, evict_seed=4)
    index, minus = ob.client_vectors(tab, ctab, K, E)
    sk = o.keygen(11)
    return dict(o=o, server=server, tbl0=tbl0, tbl=tbl, slots=ob.pack_db(tbl), index=index, minus=minus, sk=sk,
                evk=o.relin_keygen(sk, 12), ctab=ctab, inter=np.sort(items[:9]))


def _shape(ob, shape):
    return _shape_cached(ob, shape)


@functools.lru_cache(maxsize=None)
def _reference(ob, shape, R):
    """(idx, minus, want[b'][2][L][N]) of shape tiled by R (R = 1: untiled)"""
    N, L, t, k, e, K, b, E, _ = shape
    d = _shape(ob, shape)
    o, sk, B = d["o"], d["sk"], k * e
    st, mt = tile_db_slots(d["slots"], R), tile_masks(ob, t, b, B, SEEDS["mask_seed"], R)
    bt = tiled_layers(b, R)
    db = np.stack([o.encode_eval(st[h, g, j]) for h in range(K) for g in range(bt) for j in range(E)]).reshape(K, bt, E, L, N)
    masks = np.stack([o.encode_eval(mt[g]) for g in range(bt)])
    iv, mv = tile_vectors(d["index"], R), tile_vectors(d["minus"], R)
    idx = np.stack([o.encrypt_slots(sk, iv[h, j], 100 + h * E + j) for h in range(K) for j in range(E)]).reshape(K, E, 2, L, N)
    minus = o.encrypt_slots(sk, mv, 99)
    want = o.pie_run(idx, minus, db, masks, d["evk"])
    for a in (idx, minus, want):
        a.setflags(write=False)
    return idx, minus, want


def drop_references():
    """let go of the shared oracles and arrays (tests/test_gpu_layer_tiling_cpp.py shares them too)"""
    _shape_cached.cache_clear()
    _reference.cache_clear()


@pytest.fixture(scope="module", autouse=True)
def _references_live_as_long_as_the_module():
    yield
    drop_references()


def _run(op, idx, minus):
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    return op.getResultList().copy()


def _context(pie, shape, d):
    cc = pie.PieContext(shape[0], shape[1], shape[2])
    cc.load_relin_key(d["evk"])
    return cc


# ---- 1. piehip_load_db_table with the setting -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,R", [(C1, 7), (C1, 3), (FULL, 4), (C2, 6), (C2, 2), (K3, 4), (K3, 3)],
                         ids=["c1-one-layer", "c1-3+3+1", "ring-filled", "c2-one-layer", "c2-2+2+1", "k3-one-layer", "k3-3+1"])
def test_table_load_tiles_on_the_device(ob, pie, shape, R):
    N, L, t, k, e, K, b, E, _ = shape
    d = _shape(ob, shape)
    idx, minus, want = _reference(ob, shape, R)
    bt = tiled_layers(b, R)
    cc = _context(pie, shape, d)
    op = pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=SEEDS["shuffle_seed"], mask_seed=SEEDS["mask_seed"], layerTiling=R)
    assert op.b == bt and cc.layerTiling() == R
    assert (op.hashTable() == d["tbl"]).all()      # still the untiled [k][e][K][b][E], after the shuffle
    got = _run(op, idx, minus)
    cc.close()
    assert got.shape == (bt, 2, L, N)
    assert (got == want).all()
    # ... and un-tiled, the plaintext is the untiled run's: the intersection comes out of the first b blocks
    o = d["o"]
    dec = np.stack([o.decrypt_slots(d["sk"], got[g], R * k * e)[0] for g in range(bt)])
    assert (np.sort(ob.client_scan(d["ctab"], untile(dec, R, k * e, b))) == d["inter"]).all()


def test_one_inner_hash_function_tiled_by_hand(ob, pie):
    """K = 1: the hand-tiled arrays through piehip_load_db_slots (the setting is ignored there, also when it is set)"""
    N, L, t, R = 4096, 2, T16, 3
    k, e, b, E = 3, 110, 4, 3
    B = k * e
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(41)
    slots = rng.integers(-(t // 2), t // 2 + 1, (1, b, E, B))
    st, mt = tile_db_slots(slots, R), tile_masks(ob, t, b, B, 9, R)
    bt = tiled_layers(b, R)
    sk = o.keygen(11)
    index = np.zeros((1, E, B), dtype=np.int64)
    index[0, rng.integers(0, E, B), np.arange(B)] = 1
    iv, mv = tile_vectors(index, R), tile_vectors(-slots[0, 2, 1], R)
    idx = np.stack([o.encrypt_slots(sk, iv[0, j], 100 + j) for j in range(E)]).reshape(1, E, 2, L, N)
    minus = o.encrypt_slots(sk, mv, 99)
    db = np.stack([o.encode_eval(st[0, g, j]) for g in range(bt) for j in range(E)]).reshape(1, bt, E, L, N)
    masks = np.stack([o.encode_eval(mt[g]) for g in range(bt)])
    cc = pie.PieContext(N, L, t)
    cc.setLayerTiling(2)
    op = pie.BatchedFHEHIPPIE(cc, slots=st, mask_slots=mt)
    assert op.b == bt
    got = _run(op, idx, minus)
    cc.close()
    assert (got == o.pie_run(idx, minus, db, masks, np.zeros((L, 2, L, N), dtype=np.uint64))).all()


# ---- 2. piehip_build_db from a server set with the setting ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,R", [(C1, 3), (C2, 6)], ids=["c1-3+3+1", "c2-one-layer"])
def test_build_from_a_server_set_tiles_on_the_device(ob, pie, shape, R):
    N, L, t, k, e, K, b, E, _ = shape
    d = _shape(ob, shape)
    idx, minus, want = _reference(ob, shape, R)
    cc = _context(pie, shape, d)
    cc.setLayerTiling(R)
    cc.reserve(len(d["server"]), k, e, K, b, E)    # sized for b' layers of R*B slots
    op = pie.BatchedFHEHIPPIE(cc, serverSet=d["server"], hashParams=dict(k=k, e=e, K=K, b=b, E=E, **SEEDS), layerTiling=R)
    assert op.b == tiled_layers(b, R)
    reported = op.hashTable()
    got = _run(op, idx, minus)
    cc.close()
    assert (reported == d["tbl"]).all()    # the table it reports is the oracle's, so case 1's reference is this one's
    assert (got == want).all()


# ---- 3. a slice of the tiled layers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["table", "server-set"])
def test_bin_slice_counts_tiled_layers(ob, pie, build):
    shape, R = C1, 3     # three tiled layers: 3 + 3 + 1 bin layers
    N, L, t, k, e, K, b, E, _ = shape
    d = _shape(ob, shape)
    idx, minus, want = _reference(ob, shape, R)
    cc = _context(pie, shape, d)
    if build == "table":
        op = pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=SEEDS["shuffle_seed"], mask_seed=SEEDS["mask_seed"],
                                  binSlice=(1, 3), layerTiling=R)
    else:
        op = pie.BatchedFHEHIPPIE(cc, serverSet=d["server"], hashParams=dict(k=k, e=e, K=K, b=b, E=E, **SEEDS), binSlice=(1, 3),
                                  layerTiling=R)
    assert op.b == 2
    got = _run(op, idx, minus)
    assert (got == want[1:3]).all()
    # a slice is counted in tiled layers: [0, 4) is outside three of them, though inside the seven bin layers
    with pytest.raises(ValueError, match="bin-layer slice"):
        pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=2, mask_seed=3, binSlice=(0, 4), layerTiling=R)
    cc.close()


# ---- 4. R = 1 is the handle that never heard of the setting ---------------------------------------------------------------------------
def _raw_load_and_run(pie, cc, d, shape, idx, minus):
    """load_db_table + run through the C ABI alone: nothing here touches the tiling calls"""
    from nested_hashing_psi_amd._lib import lib, u64p
    N, L, t, k, e, K, b, E, _ = shape
    tbl = np.ascontiguousarray(d["tbl0"])
    pie._check(lib().piehip_load_db_table(cc._h, tbl.ctypes.data_as(u64p), k, e, K, b, E, SEEDS["shuffle_seed"], SEEDS["mask_seed"]))
    pie._check(lib().piehip_set_minus_q(cc._h, 0, np.ascontiguousarray(minus).ctypes.data_as(u64p)))
    pie._check(lib().piehip_set_index_q(cc._h, 0, np.ascontiguousarray(idx).ctypes.data_as(u64p)))
    pie._check(lib().piehip_run(cc._h))
    pie._check(lib().piehip_sync(cc._h))
    out = np.zeros((b, 2, L, N), dtype=np.uint64)
    pie._check(lib().piehip_get_results(cc._h, out.ctypes.data_as(u64p)))
    return out


def test_tiling_of_one_changes_nothing(ob, pie):
    from nested_hashing_psi_amd._lib import lib
    shape = C1
    d = _shape(ob, shape)
    idx, minus, want = _reference(ob, shape, 1)
    cc0 = _context(pie, shape, d)
    never = _raw_load_and_run(pie, cc0, d, shape, idx, minus)
    cc0.close()
    assert (never == want).all()
    cc = _context(pie, shape, d)
    assert cc.layerTiling() == 1       # the default
    assert lib().piehip_set_layer_tiling(cc._h, 1) == 0
    assert (_raw_load_and_run(pie, cc, d, shape, idx, minus) == never).all()
    # ... and after a tiled database on the same handle, back at 1: nothing of the tiling is left behind
    idx3, minus3, want3 = _reference(ob, shape, 3)
    op = pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=SEEDS["shuffle_seed"], mask_seed=SEEDS["mask_seed"], layerTiling=3)
    assert (_run(op, idx3, minus3) == want3).all()
    cc.setLayerTiling(1)
    assert (_raw_load_and_run(pie, cc, d, shape, idx, minus) == never).all()
    cc.close()


def test_an_attached_handle_takes_the_tiled_database_as_it_is(ob, pie):
    """piehip_attach_database to a tiled database: b' layers, whatever the borrower's own setting says"""
    shape, R = C1, 3
    d = _shape(ob, shape)
    idx, minus, want = _reference(ob, shape, R)
    cc = _context(pie, shape, d)
    op = pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=SEEDS["shuffle_seed"], mask_seed=SEEDS["mask_seed"], layerTiling=R)
    cc2 = pie.PieContext(shape[0], shape[1], shape[2])
    cc2.setLayerTiling(2)
    slot = pie.BatchedFHEHIPPIE(cc2, attachTo=op)
    assert slot.b == op.b == tiled_layers(shape[6], R)
    assert (_run(slot, idx, minus) == want).all()
    cc2.close()
    cc.close()


# ---- 5. end to end with the device client ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 7])
def test_end_to_end_with_tiling_clients(ob, pie, R):
    """layerTiling = R on both ends; three different clients in one batch, each under its own key; one result limb; one of the queries
    seeded.  Every intersection is the untiled handle's and the oracle's client_scan of the untiled plaintext; every budget above 0."""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    N, L, t = 4096, 3, T16
    k, e, K, E, b = 3, 110, 2, 3, 7
    nq, bt = 3, tiled_layers(b, R)
    rng = np.random.default_rng(99)
    items = distinct_items(rng, t, 1500 + nq * 40)
    server = items[:1500].copy()
    hp = dict(k=k, e=e, K=K, b=b, E=E, **SEEDS)
    sets = [np.concatenate([server[q * 50:q * 50 + 11 + q], items[1500 + q * 40:1500 + q * 40 + 25]]) for q in range(nq)]

    def serve(R_):
        """the three clients against one server tiled by R_: (intersections, untiled plaintexts [b][B], budgets)"""
        cc = pie.PieContext(N, L, t)
        srv = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=hp, layerTiling=R_)
        srv.setQueryBatch(nq)
        srv.setResultLimbs(1)
        clients = []
        for q in range(nq):
            cl = BatchedFHEPSIClient(pie.PieContext(N, L, t), k, e, K, E, b, layerTiling=R_)
            cc.load_relin_key(cl.runSetUpPhase(keySeed=11 + q, evalKeySeed=21 + q), query=q)
            minus, idx = cl.runOfflinePhase(sets[q], encSeedBase=100 + 1000 * q)
            if q == 1:    # the seeded query: c0 halves + seeds, expanded on a context of the client's and then uploaded whole
                m0, ms, i0, isd = cl.runOfflinePhaseSeeded(sets[q], encSeedBase=5000, aSeedBase=2)
                c1 = cl.cc.expand_uniform(np.concatenate([ms[None], isd.reshape(-1, 32)]))
                minus = np.stack([m0, c1[0]])
                idx = np.stack([i0, c1[1:].reshape(K, E, L, N)], axis=2)
            srv.setMinusCompareElement(minus, query=q)
            srv.setIndex(idx, query=q)
            clients.append(cl)
        srv.run()
        res = srv.getResultList().copy()
        assert res.shape == (nq, tiled_layers(b, R_), 2, 1, N)
        found, plain, budgets = [], [], []
        for q, cl in enumerate(clients):
            dec, bud = cl.decrypt(res[q], limbs=1, budget=True)
            assert dec.shape == (tiled_layers(b, R_), R_ * k * e)
            budgets += [int(v) for v in bud]
            found.append(sorted(int(v) for v in cl.extractIntersection(res[q], limbs=1)))
            plain.append(cl.batchedDecryptedResult.copy())
            cl.cc.close()
        cc.close()
        return found, plain, budgets, [cl.clientTable for cl in clients]

    f1, p1, b1, tabs = serve(1)
    fR, pR, bR, _ = serve(R)
    print("budgets untiled %s\nbudgets R = %d %s" % (b1, R, bR))
    for q in range(nq):
        truth = sorted(int(v) for v in server[q * 50:q * 50 + 11 + q])
        assert pR[q].shape == (b, k * e)
        assert fR[q] == f1[q] == truth == sorted(int(v) for v in ob.client_scan(tabs[q], p1[q]))
        assert sorted(int(v) for v in ob.client_scan(tabs[q], pR[q])) == truth
        assert (pR[q] == p1[q]).all()      # slot for slot the untiled plaintext: same table, shuffle and masks
    assert len(bR) == nq * bt and min(bR) > 0 and min(b1) > 0


# ---- 6. refusals and the getter ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(ob, pie):
    from nested_hashing_psi_amd._lib import lib, u64p
    shape = C1
    N, L, t, k, e, K, b, E, _ = shape
    d = _shape(ob, shape)
    idx, minus, want = _reference(ob, shape, 3)
    cc = _context(pie, shape, d)
    R = C.c_uint32(99)
    assert lib().piehip_get_layer_tiling(cc._h, C.byref(R)) == 0 and R.value == 1
    assert lib().piehip_set_layer_tiling(cc._h, 0) == pie.EINVAL
    assert b"layer tiling" in lib().piehip_last_error()
    assert cc.layerTiling() == 1
    with pytest.raises(ValueError, match="layer tiling"):
        cc.setLayerTiling(0)
    op = pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=SEEDS["shuffle_seed"], mask_seed=SEEDS["mask_seed"], layerTiling=3)
    assert (_run(op, idx, minus) == want).all()
    # R*k*e > N: 13 * 330 = 4290 > 4096 (12 fits); refused by both loaders and by reserve, and the old database still runs
    tbl = np.ascontiguousarray(d["tbl0"])
    srv = np.ascontiguousarray(d["server"])
    cc.setLayerTiling(13)
    assert lib().piehip_load_db_table(cc._h, tbl.ctypes.data_as(u64p), k, e, K, b, E, 2, 3) == pie.EINVAL
    assert b"R*k*e exceeds the ring dimension" in lib().piehip_last_error()
    assert lib().piehip_build_db(cc._h, srv.ctypes.data_as(u64p), len(srv), k, e, K, b, E, 987654321, 1, 2, 3) == pie.EINVAL
    assert b"R*k*e exceeds the ring dimension" in lib().piehip_last_error()
    assert lib().piehip_reserve(cc._h, len(srv), k, e, K, b, E, 0, 1) == pie.EINVAL
    assert b"R*k*e exceeds the ring dimension" in lib().piehip_last_error()
    assert cc.layerTiling() == 13
    op.run()
    assert (op.getResultList() == want).all()
    cc.setLayerTiling(12)
    op12 = pie.BatchedFHEHIPPIE(cc, hashTable=d["tbl0"], shuffle_seed=2, mask_seed=3, layerTiling=12)
    assert op12.b == 1
    cc.close()
    # both sliced loaders refuse a tiling above 1, and take the handle again at 1
    cc = pie.PieContext(N, L, t)
    cc.setLayerTiling(2)
    with pytest.raises(RuntimeError, match="query slice: not with a layer tiling"):
        pie.QuerySlicedBatchedFHEHIPPIE([cc], hashTable=d["tbl0"], shuffle_seed=2, mask_seed=3)
    with pytest.raises(RuntimeError, match="query slice: not with a layer tiling"):
        pie.QuerySlicedBatchedFHEHIPPIE([cc], serverSet=d["server"], hashParams=dict(k=k, e=e, K=K, b=b, E=E, **SEEDS))
    assert lib().piehip_load_db_table_sliced(cc._h, tbl.ctypes.data_as(u64p), k, e, K, b, E, 2, 3, 0, K * L, 0, b) == pie.ESTATE
    cc.setLayerTiling(1)
    pie.QuerySlicedBatchedFHEHIPPIE([cc], hashTable=d["tbl0"], shuffle_seed=2, mask_seed=3)
    cc.close()
    # the facades: a tiling on a database that is not built from a table or a set, and a client whose tiling does not fit
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    cc = pie.PieContext(N, L, t)
    with pytest.raises(ValueError, match="layerTiling applies"):
        pie.BatchedFHEHIPPIE(cc, slots=np.zeros((1, 1, 1, 4), dtype=np.int64), mask_slots=np.ones((1, 4), dtype=np.int64), layerTiling=2)
    with pytest.raises(ValueError, match="layerTiling"):
        BatchedFHEPSIClient(cc, k, e, K, E, b, layerTiling=13)
    cc.close()
