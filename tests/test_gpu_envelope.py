"""GPU parity over the whole parameter range piehip_create accepts (params.cpp): L up to MAX_L = 7, rings of 8 to 65536
coefficients, caller-supplied chains of mixed modulus widths and the reference's 40- and 48-bit plaintext moduli.

The library picks hand-specialised kernels by logN, by the widths of the moduli and by L; the points below reach the
branches the benchmark shapes never run (each row of the parametrisations says which).  Every point is compared against
the CPU oracle built on the same moduli, bit for bit: tables, transforms over QP and over t, the three base conversions,
EvalMult, encode and a small run().
"""
import numpy as np
import pytest

from tests.param_chains import NAMED, T16, T32, T40, T48, named_chain, uniform_chain
from tests.test_gpu_parity import _query, rand_limbs

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


def _contexts(ob, pie, N, L, t, chain):
    q, p = _chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    cc = pie.PieContext(N, L, t, q, p)
    assert (cc.moduli == o.moduli).all()
    if q is not None:
        assert (cc.q == q).all() and (cc.p == p).all()
    return o, cc


def check_ops(ob, pie, o, cc, rng):
    """tables, NTT over QP and over t, base conversions, EvalMult (+ decrypted slots) and encode against the oracle"""
    N, L, t, M = o.N, o.L, o.t, o.M
    for mi in range(M + 1):
        assert cc.psi(mi) == o.psi(mi)
    for mi in sorted({0, L - 1, L, M - 1, M}):
        f1, i1 = cc.twiddles(mi)
        f2, i2 = o.twiddles(mi)
        assert (f1[1:] == f2[1:]).all() and (i1[1:] == i2[1:]).all()
    assert (cc.slot_positions() == o.slot_positions()).all()

    # forward / inverse transform over QP; an all-zero limb and an all q - 1 limb
    x = rand_limbs(rng, o.moduli[:M], (2,), N)
    x[0, 0, :] = 0
    x[1, M - 1, :] = o.moduli[M - 1] - np.uint64(1)
    f = cc.ntt(x, 0, M)
    assert (f == np.stack([np.stack([o.ntt(mi, x[k, mi]) for mi in range(M)]) for k in range(2)])).all()
    assert (cc.ntt(f, 0, M, inverse=True) == x).all()
    # ... and over the plaintext modulus
    z = rng.integers(0, t, (2, N), dtype=np.uint64)
    z[1, :] = t - 1
    fz = cc.ntt(z, M, 1)
    assert (fz == np.stack([o.ntt(M, z[k]) for k in range(2)])).all()
    assert (cc.ntt(fz, M, 1, inverse=True) == z).all()

    # base conversions; columns 0 and Q - 1 (QP - 1) in the first polynomial
    xq = rand_limbs(rng, o.q, (4,), N)     # the extensions take polynomials in pairs, scale-and-round in triples
    xq[0, :, 0] = 0
    xq[0, :, 1] = o.q - np.uint64(1)
    assert (cc.base_convert(0, xq) == np.stack([o.expand_q_to_qp(v) for v in xq])).all()
    assert (cc.base_convert(1, xq) == np.stack([o.scale_pq_expand(v) for v in xq])).all()
    xqp = rand_limbs(rng, o.moduli[:M], (3,), N)
    xqp[0, :, 0] = 0
    xqp[0, :, 1] = o.moduli[:M] - np.uint64(1)
    assert (cc.base_convert(2, xqp) == np.stack([o.scale_round_tp(v) for v in xqp])).all()

    # EvalMult with and without relinearisation
    sk = o.keygen(3)
    evk = o.relin_keygen(sk, 4)
    cc.load_relin_key(evk)
    xs, ys = [1, 2, 3, -4], [5, -6, 7, 8]
    a = np.stack([o.encrypt_slots(sk, xs, 5), o.encrypt_slots(sk, ys, 7)])
    b = np.stack([o.encrypt_slots(sk, ys, 6), o.encrypt_slots(sk, xs, 8)])
    assert (cc.EvalMult(a, b, relin=False) == np.stack([o.mul_tensor(a[i], b[i]) for i in range(2)])).all()
    prod = cc.EvalMult(a, b)
    assert (prod == np.stack([o.mul(a[i], b[i], evk) for i in range(2)])).all()
    if L >= 2:  # at L = 1 the single BV digit is as wide as Q: the relinearised product is noise, bit-exact but undecryptable
        assert list(o.decrypt_slots(sk, prod[0], 4)[0]) == [5, -12, 21, -32]
    assert list(o.decrypt_slots(sk, cc.EvalMult(a, b, relin=False)[1], 4)[0]) == [5, -12, 21, -32]

    # encode, including the slot values +-(t - 1) / 2 and +-(t - 1) (the range the encoder accepts)
    for B in sorted({1, N // 2, N}):
        s = rng.integers(-(t // 2), t // 2 + 1, (2, B), dtype=np.int64)
        s[0, 0], s[1, 0] = t // 2, t - 1
        s[0, B - 1], s[1, B - 1] = -(t // 2), -(t - 1)
        got = cc.MakePackedPlaintext(s)
        assert (got == np.stack([o.encode_eval(s[k]) for k in range(2)])).all()
    return sk, evk


def rand_run(pie, o, cc, rng, K=2, E=3, b=2):
    """a small run() on random limbs (no hashing harness: any N) against o.pie_run; returns the inputs for re-use"""
    N, L, q = o.N, o.L, o.q
    db, masks, evk = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (L, 2), N)
    idx, minus = rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)
    cc.load_relin_key(evk)
    op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    assert (op.getResultList() == o.pie_run(idx, minus, db, masks, evk)).all()
    return op, db, masks, evk


def extreme_run(pie, o, cc, rng, K=2, E=3, b=2):
    """residues 0 and q - 1 in every array that enters run() (test_extreme_residues_through_run), then every residue q - 1:
    the column accumulators of the widest sums"""
    N, L, q = o.N, o.L, o.q

    def rl(shape):
        a = rand_limbs(rng, q, shape, N)
        for i in range(L):
            a[..., i, 0:64] = q[i] - np.uint64(1)
            a[..., i, 64:128] = 0
            a[..., i, N // 2:N // 2 + 32] = q[i] - np.uint64(1)
            a[..., i, N - 32:] = q[i] - np.uint64(1)
        return a
    evk = rl((L, 2))
    cc.load_relin_key(evk)
    allmax = lambda shape: np.broadcast_to((q - np.uint64(1))[:, None], shape + (L, N)).copy()
    for mk in (rl, allmax):
        idx, minus, db, masks = mk((K, E, 2)), mk((2,)), mk((K, b, E)), mk((b,))
        op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
        op.setMinusCompareElement(minus)
        op.setIndex(idx)
        op.run()
        assert (op.getResultList() == o.pie_run(idx, minus, db, masks, evk)).all()


# ---- L = 7 (MAX_L) on the default chain ---------------------------------------------------------------------------------
def test_L7_headline_ring(ob, pie):
    """N = 16384, L = 7: SA(7) stage A (seven key-switch digits, M = 15 limbs in the tensor product), crt_out<8> through dot128's
    MAD branch, scale_round outside its MAD && L <= 6 block; a batch of three queries (the batch kernel at L = 7) and the
    0 / q - 1 residue patterns (COLACC_MAX_TERMS = 8, COLACC_MAX_TOTAL = 15 reached)"""
    o, cc = _contexts(ob, pie, 16384, 7, T32, None)
    rng = np.random.default_rng(16384 + 7)
    check_ops(ob, pie, o, cc, rng)
    op, db, masks, evk = rand_run(pie, o, cc, rng)
    K, E, b, N, q = 2, 3, 2, o.N, o.q
    queries = [(rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)) for _ in range(3)]
    op.setQueryBatch(3)
    for i in (2, 0, 1):
        op.setIndex(queries[i][0], query=i)
        op.setMinusCompareElement(queries[i][1], query=i)
    op.run()
    got = op.getResultList()
    assert got.shape == (3, b, 2, o.L, N)
    for i, (idx, minus) in enumerate(queries):
        assert (got[i] == o.pie_run(idx, minus, db, masks, evk)).all(), "query %d of the batch" % i
    op.setQueryBatch(1)
    extreme_run(pie, o, cc, rng)
    cc.close()


@pytest.mark.parametrize("N,ops,run,extreme", [
    (32768, True, True, True),     # folded 16-coefficient transforms (2^14 slices) at L = 7
    (8192, True, False, False),    # the unfolded 16-coefficient transform (one 2^13 slice per limb) at L = 7
])
def test_L7_sixteen_coefficient_rings(ob, pie, N, ops, run, extreme):
    o, cc = _contexts(ob, pie, N, 7, T32, None)
    rng = np.random.default_rng(N + 7)
    if ops:
        check_ops(ob, pie, o, cc, rng)
    if run:
        rand_run(pie, o, cc, rng)
    if extreme:
        extreme_run(pie, o, cc, rng)
    cc.close()


# ---- ring sizes outside the benchmark's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 7])
def test_largest_ring(ob, pie, L):
    """N = 65536: the only ring whose route (ntt_route) has s0 = 2 (two ntt_global_stage passes before the fast kernel, in that order), no
    folded or 16-coefficient transform: unfolded base conversions and digits_kernel"""
    o, cc = _contexts(ob, pie, 65536, L, T32, None)
    rng = np.random.default_rng(65536 + L)
    check_ops(ob, pie, o, cc, rng)
    rand_run(pie, o, cc, rng)
    cc.close()


@pytest.mark.parametrize("N", [8, 16, 32])
@pytest.mark.parametrize("L", [1, 2])
def test_smallest_rings(ob, pie, N, L):
    """N = 8, 16, 32: ntt_lds_generic with 64 threads for 4 to 16 butterflies (idle lanes); run() on random limbs, as the
    hashing harness cannot fit its slots into so small a ring"""
    o, cc = _contexts(ob, pie, N, L, T16, None)
    rng = np.random.default_rng(N + L)
    check_ops(ob, pie, o, cc, rng)
    rand_run(pie, o, cc, rng)
    rand_run(pie, o, cc, rng, K=3, E=2, b=3)
    cc.close()


# ---- modulus widths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,below,what", [
    (32768, 4, 1 << 61, "61-bit: generic transform with one global stage, non-MAD kernels at L >= 4"),
    (65536, 2, 1 << 61, "61-bit: generic transform with two global stages"),
    (32768, 5, 1 << 50, "50-bit: folded transforms with non-MAD arithmetic"),
    (16384, 7, 1 << 50, "50-bit: folded, non-MAD, L = 7 (scale_round_kernel<7, MAD = false>)"),
])
def test_uniform_chains_off_the_mad_width(ob, pie, N, L, below, what):
    o, cc = _contexts(ob, pie, N, L, T32, below)
    rng = np.random.default_rng(N + L + below.bit_length())
    check_ops(ob, pie, o, cc, rng)
    rand_run(pie, o, cc, rng)
    cc.close()


@pytest.mark.parametrize("name", NAMED)
@pytest.mark.parametrize("N,L", [(4096, 3), (16384, 5)])
def test_mixed_width_chains(ob, pie, N, L, name):
    """tests/param_chains.py: both digit-lift implementations (fused into the fast transform at logN 12, digits_kernel at 14)
    with q_i >= 2 q_j (q0_wide: the barrett128 branch), single moduli outside (2^59, 2^60) that turn off the MAD paths or the
    lazy-residue transforms for the whole context, and the edges of the one-word Barrett"""
    o, cc = _contexts(ob, pie, N, L, T32, name)
    rng = np.random.default_rng(N + L + len(name))
    check_ops(ob, pie, o, cc, rng)
    rand_run(pie, o, cc, rng)
    cc.close()


# ---- the reference's 40- and 48-bit plaintext moduli --------------------------------------------------------------------
@pytest.mark.parametrize("t", [T40, T48])
@pytest.mark.parametrize("L", [4, 6])
def test_wide_plaintext_moduli(ob, pie, t, L):
    """client.PLAINTEXT_MODULI for bitSize 40 and 48: encode / decode, the t Q constants of scale-and-round, dec_round_kernel;
    run() on a hashed database encoded on the device, then a client-harness encrypt -> run -> decrypt round trip"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    from tests.test_oracle_pie import distinct_items
    N = 16384
    o, cc = _contexts(ob, pie, N, L, t, None)
    rng = np.random.default_rng(t % 1000 + L)
    check_ops(ob, pie, o, cc, rng)
    # the hashing harness: slots with values up to t, encoded on the device
    k, e, K, E, b = 2, 12, 2, 5, 3
    sk = o.keygen(11)
    evk = o.relin_keygen(sk, 12)
    cc.load_relin_key(evk)
    d = _query(ob, o, rng, 120, 8, k, e, K, E, b)
    idx = np.stack([o.encrypt_slots(sk, d["index"][h, j], 100 + h * E + j) for h in range(K) for j in range(E)]).reshape(K, E, 2, L, N)
    minus = o.encrypt_slots(sk, d["minus"], 99)
    db = np.stack([o.encode_eval(d["slots"][h, bn, j]) for h in range(K) for bn in range(b) for j in range(E)]).reshape(K, b, E, L, N)
    masks = np.stack([o.encode_eval(d["mask_slots"][bn]) for bn in range(b)])
    op = pie.BatchedFHEHIPPIE(cc, slots=d["slots"], mask_slots=d["mask_slots"])
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    got = op.getResultList()
    assert (got == o.pie_run(idx, minus, db, masks, evk)).all()
    dec = np.stack([o.decrypt_slots(sk, got[bn], k * e)[0] for bn in range(b)])
    assert sorted(int(v) for v in ob.client_scan(d["ctab"], dec)) == sorted(int(v) for v in d["inter"])
    # client harness round trip: keys and encryption equal the oracle's, the server's result decrypts to the intersection
    cl = BatchedFHEPSIClient(cc, k, e, K, E, b)
    evk2 = cl.runSetUpPhase(keySeed=21, evalKeySeed=22)
    sk2 = o.keygen(21)
    assert (cl.sk == sk2).all() and (evk2 == o.relin_keygen(sk2, 22)).all()
    cc.load_relin_key(evk2)
    items = distinct_items(rng, t, 130)
    server, inter = items[:120], items[:5]
    clientset = np.concatenate([inter, items[120:127]])
    srv = pie.BatchedFHEHIPPIE(cc, serverSet=server, hashParams=dict(k=k, e=e, K=K, b=b, E=E))
    minus_ct, idx_ct = cl.runOfflinePhase(clientset, encSeedBase=300)
    assert (minus_ct == o.encrypt_slots(sk2, cl.plainMinus, 299)).all()
    assert (idx_ct[1, 2] == o.encrypt_slots(sk2, cl.plainIndex[1, 2], 300 + E + 2)).all()
    srv.setMinusCompareElement(minus_ct)
    srv.setIndex(idx_ct)
    srv.run()
    res = srv.getResultList().copy()
    assert (cl.decrypt(res) == np.stack([o.decrypt_slots(sk2, res[bn], k * e)[0] for bn in range(b)])).all()
    found = cl.extractIntersection(res)
    assert sorted(int(v) for v in found) == sorted(int(v) for v in inter)
    cc.close()
