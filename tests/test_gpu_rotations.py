"""GPU parity of the rotation path over the parameter range piehip_create accepts: EvalAutomorphism (permute_kernel and the
BV key switch with a rotation key), the client's rotation keys and the rotation-based operator FHEHIPPIE
(bcast_mul_plain_kernel, rot_prepare_kernel, sum_mul_plain_kernel, the merge key switch with one key per bin).

The key switch picks its kernels by ring and moduli: the digit lift fused into the forward transform (logN <= 14) or
digits_kernel plus a separate transform (N = 32768, 65536); relin_mac_kernel's column accumulators when every modulus lies in
(2^59, 2^60), its 128-bit sums otherwise; two ciphertext rows per thread where at least two rows share a key.  Every point
is compared bit for bit with the CPU oracle on the same moduli, and the decrypted result with a plain model: the rotated
slots, or tests/test_oracle_pie.fhepie_model.
"""
import numpy as np
import pytest

from tests.param_chains import NAMED, T16, T32, T40, T48
from tests.test_gpu_envelope import _contexts
from tests.test_gpu_parity import rand_limbs
from tests.test_oracle_pie import fhepie_model, rotation_indices

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def rotate_slots(x, N, g):
    """the slots of sigma_g applied to a packing of x: rows of N / 2 rotated left by r for g = 5^r, swapped for g = 2N - 1"""
    h = N // 2
    rows = np.asarray(x).reshape(2, h)
    if g == 2 * N - 1:
        return rows[::-1].reshape(N)
    r = next(r for r in range(h) if pow(5, r, 2 * N) == g)
    return np.roll(rows, -r, axis=1).reshape(N)


# ---- EvalAutomorphism ---------------------------------------------------------------------------------------------------
def check_automorphism(o, cc, rng, decrypts=True):
    """rotation indices +-1, +-2, +-(N/2 - 1) and g = 2N - 1; a fresh encryption (bit-exact and decrypted) and the same with
    c1 all 0 and all q - 1 (bit-exact); even g and g >= 2N are refused"""
    N, L, t = o.N, o.L, o.t
    assert (cc.moduli == o.moduli).all()
    sk = o.keygen(3)
    x = rng.integers(-(t // 2), t // 2 + 1, N)
    c = o.encrypt_slots(sk, x, 4)
    edge = [c.copy(), c.copy()]
    edge[0][1] = 0
    edge[1][1] = (o.q - np.uint64(1))[:, None]
    rots = sorted({1, 2, N // 2 - 1, -1, -2, -(N // 2 - 1)} - {0})
    gs = [(r, o.rot_index(r)) for r in rots] + [(None, 2 * N - 1)]
    for n, (r, g) in enumerate(gs):
        if r is not None:
            assert cc.rotation_galois(r) == g
        rk = o.rot_keygen(sk, g, 60 + n)
        got = cc.EvalAutomorphism(c, g, rk)
        assert (got == o.automorph(c, g, rk)).all(), "rotation %s (g = %d)" % (r, g)
        if decrypts:
            dec, budget = o.decrypt_slots(sk, got, N)
            assert budget > 0 and (dec == rotate_slots(x, N, g)).all(), "rotation %s (g = %d)" % (r, g)
        for e in edge:
            assert (cc.EvalAutomorphism(e, g, rk) == o.automorph(e, g, rk)).all(), "rotation %s, c1 = 0 / q - 1" % r
    for bad in (4, 2 * N - 2, 2 * N + 1, 4 * N + 1):
        with pytest.raises(ValueError, match="odd and < 2N"):
            cc.EvalAutomorphism(c, bad, rk)


@pytest.mark.parametrize("N", [8, 16, 32])
@pytest.mark.parametrize("L", [1, 2])
def test_automorphism_smallest_rings(ob, pie, N, L):
    """rows of 4, 8 and 16 slots (rotation_galois reduces the index mod N/2).  At L = 1 the one BV digit is as wide as Q: the
    switched ciphertext is bit-exact but noise"""
    o, cc = _contexts(ob, pie, N, L, T16, None)
    check_automorphism(o, cc, np.random.default_rng(N + L), decrypts=L > 1)
    cc.close()


@pytest.mark.parametrize("N,L,t,chain", [
    (16384, 7, T32, None),        # seven digits, the digit lift fused into the transform
    (32768, 7, T32, None),        # digits_kernel + a separate transform (logN > 14)
    (65536, 3, T32, None),
    (65536, 7, T32, None),
    (4096, 3, T32, 1 << 61),      # 61-bit: relin_mac_kernel without column accumulators
    (32768, 3, T32, 1 << 61),     # ... with digits_kernel
    (16384, 5, T32, 1 << 50),     # 50-bit
] + [(4096, 3, T32, name) for name in NAMED] + [
    (16384, 4, T40, None),
    (16384, 4, T48, None),
])
def test_automorphism_envelope(ob, pie, N, L, t, chain):
    o, cc = _contexts(ob, pie, N, L, t, chain)
    check_automorphism(o, cc, np.random.default_rng(N + L + t % 97))
    cc.close()


# ---- FHEHIPPIE ----------------------------------------------------------------------------------------------------------
def rot_keys(o, sk, E, seed):
    return {r: o.rot_keygen(sk, o.rot_index(r), seed + i) for i, r in enumerate(rotation_indices(E))}


def fhepie_inputs(o, sk, rng, npie, K, E, seed=300):
    """random tables [npie][K][E][E] and index vectors [npie][K][E + 1] (full range of Z_t: every term of the sums counts), the
    index vectors encrypted"""
    t = o.t
    tbl = rng.integers(0, t, (npie, K, E, E), dtype=np.uint64)
    index = rng.integers(-(t // 2), t // 2 + 1, (npie, K, E + 1))
    idx = np.stack([o.encrypt_slots(sk, index[i, hf], seed + i * K + hf) for i in range(npie) for hf in range(K)])
    return tbl, index, idx.reshape(npie, K, 2, o.L, o.N)


def packed_rows(tbl, perm):
    """the rows FHEHIPPIE packs from the table [K][b][E] of one operator (FHEHIPPIE.cpp:41-51): bin bn of hash function hf is
    row perm[bn] (the bin permutation permVec2), its E cells then a 1 for the client's -x"""
    K, b, E = tbl.shape
    rows = np.ones((K, b, E + 1), dtype=np.int64)
    for hf in range(K):
        for bn in range(b):
            rows[hf, perm[bn], :E] = tbl[hf, bn].astype(np.int64)
    return rows


def check_fhepie(ob, o, sk, op, idx, index, tbl, keys, res=None, decrypts=True):
    """every operator of the batch: the rows packed from the caller's table, the result bit for bit against ob.fhe_pie_run
    (after undoing the result permutation), and decrypted against fhepie_model"""
    if res is None:
        res = op.getResultList()
    res = res.reshape(op.npie, op.K, 2, o.L, o.N)
    tbl = np.asarray(tbl).reshape(op.npie, op.K, op.b, op.E)
    for i in range(op.npie):
        rows = packed_rows(tbl[i], op.permVec2[i])
        assert (op.slots[i] == rows).all(), "operator %d: packed rows" % i
        got = res[i][op.permutationVector[i]]
        want = ob.fhe_pie_run(o, idx[i], rows, op.masks[i], keys)
        assert (got == want).all(), "operator %d" % i
        if not decrypts:
            continue
        model = fhepie_model(index[i], rows, op.masks[i], o.N, o.t)
        for hf in range(op.K):
            dec, budget = o.decrypt_slots(sk, got[hf], o.N)
            assert budget > 0
            assert [int(v) % o.t for v in dec] == model[hf], "operator %d, hash function %d" % (i, hf)


# Three plaintext products (table row, EvalMerge's slot-0 mask, the random mask) each multiply the noise by about t sqrt(N);
# the moduli below leave room for that, except at N = 65536, L = 3, where t = 2^32 (the smallest t = 1 mod 2^17) and
# Q = 2^180 do not: that point is bit-exact only.
@pytest.mark.parametrize("N,L,t,chain,K,E,npie,perm", [
    (8, 3, T16, None, 2, 3, 1, False),        # rows of 4 slots
    (16, 3, T16, None, 2, 7, 2, False),       # E + 1 fills the row: 2^R = 8 is the row length
    (16, 3, T16, None, 2, 4, 3, False),       # power of two: slot E is left out of the sum
    (32, 3, T16, None, 1, 5, 5, True),
    (4096, 3, T16, None, 2, 1, 2, False),     # b = E = 1: no rotate-and-add step, no merge
    (4096, 3, T16, None, 2, 2, 3, False),     # two rows per thread in the merge, the last block unpaired
    (4096, 3, T16, None, 1, 8, 1, False),
    (4096, 3, T16, None, 1, 16, 2, False),
    (4096, 3, T16, None, 2, 7, 5, True),      # b = 7, five operators
    (16384, 7, T32, None, 2, 3, 2, False),
    (32768, 6, T32, None, 2, 3, 1, False),    # digits_kernel (logN > 14)
    (65536, 3, T32, None, 1, 3, 3, False),
    (4096, 4, T32, 1 << 61, 2, 5, 3, True),   # relin_mac_kernel without column accumulators, one key per merge row
    (32768, 4, T32, 1 << 61, 1, 3, 2, False),
    (4096, 4, T16, "q_narrow_p_wide", 2, 5, 2, False),
    (4096, 4, T32, "one_p_61", 1, 6, 3, False),
    (4096, 5, T40, None, 2, 5, 2, False),
    (4096, 5, T48, None, 2, 3, 3, False),
])
def test_fhepie_envelope(ob, pie, N, L, t, chain, K, E, npie, perm):
    o, cc = _contexts(ob, pie, N, L, t, chain)
    rng = np.random.default_rng(N * 7 + L * 5 + E * 3 + npie)
    sk = o.keygen(1)
    keys = rot_keys(o, sk, E, 50)
    for r in keys:
        assert cc.rotation_galois(r) == o.rot_index(r)
    if keys:                                  # b = 1 needs none
        cc.load_rotation_keys(keys)
    tbl, index, idx = fhepie_inputs(o, sk, rng, npie, K, E)
    op = pie.FHEHIPPIE(cc, tbl, perm_seed=7 if perm else False, mask_seed=8)
    op.setIndex(idx)
    op.run()
    check_fhepie(ob, o, sk, op, idx, index, tbl, keys, decrypts=(N, L) != (65536, 3))
    cc.close()


# ---- the client harness' keys -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,t,chain,E", [
    (4096, 7, T32, None, 5),
    (8, 3, T16, None, 3),
    (65536, 7, T32, None, 2),                 # b = 2: the two keys (rotations 1 and -1) only
    (4096, 4, T32, "q0_wide", 5),
])
def test_client_rotation_keys(ob, pie, N, L, t, chain, E):
    """BatchedFHEPSIClient.rotationKeyGen == po_rot_keygen key for key; then FHEHIPPIE end to end under the client's keys,
    decrypted by the client"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    o, cc = _contexts(ob, pie, N, L, t, chain)
    K, npie = 2, 2
    cl = BatchedFHEPSIClient(cc, 1, 1, K, E, E)
    cl.runSetUpPhase(keySeed=21, evalKeySeed=22)
    sk = o.keygen(21)
    assert (cl.sk == sk).all()
    keys = cl.rotationKeyGen(E, seedBase=50)
    assert sorted(keys) == sorted(rotation_indices(E))
    for i, r in enumerate(rotation_indices(E)):
        assert (keys[r] == o.rot_keygen(sk, o.rot_index(r), 50 + i)).all(), "rotation %d" % r
    if N == 65536:
        cc.close()
        return
    cc.load_rotation_keys(keys)
    rng = np.random.default_rng(N + L)
    tbl = rng.integers(0, t, (npie, K, E, E), dtype=np.uint64)
    index = rng.integers(-(t // 2), t // 2 + 1, (npie, K, E + 1))
    idx = cl._encrypt(index.reshape(npie * K, E + 1), 300 + np.arange(npie * K)).reshape(npie, K, 2, L, N)
    op = pie.FHEHIPPIE(cc, tbl, perm_seed=5, mask_seed=6)
    op.setIndex(idx)
    op.run()
    res = op.getResultList()
    dec = cl.decrypt(res.reshape(npie * K, 2, L, N), nslots=N).reshape(npie, K, N)
    for i in range(npie):
        model = fhepie_model(index[i], packed_rows(tbl[i], op.permVec2[i]), op.masks[i], N, t)
        assert [[int(v) % t for v in row] for row in dec[i][op.permutationVector[i]]] == model
    check_fhepie(ob, o, sk, op, idx, index, tbl, keys, res)
    cc.close()


# ---- handle state -------------------------------------------------------------------------------------------------------
def test_fhepie_handle_state(ob, pie):
    """one context: a second table with another b (the merge keys fp_negkeys are rebuilt for it), rotation keys reloaded
    under new seeds between two runs, then BatchedFHEHIPPIE.run() and FHEHIPPIE.run() alternating without a host wait"""
    N, L, t, K = 4096, 3, T16, 2
    o, cc = _contexts(ob, pie, N, L, t, None)
    rng = np.random.default_rng(4242)
    sk = o.keygen(1)
    keys = rot_keys(o, sk, 6, 50)            # covers b = 3 and b = 6
    cc.load_rotation_keys(keys)
    for E, npie in ((6, 2), (3, 3), (6, 1)):
        tbl, index, idx = fhepie_inputs(o, sk, rng, npie, K, E)
        op = pie.FHEHIPPIE(cc, tbl, perm_seed=False, mask_seed=E)
        op.setIndex(idx)
        op.run()
        check_fhepie(ob, o, sk, op, idx, index, tbl, keys)

    # new keys for the same indices: the next run follows them
    first = op.getResultList().copy()
    keys2 = rot_keys(o, sk, 6, 90)
    cc.load_rotation_keys(keys2)
    op.run()
    second = op.getResultList()
    assert (second != first).any()
    check_fhepie(ob, o, sk, op, idx, index, tbl, keys2, second)

    # the hot path and the rotation operator on one handle, queued back to back
    Kb, Eb, b = 2, 3, 4
    db, masks, evk = rand_limbs(rng, o.q, (Kb, b, Eb), N), rand_limbs(rng, o.q, (b,), N), rand_limbs(rng, o.q, (L, 2), N)
    cc.load_relin_key(evk)
    bop = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
    bidx, bminus = rand_limbs(rng, o.q, (Kb, Eb, 2), N), rand_limbs(rng, o.q, (2,), N)
    bop.setIndex(bidx)
    bop.setMinusCompareElement(bminus)
    tbl, index, idx = fhepie_inputs(o, sk, rng, 3, K, 5, seed=500)
    op = pie.FHEHIPPIE(cc, tbl, perm_seed=False, mask_seed=9)
    op.setIndex(idx)
    for _ in range(2):
        bop.run(sync=False)
        op.run()
    bop.run(sync=False)
    bop.sync()
    check_fhepie(ob, o, sk, op, idx, index, tbl, keys2)
    assert (bop.getResultList() == o.pie_run(bidx, bminus, db, masks, evk)).all()
    cc.close()


def test_fhepie_refusals_at_the_smallest_ring(ob, pie):
    """N = 8: a row holds 4 slots.  E + 1 > N / 2 is refused, and so are rotation indices that are multiples of the row length
    (Galois element 1), by the server and by the client"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    N, L, t = 8, 3, T16
    o, cc = _contexts(ob, pie, N, L, t, None)
    with pytest.raises(ValueError, match="exceed one row"):
        pie.FHEHIPPIE(cc, np.ones((2, 4, 4), dtype=np.uint64))
    sk = o.keygen(1)
    key = o.rot_keygen(sk, o.rot_index(1), 5)
    for r in (4, -4, 8):
        assert cc.rotation_galois(r) == 1
        with pytest.raises(ValueError, match="multiple of the row length"):
            cc.load_rotation_keys({r: key})
    cl = BatchedFHEPSIClient(cc, 1, 1, 2, 3, 3)
    cl.runSetUpPhase()
    with pytest.raises(ValueError, match="multiple of the row length"):
        cl.rotationKeyGen(5)        # EvalSum's rotation by 4
    # E = 3 (E + 1 = N / 2) still runs
    keys = rot_keys(o, sk, 3, 50)
    cc.load_rotation_keys(keys)
    rng = np.random.default_rng(8)
    tbl, index, idx = fhepie_inputs(o, sk, rng, 1, 2, 3)
    op = pie.FHEHIPPIE(cc, tbl, perm_seed=False, mask_seed=3)
    op.setIndex(idx)
    op.run()
    check_fhepie(ob, o, sk, op, idx, index, tbl, keys)
    cc.close()
