"""Result relinearisation: the exact definition of run() without the last relinearisation (include/piehip.h "Result
relinearisation"), pinned on the CPU oracle, and what the third component does to the noise budget.

run_deg2_exact is the definition: the composition of BatchedFHEHIPPIE::run() (reference BatchedFHEHIPPIE.cpp:101-126) from the
oracle's primitives with the LAST ciphertext product left as its three-component tensor result and the mask multiplied into all
three components, limb by limb, in Python integers.  tests/test_gpu_result_relin.py compares the library against it bit for bit.
"""
import numpy as np
import pytest

from tests.param_chains import T16
from tests.test_result_limbs import mod_reduce_exact, reduced_oracle

T32 = 4296540161


def rand_limbs(rng, moduli, shape_prefix, N):
    out = np.zeros(tuple(shape_prefix) + (len(moduli), N), dtype=np.uint64)
    for i, m in enumerate(moduli):
        out[..., i, :] = rng.integers(0, int(m), tuple(shape_prefix) + (N,), dtype=np.uint64)
    return out


def mask_mul(o, ct, mask):
    """every component of ct[c][L][N] times the plaintext mask[L][N], limb by limb, in Python integers"""
    out = np.zeros_like(ct)
    for l in range(o.L):
        q = int(o.q[l])
        m = mask[l].astype(object)
        for c in range(ct.shape[0]):
            out[c, l] = (ct[c, l].astype(object) * m % q).astype(np.uint64)
    return out


def chain_inputs(o, idx, minus, db, beta):
    """the K accumulators of bin layer beta (.cpp:101-116): sum_j idx[h][j] (.) db[h][beta][j] + minus"""
    K, E = idx.shape[0], idx.shape[1]
    accs = []
    for h in range(K):
        acc = o.mul_plain(idx[h, 0], db[h, beta, 0])
        for j in range(1, E):
            acc = o.add(acc, o.mul_plain(idx[h, j], db[h, beta, j]))
        accs.append(o.add(acc, minus))
    return accs


def mask_mul_oracle(o, ct, mask):
    """mask_mul through the oracle's ciphertext-by-plaintext product, two components at a time (pinned against mask_mul below;
    what the GPU tests use on their larger rings)"""
    return np.concatenate([o.mul_plain(np.ascontiguousarray(ct[:2]), mask), o.mul_plain(np.stack([ct[2], ct[2]]), mask)[:1]])


def layer_rows(o, idx, minus, db, masks, evk, beta, reference=False, mask=mask_mul):
    """bin layer beta: (the three-component row, the reference's relinearised row or None)"""
    K = idx.shape[0]
    assert K >= 2
    accs = chain_inputs(o, idx, minus, db, beta)
    x = accs[0]
    for h in range(1, K - 1):
        x = o.mul(x, accs[h], evk)
    t3 = o.mul_tensor(x, accs[K - 1])
    return mask(o, t3, masks[beta]), (o.mul_plain(o.relin(t3, evk), masks[beta]) if reference else None)


def run_deg2_exact(o, idx, minus, db, masks, evk, relin_last=False):
    """idx[K][E][2][L][N], minus[2][L][N], db[K][b][E][L][N], masks[b][L][N] -> [b][3][L][N] (K >= 2; evk may be None at K = 2).
    relin_last: end with o.relin + o.mul_plain instead -- the reference's run(), [b][2][L][N] (pinned against o.pie_run below)"""
    rows = [layer_rows(o, idx, minus, db, masks, evk, beta, reference=relin_last) for beta in range(db.shape[1])]
    return np.stack([r[1] if relin_last else r[0] for r in rows])


@pytest.mark.parametrize("N,L,t,K,E,b", [(64, 2, T16, 2, 3, 2), (64, 2, T16, 3, 2, 2), (2048, 3, T32, 2, 3, 2), (2048, 3, T32, 3, 2, 1)])
def test_composition_is_the_reference_run(ob, N, L, t, K, E, b):
    """(a) the same composition, ended with relin + mul_plain, is o.pie_run bit for bit (random limbs)"""
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(N + K)
    q = o.q
    db, masks, evk = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (L, 2), N)
    idx, minus = rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)
    assert (run_deg2_exact(o, idx, minus, db, masks, evk, relin_last=True) == o.pie_run(idx, minus, db, masks, evk)).all()
    got = run_deg2_exact(o, idx, minus, db, masks, evk if K > 2 else None)
    assert got.shape == (b, 3, L, N) and all((got[:, :, l] < q[l]).all() for l in range(L))
    fast = np.stack([layer_rows(o, idx, minus, db, masks, evk, beta, mask=mask_mul_oracle)[0] for beta in range(b)])
    assert (fast == got).all()


def fresh_query(ob, o, rng, K, E, b, B):
    """fresh secret-key queries against a random database and random masks: everything run() takes, and the keys"""
    N, L, t = o.N, o.L, o.t
    sk = o.keygen(int(rng.integers(1, 1 << 30)))
    evk = o.relin_keygen(sk, int(rng.integers(1, 1 << 30)))
    half = t // 2
    slots = lambda n: rng.integers(-half, half, (n, B), dtype=np.int64)
    db = np.stack([o.encode_eval(v) for v in slots(K * b * E)]).reshape(K, b, E, L, N)
    masks = np.stack([o.encode_eval(v) for v in slots(b)])
    idx = np.stack([o.encrypt_slots(sk, v, 100 + i) for i, v in enumerate(slots(K * E))]).reshape(K, E, 2, L, N)
    minus = o.encrypt_slots(sk, slots(1)[0], 99)
    return sk, evk, idx, minus, db, masks


@pytest.mark.parametrize("N,L,t,K,E", [(64, 2, T16, 2, 2), (2048, 3, T32, 2, 3), (2048, 3, T16, 3, 2)])
def test_three_components_decrypt_to_the_relinearised_plaintext(ob, N, L, t, K, E):
    """(b) o.decrypt of the three-component row gives the plaintext of the relinearised row, with budget left.  (K = 3 is two
    chained ciphertext products between plaintext products: on three 60-bit limbs that leaves budget for the 17-bit t, not for
    the 33-bit one -- relinearised or not.)"""
    o = ob.Oracle(N, L, t)
    sk, evk, idx, minus, db, masks = fresh_query(ob, o, np.random.default_rng(N + 3 * K), K, E, 1, N // 2)
    row3 = run_deg2_exact(o, idx, minus, db, masks, evk)[0]
    row2 = o.pie_run(idx, minus, db, masks, evk)[0]
    m3, b3 = o.decrypt(sk, row3)
    m2, b2 = o.decrypt(sk, row2)
    print("N=%d L=%d K=%d: budget degree-2 %d bits, relinearised %d bits" % (N, L, K, b3, b2))
    assert (m3 == m2).all()
    assert b3 >= 1 and b2 >= 1


@pytest.mark.parametrize("N,L,t,E", [(16384, 4, T32, 14), (4096, 3, T16, 6)])
def test_noise_budget_after_the_limb_drop(ob, N, L, t, E):
    """(c) the two parameter rows of DESIGN.md section 4d (C3's, and a small one), K = 2: after the limb drop to every keep < L the
    degree-2 row still decrypts to the relinearised row's plaintext; the third component's rounding error, multiplied by s^2, costs
    budget -- never gains any"""
    o = ob.Oracle(N, L, t)
    sk, evk, idx, minus, db, masks = fresh_query(ob, o, np.random.default_rng(N + E), 2, E, 1, N // 2)
    row3 = run_deg2_exact(o, idx, minus, db, masks, None)[0]
    row2 = o.pie_run(idx, minus, db, masks, evk)[0]
    m3, b3 = o.decrypt(sk, row3)
    m2, b2 = o.decrypt(sk, row2)
    print("N=%d L=%d t=%d E=%d full chain: budget degree-2 %d bits, relinearised %d bits" % (N, L, t, E, b3, b2))
    assert (m3 == m2).all() and b3 >= 1 and b3 <= b2
    for keep in range(1, L):
        ok = reduced_oracle(ob, o, keep)
        skk = np.ascontiguousarray(sk[:keep])
        r3, c3 = ok.decrypt(skk, mod_reduce_exact(o, row3, keep))
        r2, c2 = ok.decrypt(skk, mod_reduce_exact(o, row2, keep))
        print("N=%d L=%d t=%d E=%d keep=%d: budget degree-2 %d bits, relinearised %d bits" % (N, L, t, E, keep, c3, c2))
        assert (r3 == r2).all()
        assert c3 >= 1 and c2 >= 1 and c3 <= c2
