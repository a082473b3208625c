"""Chain limbs: the exact definition of run() with the product chain on a prefix of the prime chain (include/piehip.h "Chain
limbs"), pinned on the CPU oracle, and what the early limb drop does to the noise budget.

run_chain_limbs_exact is the definition: stage A on all L limbs (chain_inputs of tests/test_result_relin.py), every accumulator
dropped to its first Lc limbs (mod_reduce_exact of tests/test_result_limbs.py), then the product chain and the mask multiply of
BatchedFHEHIPPIE::run() (reference BatchedFHEHIPPIE.cpp:117-126) on the level oracle (N, Lc, t, q[:Lc], p[:Lc+1]) with the key
evk[:Lc, :, :Lc] and the masks' first Lc limbs.  tests/test_gpu_chain_limbs.py compares the library against it bit for bit.
"""
import numpy as np
import pytest

from tests.param_chains import T16
from tests.test_result_limbs import mod_reduce_exact
from tests.test_result_relin import T32, chain_inputs, fresh_query, mask_mul_oracle, rand_limbs


def level_oracle(ob, o, Lc):
    """the level context of the first Lc limbs: (N, Lc, t, q[:Lc], p[:Lc+1])"""
    return ob.Oracle(o.N, Lc, o.t, np.ascontiguousarray(o.q[:Lc]), np.ascontiguousarray(o.p[:Lc + 1]))


def level_key(evk, Lc):
    """evk[i][c][j] restricted to i, j < Lc (None stays None: K = 2 without the last relinearisation needs no key)"""
    return None if evk is None else np.ascontiguousarray(evk[:Lc, :, :Lc])


def chain_layer_exact(o, ol, idx, minus, db, masks, evk, Lc, beta, relin_last=True):
    """bin layer beta: [2][Lc][N], or [3][Lc][N] without the last relinearisation.  evk: the LEVEL's key (level_key)"""
    K = idx.shape[0]
    accs = chain_inputs(o, idx, minus, db, beta)
    if K == 1:   # no product: the setting changes nothing
        return o.mul_plain(accs[0], masks[beta])
    accs = [np.ascontiguousarray(mod_reduce_exact(o, a, Lc)) for a in accs] if Lc < o.L else accs
    mask = np.ascontiguousarray(masks[beta][:Lc])
    x = accs[0]
    for h in range(1, K - 1):
        x = ol.mul(x, accs[h], evk)
    if relin_last:
        return ol.mul_plain(ol.mul(x, accs[K - 1], evk), mask)
    return mask_mul_oracle(ol, ol.mul_tensor(x, accs[K - 1]), mask)


def run_chain_limbs_exact(ob, o, idx, minus, db, masks, evk, Lc, relin_last=True):
    """idx[K][E][2][L][N], minus[2][L][N], db[K][b][E][L][N], masks[b][L][N], evk[L][2][L][N] (or None) ->
    [b][2 or 3][Lc][N] ([b][2][L][N] at K = 1)"""
    ol = o if Lc == o.L else level_oracle(ob, o, Lc)
    k = level_key(evk, Lc)
    return np.stack([chain_layer_exact(o, ol, idx, minus, db, masks, k, Lc, beta, relin_last) for beta in range(db.shape[1])])


@pytest.mark.parametrize("N,L,t,K,E,b", [(64, 2, T16, 2, 3, 2), (64, 3, T16, 3, 2, 2), (2048, 3, T32, 2, 3, 1)])
def test_all_limbs_is_the_reference_run(ob, N, L, t, K, E, b):
    """(a) Lc = L is o.pie_run bit for bit, on random limbs; and Lc < L gives canonical rows of Lc limbs that differ from a
    truncation of the full run (the drop is not a projection)"""
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(N + K)
    q = o.q
    db, masks, evk = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (L, 2), N)
    idx, minus = rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)
    full = o.pie_run(idx, minus, db, masks, evk)
    assert (run_chain_limbs_exact(ob, o, idx, minus, db, masks, evk, L) == full).all()
    for Lc in range(1, L):
        got = run_chain_limbs_exact(ob, o, idx, minus, db, masks, evk, Lc)
        assert got.shape == (b, 2, Lc, N) and all((got[:, :, l] < q[l]).all() for l in range(Lc))
        assert (got != full[:, :, :Lc]).any()
        got3 = run_chain_limbs_exact(ob, o, idx, minus, db, masks, evk if K > 2 else None, Lc, relin_last=False)
        assert got3.shape == (b, 3, Lc, N)


def test_level_oracle_is_the_prefix_context(ob):
    o = ob.Oracle(4096, 4, T32)
    ol = level_oracle(ob, o, 3)
    assert (ol.q == o.q[:3]).all() and (ol.p == o.p[:4]).all() and ol.t == o.t


def _decrypt_level(ob, o, sk, row, limbs):
    ol = o if limbs == o.L else level_oracle(ob, o, limbs)
    return ol.decrypt(np.ascontiguousarray(sk[:limbs]), row)


# the first two rows of the table in include/piehip.h "Chain limbs": (N, L, t, E, Lc, the keep columns)
ROWS = [(16384, 4, T32, 14, 3, (2, 1)), (4096, 3, T16, 6, 2, (1,))]


@pytest.mark.parametrize("N,L,t,E,Lc,keeps", ROWS)
def test_chain_on_fewer_limbs_decrypts_to_the_full_runs_plaintext(ob, N, L, t, E, Lc, keeps):
    """(b) K = 2, fresh queries: the chain on L - 1 limbs decrypts to the full run's plaintext with budget left, and so do its
    keep columns; the budgets are printed"""
    o = ob.Oracle(N, L, t)
    sk, evk, idx, minus, db, masks = fresh_query(ob, o, np.random.default_rng(N + E), 2, E, 1, N // 2)
    m_full, b_full = o.decrypt(sk, o.pie_run(idx, minus, db, masks, evk)[0])
    row = run_chain_limbs_exact(ob, o, idx, minus, db, masks, evk, Lc)[0]
    m, bud = _decrypt_level(ob, o, sk, row, Lc)
    print("N=%d L=%d t=%d E=%d: budget full chain %d bits, chain limbs %d: %d bits" % (N, L, t, E, b_full, Lc, bud))
    assert b_full >= 1 and bud >= 1 and (m == m_full).all()
    ol = level_oracle(ob, o, Lc)
    for keep in keeps:
        mk, bk = _decrypt_level(ob, o, sk, mod_reduce_exact(ol, row, keep), keep)
        print("N=%d L=%d t=%d E=%d: chain limbs %d then keep %d: %d bits" % (N, L, t, E, Lc, keep, bk))
        assert bk >= 1 and (mk == m_full).all()


def test_degree_two_results_at_a_lower_level_decrypt(ob):
    """(c) the degree-2 form -- mul_tensor on the level oracle plus the mask multiply -- on the first row, no key"""
    N, L, t, E, Lc, _ = ROWS[0]
    o = ob.Oracle(N, L, t)
    sk, evk, idx, minus, db, masks = fresh_query(ob, o, np.random.default_rng(N + E), 2, E, 1, N // 2)
    m_full, b_full = o.decrypt(sk, o.pie_run(idx, minus, db, masks, evk)[0])
    row3 = run_chain_limbs_exact(ob, o, idx, minus, db, masks, None, Lc, relin_last=False)[0]
    assert row3.shape == (3, Lc, N)
    m3, b3 = _decrypt_level(ob, o, sk, row3, Lc)
    print("N=%d L=%d t=%d E=%d: degree-2 row at chain limbs %d: %d bits (full chain, relinearised: %d)" % (N, L, t, E, Lc, b3, b_full))
    assert b3 >= 1 and (m3 == m_full).all()
