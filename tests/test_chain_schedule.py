"""Chain schedule: the exact definition of run() with a limb count per product (include/piehip.h "Chain limbs",
piehip_set_chain_schedule), pinned on the CPU oracle, the noise budgets of the schedules in that section's table, and the two symbols
of the built library.

run_chain_schedule_exact is the definition.  A schedule (l_1, .., l_n) is non-increasing; product hf (1-based, hf < K) runs on
l_hf = sched[min(hf, n) - 1] limbs:
  1. stage A on all L limbs (chain_inputs of tests/test_result_relin.py);
  2. x = drop(acc[0], L -> l_1);
  3. for hf = 1 .. K - 1: where l_hf is below the level of x, x = mod_reduce(level(l_{hf-1}), x, l_hf); y = mod_reduce(top, acc[hf], l_hf);
     x = level(l_hf).mul(x, y, evk[:l_hf, :, :l_hf]) -- the last product the tensor product alone without the last relinearisation;
  4. the mask multiply with masks[:, :l_last].
mod_reduce is mod_reduce_exact of tests/test_result_limbs.py, level is level_oracle of tests/test_chain_limbs.py.
tests/test_gpu_chain_schedule.py compares the library against it bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.param_chains import T16
from tests.test_chain_limbs import level_key, level_oracle, run_chain_limbs_exact
from tests.test_result_limbs import mod_reduce_exact
from tests.test_result_relin import T32, chain_inputs, fresh_query, mask_mul_oracle, rand_limbs


def product_level(sched, hf):
    """limbs of product hf (1-based)"""
    return sched[min(hf, len(sched)) - 1]


def last_level(sched, K):
    """limbs of the last product that runs, of the mask multiply and of the result rows (K >= 2)"""
    return product_level(sched, K - 1)


def level_oracles(ob, o, sched):
    """{limbs: oracle} for every level of the schedule (the top level is o itself)"""
    return {l: (o if l == o.L else level_oracle(ob, o, l)) for l in set(sched) | {o.L}}


def schedule_layer_exact(o, levels, idx, minus, db, masks, evk, sched, beta, relin_last=True):
    """bin layer beta: [2][l_last][N], or [3][l_last][N] without the last relinearisation.  evk: the handle's key [L][2][L][N]"""
    K = idx.shape[0]
    accs = chain_inputs(o, idx, minus, db, beta)
    if K == 1:   # no product: the setting changes nothing
        return o.mul_plain(accs[0], masks[beta])
    drop = lambda ol, ct, l: ct if l == ol.L else np.ascontiguousarray(mod_reduce_exact(ol, ct, l))
    at = product_level(sched, 1)
    x = drop(o, accs[0], at)
    for hf in range(1, K):
        l = product_level(sched, hf)
        if l < at:
            x = drop(levels[at], x, l)
        at = l
        y = drop(o, accs[hf], l)
        ol = levels[l]
        if hf == K - 1 and not relin_last:
            return mask_mul_oracle(ol, ol.mul_tensor(x, y), np.ascontiguousarray(masks[beta][:l]))
        x = ol.mul(x, y, level_key(evk, l))
    return levels[at].mul_plain(x, np.ascontiguousarray(masks[beta][:at]))


def run_chain_schedule_exact(ob, o, idx, minus, db, masks, evk, sched, relin_last=True):
    """idx[K][E][2][L][N], minus[2][L][N], db[K][b][E][L][N], masks[b][L][N], evk[L][2][L][N] -> [b][2 or 3][l_last][N]
    ([b][2][L][N] at K = 1)"""
    sched = [int(v) for v in sched]
    assert 1 <= len(sched) <= 7 and all(1 <= v <= o.L for v in sched) and all(a >= b for a, b in zip(sched, sched[1:]))
    levels = level_oracles(ob, o, sched)
    return np.stack([schedule_layer_exact(o, levels, idx, minus, db, masks, evk, sched, beta, relin_last) for beta in range(db.shape[1])])


def _random_run(o, rng, K, E, b):
    q, L, N = o.q, o.L, o.N
    db, masks, evk = rand_limbs(rng, q, (K, b, E), N), rand_limbs(rng, q, (b,), N), rand_limbs(rng, q, (L, 2), N)
    idx, minus = rand_limbs(rng, q, (K, E, 2), N), rand_limbs(rng, q, (2,), N)
    return idx, minus, db, masks, evk


@pytest.mark.parametrize("N,L,t,K,E,b", [(64, 3, T16, 3, 2, 2), (64, 4, T16, 4, 2, 1), (2048, 3, T32, 3, 2, 1)])
def test_uniform_schedules_are_chain_limbs_and_a_step_is_neither(ob, N, L, t, K, E, b):
    """{L} and {L, .., L} are o.pie_run bit for bit; {x} and {x, x} are run_chain_limbs_exact(.., x); a schedule with a real step
    gives canonical rows of l_last limbs that differ from both uniform settings of its two levels"""
    o = ob.Oracle(N, L, t)
    args = _random_run(o, np.random.default_rng(N + K), K, E, b)
    full = o.pie_run(*args)
    assert (run_chain_schedule_exact(ob, o, *args, [L]) == full).all()
    assert (run_chain_schedule_exact(ob, o, *args, [L] * (K - 1)) == full).all()
    assert (run_chain_schedule_exact(ob, o, *args, [L] * 7) == full).all()
    uniform = {L: full}
    for x in range(1, L):
        uniform[x] = run_chain_limbs_exact(ob, o, *args, x)
        assert (run_chain_schedule_exact(ob, o, *args, [x]) == uniform[x]).all()
        assert (run_chain_schedule_exact(ob, o, *args, [x, x]) == uniform[x]).all()
    for hi in range(2, L + 1):
        for lo in range(1, hi):
            sched = [hi] * (K - 2) + [lo]
            got = run_chain_schedule_exact(ob, o, *args, sched)
            assert got.shape == (b, 2, lo, N) and all((got[:, :, l] < o.q[l]).all() for l in range(lo))
            assert (got != uniform[lo]).any() and (got != uniform[hi][:, :, :lo]).any(), sched
            # entries behind the last product that runs change nothing
            assert (run_chain_schedule_exact(ob, o, *args, sched + [1]) == got).all()
    got3 = run_chain_schedule_exact(ob, o, *args, [L, L - 1], relin_last=False)
    assert got3.shape == (b, 3, L - 1, N)


# The table of include/piehip.h "Chain limbs" (chain schedule): K = 3, b = 1, B = N / 2 slots, fresh queries, rng seed N + E.
# (N, L, t, E, schedules that keep the full run's plaintext, schedules that lose it)
NOISE = [
    (16384, 4, T32, 14, [(4, 4), (4, 3)], [(3, 3), (3, 2), (4, 2)]),
    (32768, 6, T32, 30, [(6, 6), (6, 5), (5, 5), (5, 4), (6, 4), (4, 4), (4, 3), (5, 3), (6, 3)], [(3, 3)]),
    (4096, 4, T16, 4, [(4, 4), (4, 3), (3, 3), (3, 2), (4, 2)], [(2, 2)]),
]


@pytest.mark.parametrize("N,L,t,E,same,wrong", NOISE)
def test_noise_budget_of_a_schedule(ob, N, L, t, E, same, wrong):
    """every schedule marked "same" decrypts to the full run's plaintext with budget left; (3,3) on the first two rows and (2,2) on
    the third do not.  All budgets are printed: the header's and DESIGN.md's table is this output"""
    K = 3
    o = ob.Oracle(N, L, t)
    sk, evk, idx, minus, db, masks = fresh_query(ob, o, np.random.default_rng(N + E), K, E, 1, N // 2)
    m_full, b_full = o.decrypt(sk, o.pie_run(idx, minus, db, masks, evk)[0])
    assert b_full >= 1
    levels = level_oracles(ob, o, range(1, L + 1))
    out = []
    for sched in same + wrong:
        row = schedule_layer_exact(o, levels, idx, minus, db, masks, evk, list(sched), 0)
        l = last_level(sched, K)
        assert row.shape == (2, l, N)
        m, bud = levels[l].decrypt(np.ascontiguousarray(sk[:l]), row)
        ok = bool((m == m_full).all())
        out.append((sched, bud, ok))
        print("N=%d L=%d t=%d E=%d K=%d schedule %s: %d bits, %s plaintext" % (N, L, t, E, K, sched, bud, "same" if ok else "WRONG"))
    for sched, bud, ok in out:
        if sched in same:
            assert ok and bud >= 1, (sched, bud)
        else:
            assert not ok, (sched, bud)
    assert dict((s, b) for s, b, _ in out)[(L, L)] == b_full


def test_library_exports_the_schedule_symbols():
    """without a GPU: the built library has both symbols, they answer a null handle with PIEHIP_EINVAL, and the prototypes of
    nested_hashing_psi_amd/_lib.py are the header's"""
    from nested_hashing_psi_amd import build
    path = build()
    from nested_hashing_psi_amd._lib import SYMBOLS, lib, u32p
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "piehip.h")).read()
    raw = C.CDLL(path if isinstance(path, str) and path.endswith(".so") else os.path.join(root, "nested_hashing_psi_amd", "libpiehip.so"))
    assert "int piehip_set_chain_schedule(piehip_handle h, const uint32_t *Lc /*[n]*/, uint32_t n);" in hdr
    assert "int piehip_get_chain_schedule(piehip_handle h, uint32_t *Lc /*[cap]*/, uint32_t cap, uint32_t *n);" in hdr
    assert hasattr(raw, "piehip_set_chain_schedule") and hasattr(raw, "piehip_get_chain_schedule")
    assert SYMBOLS["piehip_set_chain_schedule"] == (C.c_int, [C.c_void_p, u32p, C.c_uint32])
    assert SYMBOLS["piehip_get_chain_schedule"] == (C.c_int, [C.c_void_p, u32p, C.c_uint32, u32p])
    L = lib()
    assert L.piehip_version() == 102    # new symbols, no new number
    sched = (C.c_uint32 * 2)(2, 1)
    n = C.c_uint32(9)
    EINVAL = -1
    assert L.piehip_set_chain_schedule(None, sched, 2) == EINVAL and L.piehip_last_error()
    assert L.piehip_get_chain_schedule(None, sched, 2, C.byref(n)) == EINVAL
    assert n.value == 9 and list(sched) == [2, 1]
