"""Noise budgets from the device client and the schedule chooser, without a GPU: the two symbols of the built library, the readout
against the oracle's formula, the planted ciphertexts of tests/budget_columns.py pinned on the oracle, and the pure part of
nested_hashing_psi_amd/schedule.py on the oracle's own table.  tests/test_gpu_noise_budget.py holds the device to the same numbers.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import budget_columns as bc
from tests.param_chains import T16, T32


def test_library_exports_the_budget_symbols():
    """the built library has both symbols, the prototypes of nested_hashing_psi_amd/_lib.py are the header's, a null handle answers
    PIEHIP_EINVAL and writes nothing"""
    from nested_hashing_psi_amd import build
    path = build()
    from nested_hashing_psi_amd._lib import SYMBOLS, i32p, i64p, lib, u64p
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "piehip.h")).read()
    raw = C.CDLL(path)
    assert ("int piehip_client_decrypt_budget(piehip_handle h, const uint64_t *sk, const uint64_t *ct /*[nct][ncomp][L][N]*/,\n"
            "                                 uint32_t nct, uint32_t ncomp /*2 or 3*/, uint32_t B,\n"
            "                                 int64_t *slots /*[nct][B]; null iff B == 0*/,\n"
            "                                 int32_t *budget /*[nct]*/, uint64_t *max_dist /*[nct], may be null*/);\n"
            "int piehip_budget_from_distance(uint64_t max_dist);   /* host only, no handle */\n") in hdr
    assert hasattr(raw, "piehip_client_decrypt_budget") and hasattr(raw, "piehip_budget_from_distance")
    assert SYMBOLS["piehip_client_decrypt_budget"] == (C.c_int, [C.c_void_p, u64p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, i64p, i32p, u64p])
    assert SYMBOLS["piehip_budget_from_distance"] == (C.c_int, [C.c_uint64])
    L = lib()
    assert L.piehip_version() == 102    # new symbols, no new number
    EINVAL = -1
    sk, ct, md = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 1)(77)
    slots, budget = (C.c_int64 * 1)(55), (C.c_int32 * 1)(66)
    assert L.piehip_client_decrypt_budget(None, sk, ct, 1, 2, 1, slots, budget, md) == EINVAL and L.piehip_last_error()
    assert (slots[0], budget[0], md[0]) == (55, 66, 77)


def test_budget_from_distance_is_the_oracles_readout():
    """piehip_budget_from_distance at 0, 1 and around every power of two against po_decrypt's formula (bc.budget_readout)"""
    from nested_hashing_psi_amd._lib import lib
    f = lib().piehip_budget_from_distance
    ds = [0, 1] + [v for j in range(1, 64) for v in ((1 << j) - 1, 1 << j, (1 << j) + 1)]
    assert max(ds) == (1 << 63) + 1
    for d in ds:
        assert f(d) == bc.budget_readout(d), hex(d)
    assert (f(0), f(1), f(2), f(3), f(4)) == (58, 58, 57, 57, 56)
    assert f((1 << 58) - 1) == 1 and f(1 << 58) == 0 and f((1 << 64) - 1) == 0
    # a distance never exceeds 2^59; the readout there and beyond is 0, not negative


# (N, L, t): the four contexts the planted column was checked on, and L = 7 of the default chain
PLANTED = [(64, 1, T16), (64, 3, T32), (512, 4, T16), (256, 2, T32), (64, 7, T32)]


@pytest.mark.parametrize("N,L,t", PLANTED)
def test_planted_budgets_on_the_oracle(ob, N, L, t):
    """o.decrypt reports exactly k for the planted column, every k in 0..50, both signs, the loud coefficient first and last, with
    c1 = 0 and with c1 (and c2) uniform under a sampled key; and 58 for the quiet polynomial in the same forms"""
    from tests import coeff_columns as ccol
    o = ob.Oracle(N, L, t)
    rng = np.random.default_rng(N + L)
    sk = o.keygen(61 + L)
    forms = [lambda X: ccol.phase_ct(o, X), lambda X: bc.sampled_ct(o, X, sk, rng, 2), lambda X: bc.sampled_ct(o, X, sk, rng, 3)]
    for form in forms:
        assert o.decrypt(sk, form(bc.quiet_poly(o)))[1] == bc.QUIET
    for k in range(bc.K_MAX + 1):
        for sign in (1, -1):
            for pos in (0, N - 1):
                X = bc.planted_poly(o, k, sign, pos)
                for f, form in enumerate(forms):
                    got = o.decrypt(sk, form(X))[1]
                    assert got == k, "k = %d, sign %d, coefficient %d, form %d: the oracle reads %d" % (k, sign, pos, f, got)


def test_candidate_schedules():
    from nested_hashing_psi_amd.schedule import candidate_schedules
    c = candidate_schedules(4, 3)
    assert len(c) == 10 and len(set(c)) == 10 and c[0] == (4, 4)
    assert sorted(c) == sorted((a, b) for a in range(1, 5) for b in range(1, a + 1))
    c = candidate_schedules(7, 4)
    assert len(c) == 84 and len(set(c)) == 84
    assert all(len(s) == 3 and 7 >= s[0] >= s[1] >= s[2] >= 1 for s in c)
    for L in (1, 4, 7):
        assert candidate_schedules(L, 1) == [()]
    assert candidate_schedules(3, 2) == [(3,), (2,), (1,)]
    # a chain of more than eight accumulators: seven entries, the last one holds for every later product
    assert all(len(s) == 7 for s in candidate_schedules(2, 12)) and len(candidate_schedules(2, 12)) == 8


def test_schedule_cost_and_pick_on_small_tables():
    from nested_hashing_psi_amd.schedule import pick_schedule, schedule_cost
    assert schedule_cost(()) == 0 and schedule_cost((4,)) == 80 and schedule_cost((4, 3)) == 80 + 57 and schedule_cost([1] * 7) == 7 * 17
    table = [((4, 4), 57, True), ((4, 3), 40, True), ((3, 3), 12, True), ((2, 2), 30, False)]
    assert pick_schedule(table, 10) == (3, 3)
    assert pick_schedule(table, 12) == (3, 3) and pick_schedule(table, 13) == (4, 3)      # min_budget >= margin_bits
    assert pick_schedule(table, 41) == (4, 4) and pick_schedule(table, 58) is None
    assert pick_schedule([((2, 2), 58, False)], 0) is None and pick_schedule([], 0) is None
    # equal cost: the lexicographically larger schedule, whatever the order of the rows
    flat = lambda s: 1
    for rows in (table[:3], table[:3][::-1]):
        assert pick_schedule(rows, 10, cost=flat) == (4, 4)
    assert pick_schedule(table, 10, cost=lambda s: -schedule_cost(s)) == (4, 4)


def _restated_pick(table, margin):
    """the rule, restated: qualifying rows by (cost, then the larger tuple)"""
    ok = [s for s, bud, same in table if same and bud >= margin]
    if not ok:
        return None
    cost = lambda s: sum(l * l + 16 * l for l in s)
    low = min(cost(s) for s in ok)
    return max(s for s in ok if cost(s) == low)


def test_pick_schedule_on_the_oracles_table(ob):
    """N = 4096, L = 4, t = 65537, K = 3, E = 4, b = 1, all 10 pairs: the budgets tests/test_chain_schedule.py prints (57, 57, 48, 14,
    14; (2,2) wrong), and what the rule makes of them"""
    from nested_hashing_psi_amd.schedule import candidate_schedules, pick_schedule
    _, _, table = bc.chooser_case(ob)
    print("\n".join("schedule %s: %d bits, %s plaintext" % (s, bud, "same" if same else "WRONG") for s, bud, same in table))
    assert [s for s, _, _ in table] == candidate_schedules(4, 3)
    row = {s: (bud, same) for s, bud, same in table}
    assert row[(4, 4)] == (57, True) and row[(4, 3)] == (57, True) and row[(3, 3)] == (48, True)
    assert row[(3, 2)] == (14, True) and row[(4, 2)] == (14, True) and not row[(2, 2)][1]
    for margin, want in ((20, (3, 3)), (10, (3, 2)), (59, None)):
        got = pick_schedule(table, margin)
        assert got == _restated_pick(table, margin), margin
        assert got == want, margin
        if got is not None:
            assert row[got][1] and row[got][0] >= margin
