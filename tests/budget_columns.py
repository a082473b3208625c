"""Ciphertexts of a known noise budget, and the oracle's table of chain schedules (plain module, imported by
tests/test_noise_budget.py and tests/test_gpu_noise_budget.py; not a conftest).  Built on tests/coeff_columns.py.

The planted column.  Decryption rounds t x / Q; the budget is read from the largest distance of t x / Q from an integer over the
coefficients of the phase x (include/piehip.h, piehip_client_decrypt_budget; oracle/pie_oracle.c, po_decrypt):
budget = floor(-log2(2 distance)).  With Q the product of the chain and r = 3 Q >> (k + 3), the column x = +-r t^-1 mod Q has
t x = +-r (mod Q): a distance d = 1.5 * 2^-(k + 2) up to the floor, so 2 d = 1.5 * 2^-(k + 1) sits in the middle of the interval
[2^-(k + 1), 2^-k) that reads as k bits, and the per-limb truncation of the 60-bit fractions (L units of 2^-60) cannot move the
readout for k <= 50.  A polynomial
with that column in one coefficient and zeros elsewhere has budget k; the all-zero phase has distance 0 and budget 58.
"""
import functools

import numpy as np

from oracle import exact as ex
from tests import coeff_columns as ccol

QUIET = 58      # the readout of a distance of 0
K_MAX = 50      # planted budgets go up to here (at 56 and 57 the truncation moves the readout by one)


def planted_value(o, k, sign):
    """x in [0, Q) with t x = sign * (3 Q >> (k + 3)) (mod Q)"""
    qs, _ = ccol.moduli(o)
    Q = ex.prod(qs)
    r = (3 * Q) >> (k + 3)
    return sign * r * pow(o.t % Q, -1, Q) % Q


def planted_poly(o, k, sign, pos):
    """COEFFICIENT polynomial [L][N]: planted_value at coefficient pos, zeros elsewhere"""
    qs, _ = ccol.moduli(o)
    poly = ccol.columns_poly([], qs, o.N)
    poly[:, pos] = np.array(ccol.reduce_col(planted_value(o, k, sign), qs), dtype=np.uint64)
    return poly


def quiet_poly(o):
    qs, _ = ccol.moduli(o)
    return ccol.columns_poly([], qs, o.N)


def sampled_ct(o, X, sk, rng, ncomp):
    """the ciphertext [ncomp][L][N] of phase X under sk with c1 (and c2) uniform"""
    qs, _ = ccol.moduli(o)
    u = [ccol.uniform_poly(qs, o.N, rng) for _ in range(ncomp - 1)]
    return ccol.phase_ct(o, X, sk, *u)


def oracle_budgets(o, sk, cts):
    return np.array([o.decrypt(sk, ct)[1] for ct in cts], dtype=np.int32)


def budget_readout(max_dist):
    """the oracle's readout (po_decrypt), restated: 58 at 0, else 59 - bit length, clamped to [0, 58]"""
    if max_dist == 0:
        return 58
    return max(0, min(58, 59 - int(max_dist).bit_length()))


# ---- the chooser's case: N = 4096, L = 4, t = 65537, K = 3, E = 4, b = 1 (the third row of the header's schedule table) ----------------
CHOOSER = dict(N=4096, L=4, t=65537, K=3, E=4, b=1)


def oracle_schedule_table(ob, o, sk, evk, idx, minus, db, masks, candidates):
    """[(schedule, budget, same plaintext)] of bin layer 0 by the definition (tests/test_chain_schedule.py), every row decrypted
    by the level oracle of its last product; the reference plaintext is the full run's"""
    from tests.test_chain_schedule import last_level, level_oracles, schedule_layer_exact
    K = idx.shape[0]
    levels = level_oracles(ob, o, range(1, o.L + 1))
    m_full, _ = o.decrypt(sk, schedule_layer_exact(o, levels, idx, minus, db, masks, evk, [o.L], 0))
    table = []
    for sched in candidates:
        row = schedule_layer_exact(o, levels, idx, minus, db, masks, evk, list(sched), 0)
        l = last_level(sched, K)
        m, bud = levels[l].decrypt(np.ascontiguousarray(sk[:l]), row)
        table.append((tuple(sched), int(bud), bool((m == m_full).all())))
    return table


@functools.lru_cache(maxsize=1)
def chooser_case(ob):
    """(oracle, (sk, evk, idx, minus, db, masks), table over candidate_schedules(L, K)): the fresh query of
    tests/test_chain_schedule.py::NOISE's third row (rng seed N + E) and the oracle's table of all 10 pairs.  Computed once; the
    arrays are read-only"""
    from nested_hashing_psi_amd.schedule import candidate_schedules
    from tests.test_result_relin import fresh_query
    c = CHOOSER
    o = ob.Oracle(c["N"], c["L"], c["t"])
    inputs = fresh_query(ob, o, np.random.default_rng(c["N"] + c["E"]), c["K"], c["E"], c["b"], c["N"] // 2)
    table = oracle_schedule_table(ob, o, *inputs, candidate_schedules(c["L"], c["K"]))
    for v in inputs:
        v.setflags(write=False)
    return o, inputs, table
