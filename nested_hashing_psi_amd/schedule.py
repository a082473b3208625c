"""Choosing a chain schedule (include/piehip.h "Chain limbs", piehip_set_chain_schedule) from measured noise budgets.

The library checks no noise: a schedule with too few limbs does not fail, it decrypts to a wrong plaintext.  The client can measure
what a result row has left (client.BatchedFHEPSIClient.decrypt(.., budget=True), piehip_client_decrypt_budget), so the choice is:
run every candidate schedule on a query of the real parameters, keep those that give the full run's plaintext with a margin of
budget to spare, and take the cheapest.

Two parts.  The pure one -- candidate_schedules, schedule_cost, pick_schedule -- is the rule, and needs no device.  The device one
-- measure_schedules, choose_chain_schedule -- drives an operator and a client that the caller has set up.  A budget is a
measurement on one query, one database and one key, not a bound: the margin is what covers the others.
"""
import itertools

import numpy as np

MAX_ENTRIES = 7    # piehip_set_chain_schedule takes 1 to 7 entries


def candidate_schedules(L, K):
    """every non-increasing tuple of min(K - 1, 7) limb counts in 1..L -- one per product of a chain of K accumulators -- from
    (L, .., L) downwards.  K = 1 has no product: [()]"""
    L, K = int(L), int(K)
    if L < 1 or K < 1:
        raise ValueError("L and K must be at least 1")
    return list(itertools.combinations_with_replacement(range(L, 0, -1), min(K - 1, MAX_ENTRIES)))


def schedule_cost(sched):
    """sum of l^2 + 16 l over the entries: the part of DESIGN.md section 4's limb-transform count of one product that depends on
    its limb count (the L^2 digit transforms of the key switch, and the transforms of operands, tensor result and product that
    grow with L).  A PROXY for ordering schedules, not a timing: it knows nothing of routes, fusions or queues.  Measure the
    schedules it ranks close together."""
    return sum(int(l) * int(l) + 16 * int(l) for l in sched)


def pick_schedule(table, margin_bits, cost=schedule_cost):
    """table: rows (schedule, min_budget, same_plaintext).  Among the rows with the reference plaintext and min_budget >=
    margin_bits, the schedule of lowest cost; of two with the same cost, the lexicographically larger (more limbs early in the
    chain).  None when no row qualifies"""
    best = None
    for sched, min_budget, same in table:
        if not same or min_budget < margin_bits:
            continue
        key = (-cost(sched), tuple(sched))
        if best is None or key > best[0]:
            best = (key, tuple(sched))
    return None if best is None else best[1]


def _decrypt_rows(op, client, nslots):
    """run() as the operator stands -> (slots of every row of every query, the smallest budget among them)"""
    op.run()
    rows = op.getResultList()
    # rows [..][components][limbs][N]: min(resultLimbs, limbs of the last product) limbs, as the operator sized them
    rows = np.ascontiguousarray(rows.reshape((-1,) + rows.shape[-3:]))
    slots, budgets = client.decrypt(rows, nslots=nslots, limbs=rows.shape[-2], budget=True)
    return slots, int(budgets.min())


def measure_schedules(op, client, candidates=None, nslots=None):
    """op: a pie.BatchedFHEHIPPIE with its database, EvalMult key and a query of `client` (a client.BatchedFHEPSIClient with that
    query's secret key) in place.  Runs the default schedule [L], whose slots are the reference plaintext, then every candidate
    (default: candidate_schedules(L, K)), and returns the table [(schedule, min_budget, same_plaintext)]: the smallest budget
    among the result rows of all queries, and whether every slot of every row equals the reference.  The result-limbs and
    result-relin settings stay as they are and take part in what is measured.  The operator's schedule is put back on every way
    out."""
    L, K = op.cc.L, op.K
    if candidates is None:
        candidates = candidate_schedules(L, K)
    before = op.chainSchedule()
    table = []
    try:
        op.setChainSchedule([L])
        reference, _ = _decrypt_rows(op, client, nslots)
        reference = reference.copy()
        for sched in candidates:
            sched = tuple(int(v) for v in sched)
            if sched:
                op.setChainSchedule(sched)
            slots, min_budget = _decrypt_rows(op, client, nslots)
            table.append((sched, min_budget, bool(slots.shape == reference.shape and (slots == reference).all())))
    finally:
        op.setChainSchedule(before)
    return table


def choose_chain_schedule(op, client, margin_bits, candidates=None, cost=schedule_cost):
    """(pick_schedule(table, margin_bits, cost), table) of measure_schedules(op, client, candidates).  Nothing is left set on op:
    the caller sets what it takes -- op.setChainSchedule(choice) -- and None means that no candidate keeps margin_bits bits"""
    table = measure_schedules(op, client, candidates)
    return pick_schedule(table, margin_bits, cost), table
