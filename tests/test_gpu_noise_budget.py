"""Noise budgets from the device client (piehip_client_decrypt_budget, dec_round_budget_kernel) and the schedule chooser
(nested_hashing_psi_amd/schedule.py) on the GPU.

The budget is an integer readout of a 60-bit fixed-point number that the device and the oracle form with the same arithmetic, so
every comparison is for equality: planted ciphertexts of a known budget (tests/budget_columns.py; tests/test_noise_budget.py pins
them on the oracle) on rings below, at and above one 256-thread block, slots against the plain decryption entry points, no
carry-over between calls, honest ciphertexts and products, reduced rows, and the chooser against the oracle's table of schedules.
"""
import ctypes as C

import numpy as np
import pytest

from tests import budget_columns as bc
from tests import coeff_columns as ccol
from tests.param_chains import T16, T32
from tests.test_gpu_client_columns import ROUTE_CASES, _context, dev_decrypt
from tests.test_result_limbs import reduced_oracle

pytestmark = pytest.mark.gpu

KS = (0, 1, 17, 50)
SENTINEL = -7


def dev_budget_rc(h, sk, cts, ncomp, B, nct=None, slots=True, dist=True, null=()):
    """piehip_client_decrypt_budget, called directly: (return code, slots [nct][B], budget [nct], max_dist [nct]), every array with
    at least one entry; slots and budget start at SENTINEL, max_dist at 2^63; `null` names arguments passed as null pointers"""
    from nested_hashing_psi_amd._lib import i32p, i64p, lib, u64p
    a = np.ascontiguousarray(cts, dtype=np.uint64)
    n = a.shape[0] if nct is None else nct
    out = np.full((max(n, 1), max(B, 1)), SENTINEL, dtype=np.int64)
    bud = np.full(max(n, 1), SENTINEL, dtype=np.int32)
    md = np.full(max(n, 1), 1 << 63, dtype=np.uint64)
    rc = lib().piehip_client_decrypt_budget(None if "h" in null else h, None if "sk" in null else sk.ctypes.data_as(u64p),
                                            None if "ct" in null else a.ctypes.data_as(u64p), n, ncomp, B,
                                            out.ctypes.data_as(i64p) if slots else None,
                                            None if "budget" in null else bud.ctypes.data_as(i32p), md.ctypes.data_as(u64p) if dist else None)
    return rc, out, bud, md


def dev_budget(cc, sk, cts, B=0):
    """(slots, budget, max_dist) of cts [nct][2 or 3][L][N] in ONE call; B = 0 passes null slots"""
    a = np.ascontiguousarray(cts, dtype=np.uint64)
    assert a.ndim == 4 and a.shape[1] in (2, 3) and a.shape[2:] == (cc.L, cc.N)
    rc, slots, bud, md = dev_budget_rc(cc._h, sk, a, a.shape[1], B, slots=B > 0)
    assert rc == 0
    return slots, bud, md


def readout(md):
    from nested_hashing_psi_amd._lib import lib
    return np.array([lib().piehip_budget_from_distance(int(v)) for v in md], dtype=np.int32)


# ---- 1. planted budgets ----------------------------------------------------------------------------------------------------------------
# rings below one 256-thread block (64, 128: threads behind the ring still reach the barrier), exactly one (256) and more (512,
# 1024: one atomicMax per block into the same word); the loud coefficient in the first and last lane of a wave, of a block, of the ring
@pytest.mark.parametrize("L,t", [(1, T16), (3, T32)], ids=["L1", "L3"])
@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024])
def test_planted_budgets(ob, pie_mod, N, L, t):
    o = ob.Oracle(N, L, t)
    cc = _context(pie_mod, o)
    rng = np.random.default_rng(N + L)
    sk = o.keygen(71 + L)
    positions = [p for p in (0, 63, 64, 255, 256, N - 1) if p < N]
    positions = sorted(set(positions))
    try:
        for ncomp in (2, 3):
            cts, want = [], []
            for pos in positions:
                for k in KS:
                    for sign in (1, -1):
                        cts.append(bc.sampled_ct(o, bc.planted_poly(o, k, sign, pos), sk, rng, ncomp))     # loud
                        cts.append(bc.sampled_ct(o, bc.quiet_poly(o), sk, rng, ncomp))                     # quiet
                        want += [k, bc.QUIET]
            cts, want = np.stack(cts), np.array(want, dtype=np.int32)
            _, bud, md = dev_budget(cc, sk, cts)
            assert (bc.oracle_budgets(o, sk, cts) == want).all()
            bad = np.argwhere(bud != want)
            assert not len(bad), "%d components: %d of %d budgets differ, first ciphertext %d: %d for %d" % (
                ncomp, len(bad), len(want), bad[0][0], bud[bad[0][0]], want[bad[0][0]])
            assert (md[1::2] == 0).all() and (md[0::2] > 0).all()
            assert (readout(md) == bud).all()
    finally:
        cc.close()


# ---- 2. slots, the B = 0 form, refusals ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ob, pie_mod):
    """N = 512 (two blocks), L = 3: a batch of planted, quiet and uniform phases in both component counts"""
    o = ob.Oracle(512, 3, T32)
    cc = _context(pie_mod, o)
    rng = np.random.default_rng(512)
    sk = o.keygen(73)
    qs, _ = ccol.moduli(o)
    polys = [bc.planted_poly(o, 17, 1, 300), bc.quiet_poly(o), ccol.uniform_poly(qs, o.N, rng), bc.planted_poly(o, 40, -1, 5),
             ccol.tile(ccol.decrypt_families(o), o.N, rng)]
    batches = {n: np.stack([bc.sampled_ct(o, X, sk, rng, n) for X in polys]) for n in (2, 3)}
    yield o, cc, sk, batches
    cc.close()


def test_slots_are_those_of_the_plain_decryption(mixed):
    o, cc, sk, batches = mixed
    for ncomp, cts in batches.items():
        want_bud = bc.oracle_budgets(o, sk, cts)
        assert want_bud[0] == 17 and want_bud[1] == bc.QUIET and want_bud[2] <= 1 and want_bud[3] == 40
        for B in (1, 7, o.N // 2, o.N):
            slots, bud, md = dev_budget(cc, sk, cts, B)
            assert slots.shape == (len(cts), B) and (slots == dev_decrypt(cc, sk, cts, B)).all(), "%d components, B = %d" % (ncomp, B)
            assert (bud == want_bud).all() and (readout(md) == bud).all()
        _, bud, md = dev_budget(cc, sk, cts, 0)
        assert (bud == want_bud).all() and (readout(md) == bud).all()
        # max_dist is optional
        rc, _, bud, md = dev_budget_rc(cc._h, sk, cts, ncomp, 0, slots=False, dist=False)
        assert rc == 0 and (bud == want_bud).all() and (md == 1 << 63).all()


def test_refusals_write_nothing(mixed, pie_mod):
    o, cc, sk, batches = mixed
    cts = batches[2]
    cases = [dict(null=("h",)), dict(null=("sk",)), dict(null=("ct",)), dict(nct=0), dict(ncomp=0), dict(ncomp=1), dict(ncomp=4),
             dict(B=o.N + 1), dict(B=7, slots=False)]
    for kw in cases:
        args = dict(ncomp=2, B=7)
        args.update(kw)
        rc, slots, bud, md = dev_budget_rc(cc._h, sk, cts, args.pop("ncomp"), args.pop("B"), **args)
        assert rc == pie_mod.EINVAL, kw
        assert (bud == SENTINEL).all() and (md == 1 << 63).all() and (slots == SENTINEL).all(), kw
    rc, slots, _, md = dev_budget_rc(cc._h, sk, cts, 2, 7, null=("budget",))
    assert rc == pie_mod.EINVAL and (md == 1 << 63).all() and (slots == SENTINEL).all()
    # and the handle measures afterwards
    assert (dev_budget(cc, sk, cts)[1] == bc.oracle_budgets(o, sk, cts)).all()


# ---- 3. no carry-over between calls on one handle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nct", [1, 2, 17, 33])
def test_a_quiet_batch_after_a_loud_one(mixed, nct):
    """max_dist is scratch that the next call gets again: a loud batch (k = 0: the largest distances there are), then a quiet one of
    the same size, which must read 58 with max_dist = 0"""
    o, cc, sk, _ = mixed
    rng = np.random.default_rng(nct)
    loud = np.stack([bc.sampled_ct(o, bc.planted_poly(o, 0, 1 if c % 2 else -1, (37 * c) % o.N), sk, rng, 2) for c in range(nct)])
    quiet = np.stack([bc.sampled_ct(o, bc.quiet_poly(o), sk, rng, 2) for _ in range(nct)])
    _, bud, md = dev_budget(cc, sk, loud)
    assert (bud == 0).all() and (md >= 1 << 58).all()
    _, bud, md = dev_budget(cc, sk, quiet)
    assert (bud == bc.QUIET).all() and (md == 0).all()


# ---- 4. honest ciphertexts ---------------------------------------------------------------------------------------------------------------
REAL = [c for c in ROUTE_CASES if c[:2] in ((256, 1), (1024, 3), (4096, 2))]


@pytest.mark.parametrize("n,L,chain,t", REAL, ids=["%d-%d" % c[:2] for c in REAL])
def test_fresh_encryptions_and_products(ob, pie_mod, n, L, chain, t):
    """fresh encryptions, their relinearised product and their tensor product (piehip_eval_mult): the oracle's budget, whatever it
    is -- a product on one limb has none left"""
    assert len(REAL) == 3 and chain is None
    o = ob.Oracle(n, L, t)
    rng = np.random.default_rng(n + L)
    sk = o.keygen(75)
    evk = o.relin_keygen(sk, 76)
    slots = rng.integers(-(t // 2), t // 2, (2, n // 2), dtype=np.int64)
    enc = np.stack([o.encrypt_slots(sk, slots[c], 900 + c) for c in range(2)])
    cc = _context(pie_mod, o)
    try:
        cc.load_relin_key(evk)
        prod2 = cc.EvalMult(enc[0], enc[1], relin=True)
        prod3 = cc.EvalMult(enc[0], enc[1], relin=False)
        assert (prod2 == o.mul(enc[0], enc[1], evk)).all()
        two = np.stack([enc[0], enc[1], prod2])
        got2, got3 = dev_budget(cc, sk, two, n), dev_budget(cc, sk, prod3[None], n)
    finally:
        cc.close()
    want2, want3 = bc.oracle_budgets(o, sk, two), bc.oracle_budgets(o, sk, prod3[None])
    print("N=%d L=%d t=2^%d: fresh %d, %d bits; product %d bits, not relinearised %d bits" % (n, L, t.bit_length() - 1, *want2, *want3))
    assert (got2[1] == want2).all() and (got3[1] == want3).all()
    assert want2[0] >= 1 and want2[1] >= 1
    assert (readout(got2[2]) == got2[1]).all() and (readout(got3[2]) == got3[1]).all()
    assert (got2[0] == np.stack([o.decode(o.decrypt(sk, ct)[0], n) for ct in two])).all()


@pytest.mark.parametrize("keep", [1, 2])
def test_client_budgets_of_reduced_rows(ob, pie_mod, keep):
    """client.decrypt(.., limbs=keep, budget=True) and noiseBudget on rows reduced with piehip_mod_reduce, against the level oracle;
    budget=False is the call it always was"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    n, L, t = 1024, 3, T32
    o = ob.Oracle(n, L, t)
    ro = reduced_oracle(ob, o, keep)
    rng = np.random.default_rng(keep)
    sk = o.keygen(77)
    slots = rng.integers(-(t // 2), t // 2, (3, n // 2), dtype=np.int64)
    enc = np.stack([o.encrypt_slots(sk, slots[c], 910 + c) for c in range(3)])
    cc = _context(pie_mod, o)
    try:
        cl = BatchedFHEPSIClient(cc, 1, n // 2, 1, 1, 1)
        cl.sk = sk
        rows = cc.mod_reduce(enc, keep)
        got, bud = cl.decrypt(rows, limbs=keep, budget=True)
        plain = cl.decrypt(rows, limbs=keep)
        low = cl.noiseBudget(rows, limbs=keep)
        full, bud_full = cl.decrypt(enc, budget=True)
    finally:
        cc.close()
    skk = np.ascontiguousarray(sk[:keep])
    want = bc.oracle_budgets(ro, skk, rows)
    print("N=%d t=2^%d: %d of %d limbs kept: %s bits (all limbs: %s)" % (n, t.bit_length() - 1, keep, L, list(want), list(bud_full)))
    assert bud.dtype == np.int32 and bud.shape == (3,) and (bud == want).all() and low == int(want.min())
    assert isinstance(plain, np.ndarray) and (got == plain).all() and (got == slots).all() and (full == slots).all()
    assert (bud_full == bc.oracle_budgets(o, sk, enc)).all() and want.min() >= 1


# ---- 5. the chooser end to end -------------------------------------------------------------------------------------------------------
def test_chooser_against_the_oracles_table(ob, pie_mod):
    """the N = 4096 case of tests/test_noise_budget.py on the device: the table of measure_schedules is the oracle's row for row, the
    choices are the CPU test's, and the operator is left as it was found"""
    from nested_hashing_psi_amd import schedule
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    pie = pie_mod
    c = bc.CHOOSER
    o, (sk, evk, idx, minus, db, masks), want = bc.chooser_case(ob)
    cc = pie.PieContext(c["N"], c["L"], c["t"])
    try:
        assert (cc.moduli == o.moduli).all()
        op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=db, preCalcRandomMask=masks)
        cc.load_relin_key(evk)
        op.setMinusCompareElement(minus)
        op.setIndex(idx)
        cl = BatchedFHEPSIClient(cc, 1, c["N"], c["K"], c["E"], c["b"])      # every slot: the oracle compares every coefficient
        cl.sk = np.array(sk)
        op.setChainSchedule((4, 3))
        op.run()
        before = op.getResultList().copy()
        state = (op.chainSchedule(), op.resultLimbs, op.resultRelin)
        assert state == ([4, 3], c["L"], True)

        table = schedule.measure_schedules(op, cl)
        assert table == want
        assert (op.chainSchedule(), op.resultLimbs, op.resultRelin) == state
        for margin, choice in ((20, (3, 3)), (10, (3, 2)), (59, None)):
            got, tab = schedule.choose_chain_schedule(op, cl, margin)
            assert got == choice and tab == want, margin
            assert (op.chainSchedule(), op.resultLimbs, op.resultRelin) == state
        op.run()
        assert (op.getResultList() == before).all()

        # an illegal candidate raises where it is set, and the schedule is put back all the same
        with pytest.raises(ValueError):
            schedule.measure_schedules(op, cl, candidates=[(4, 4), (3, 4), (2, 2)])
        assert (op.chainSchedule(), op.resultLimbs, op.resultRelin) == state
        op.run()
        assert (op.getResultList() == before).all()
        # a caller's own candidates and cost
        got, tab = schedule.choose_chain_schedule(op, cl, 10, candidates=[(4, 2), (4, 4)], cost=lambda s: -sum(s))
        assert got == (4, 4) and tab == [r for r in want if r[0] in ((4, 2), (4, 4))][::-1]
    finally:
        cc.close()
