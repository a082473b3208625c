"""The device's offline phase (piehip_build_db_bins: kernels_hash.hip) against the oracle where the insertion walk goes deep:
loaded and full tables, walks of many passes, both insertion kernels, 1 to 4 waves per workgroup, repeats and item 0, the
failure path.  What each case is there for is stated in tests/hashing_cases.py and held on the CPU by
tests/test_hashing_model.py; here the device's table is compared with the oracle's, cell for cell.
"""
import numpy as np
import pytest

from tests import hashing_cases as hc
from tests import hashing_model as hm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pie():
    from nested_hashing_psi_amd import pie as p
    return p


def build_on_device(pie, cc, case, ref, **kw):
    return pie.BatchedFHEHIPPIE(cc, serverSet=ref["items"], hashParams=case.hash_params(), **kw)


def assert_same_table(case, ref, got):
    want = ref["shuffled"]
    assert got.shape == want.shape
    diff = np.argwhere(got != want)
    if len(diff) == 0:
        return
    i, p = int(diff[0][0]), int(diff[0][1])
    count = sum(1 for x in ref["items"].tolist() if ref["tab"].hash(x, i) % case.e == p)
    tables = sorted(set((int(d[0]), int(d[1])) for d in diff))
    kernel, wpb = hm.launch(case.K, case.b, case.E)
    raise AssertionError(
        "%s: the device's table differs from the oracle's first in (outer function %d, inner table %d), which takes %d items; "
        "%d cells in %d of %d inner tables differ; kernel: %s%s; first cell [row, bin, column] = %s holds %d, the oracle %d"
        % (case.name, i, p, count, len(diff), len(tables), case.k * case.e, kernel,
           " at %d waves per workgroup" % wpb if wpb else "", diff[0][2:].tolist(), int(got[tuple(diff[0])]), int(want[tuple(diff[0])])))


def query(ob, case, o):
    """random index and minus ciphertexts, as test_offline_phase_on_device draws them"""
    B = case.k * case.e
    sk = o.keygen(1)
    rng = np.random.default_rng(5)
    idx = np.stack([o.encrypt_slots(sk, rng.integers(0, 2, B), 10 + i) for i in range(case.K * case.E)])
    idx = idx.reshape(case.K, case.E, 2, hc.L, hc.N)
    minus = o.encrypt_slots(sk, -rng.integers(1, 1000, B), 9)
    return sk, idx, minus


def run_once(op, idx, minus):
    op.setMinusCompareElement(minus)
    op.setIndex(idx)
    op.run()
    return op.getResultList().copy()


@pytest.mark.parametrize("case", hc.SUCCEEDING, ids=repr)
def test_table_matches_oracle(ob, pie, case):
    """hashTable() == ph_hct_build + ph_hct_shuffle_bins, and the invariants hold on the device's own table; for the small
    cases the gathered, encoded database answers a run() as one built from the oracle's slots and masks does"""
    ref = hc.reference(ob, case)
    cc = pie.PieContext(hc.N, hc.L, case.t)
    op = build_on_device(pie, cc, case, ref)
    got = op.hashTable()
    assert_same_table(case, ref, got)
    assert hm.invariants(ref["tab"], ref["items"], got, case.k, case.e, case.K, case.b, case.E) == []
    if case.online:
        o = ob.Oracle(hc.N, hc.L, case.t)
        sk, idx, minus = query(ob, case, o)
        cc.load_relin_key(o.relin_keygen(sk, 2))
        res = run_once(op, idx, minus)
        if case.name == "wave-b70":
            # a shard that keeps the upper half of the bin layers holds those layers of the whole database
            lo, hi = case.b // 2, case.b
            part = run_once(build_on_device(pie, cc, case, ref, binSlice=(lo, hi)), idx, minus)
            assert part.shape[0] == hi - lo and (part == res[lo:hi]).all()
        slots = ob.pack_db(ref["shuffled"])
        mask_slots = ob.masks(case.t, case.b, case.k * case.e, hc.SEEDS["mask_seed"])
        want = run_once(pie.BatchedFHEHIPPIE(cc, slots=slots, mask_slots=mask_slots), idx, minus)
        assert (res == want).all()
    cc.close()


@pytest.mark.parametrize("case", hc.FAILING, ids=repr)
def test_failed_build_is_reported_and_leaves_the_handle_clean(ob, pie, case):
    """a set that the oracle cannot place is refused with the reference's error; the same context then builds a full table
    correctly and refuses the set again: fail flag and scratch arena are left clean, and a failure in one inner table of
    several is not lost while the other waves finish"""
    ref = hc.reference(ob, case)
    assert ref["built"] is None
    good = hc.BY_NAME["wave-full"]
    good_ref = hc.reference(ob, good)
    cc = pie.PieContext(hc.N, hc.L, case.t)
    with pytest.raises(RuntimeError, match="Cuckoo"):
        build_on_device(pie, cc, case, ref)
    assert good.t <= case.t  # the good case's items fit the failing case's plaintext modulus; the table does not depend on it
    op = build_on_device(pie, cc, good, good_ref)
    got = op.hashTable()
    assert_same_table(good, good_ref, got)
    assert hm.invariants(good_ref["tab"], good_ref["items"], got, good.k, good.e, good.K, good.b, good.E) == []
    with pytest.raises(RuntimeError, match="Cuckoo"):
        build_on_device(pie, cc, case, ref)
    cc.close()


def test_build_is_repeatable(ob, pie):
    """two builds of one set on one context give one table: nothing of the LDS carving or of the first table leaks"""
    case = hc.BY_NAME["wave-1"]
    ref = hc.reference(ob, case)
    cc = pie.PieContext(hc.N, hc.L, case.t)
    first = build_on_device(pie, cc, case, ref).hashTable()
    second = build_on_device(pie, cc, case, ref).hashTable()
    assert (first == second).all()
    assert_same_table(case, ref, second)
    cc.close()
