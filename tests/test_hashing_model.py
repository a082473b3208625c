"""The offline-phase cases on the CPU: tests/hashing_model.py against the oracle, and every case against what it declares.

The GPU test (tests/test_gpu_offline_hashing.py) compares tables; whether a table's walk went anywhere is decided here, from
the model's statistics: a case whose evictions, retry depth, repeats or kernel are no longer what tests/hashing_cases.py
states fails in this file instead of passing vacuously on the device.
"""
import os

import numpy as np
import pytest

from tests import hashing_cases as hc
from tests import hashing_model as hm

_model = {}


def model(ob, case):
    """hashing_model.build of a case, once per session"""
    if case.name not in _model:
        ref = hc.reference(ob, case)
        _model[case.name] = hm.build(ref["tab"], ref["items"], case.k, case.e, case.K, case.b, case.E, hc.SEEDS["evict_seed"])
    return _model[case.name]


@pytest.mark.parametrize("case", hc.CASES, ids=repr)
def test_model_equals_oracle(ob, case):
    """cell for cell, or both fail"""
    ref, got = hc.reference(ob, case), model(ob, case)
    if isinstance(got, hm.Failed):
        assert ref["built"] is None, "the model fails (%r), the oracle builds" % got
        return
    assert ref["built"] is not None, "the model builds, the oracle fails"
    tbl, _ = got
    diff = np.argwhere(tbl != ref["built"])
    assert len(diff) == 0, "first of %d differing cells at [outer, inner, row, bin, column] = %s" % (len(diff), diff[0])


@pytest.mark.parametrize("case", hc.SUCCEEDING, ids=repr)
def test_invariants_hold(ob, case):
    """on the model's table, and on the oracle's after the bin shuffle"""
    ref = hc.reference(ob, case)
    shape = (case.k, case.e, case.K, case.b, case.E)
    assert hm.invariants(ref["tab"], ref["items"], model(ob, case)[0], *shape) == []
    assert hm.invariants(ref["tab"], ref["items"], ref["shuffled"], *shape) == []


@pytest.mark.parametrize("case", hc.CASES, ids=repr)
def test_case_reaches_its_conditions(ob, case):
    ref, got, cond = hc.reference(ob, case), model(ob, case), case.conditions
    items = ref["items"]
    assert case.k * case.e <= hc.N
    assert int(items.max()) < case.t
    kernel, wpb = hm.launch(case.K, case.b, case.E)
    reached = dict(kernel=kernel, wpb=wpb, idle_wave=wpb > 0 and case.e % wpb != 0, b_over_64=case.b > 64,
                   fails=isinstance(got, hm.Failed), contains=tuple(v for v in cond.get("contains", ()) if v in set(items.tolist())))
    stats = got.stats if isinstance(got, hm.Failed) else got[1]
    reached.update(min_evictions=sum(s.evictions for s in stats), min_run=max(s.max_run for s in stats),
                   min_dups=sum(s.dup_hits for s in stats), min_dups_later_batch=sum(s.dup_later_batch for s in stats),
                   min_zero_hits=sum(s.zero_hits for s in stats))
    if not reached["fails"]:
        per_table = [n for s in stats for n in s.per_table]
        reached.update(full=bool((got[0] != 0).all()), empty_inner=0 in per_table and 1 in per_table)
        # item 0 with every column of its own full would be inserted and leave a hole; behind a hole the reference's lookUp, which
        # stops at the first empty cell, and a look at the whole column differ, and a repeat may be stored twice
        assert sum(s.zero_walks for s in stats) == 0
    print("%s: %d items, %s" % (case.name, len(items), ", ".join("%s=%s" % (c, reached[c]) for c in sorted(reached))))
    for c, want in cond.items():
        if c.startswith("min_"):
            assert reached[c] >= want, "%s: %s is %d, declared at least %d" % (case.name, c, reached[c], want)
        else:
            assert reached[c] == want, "%s: %s is %r, declared %r" % (case.name, c, reached[c], want)
    if "fails" not in cond:
        assert not reached["fails"], "%s is not declared to fail, the model fails at %r" % (case.name, got)


def test_invariants_reject_damaged_tables(ob):
    """an item moved to a wrong column, an item dropped, an item doubled"""
    case = hc.BY_NAME["edge-values"]
    ref = hc.reference(ob, case)
    shape = (case.k, case.e, case.K, case.b, case.E)
    good = ref["shuffled"]
    # an item with an empty cell beside it in its bin layer and one above it in its column
    at = next(tuple(int(v) for v in a) for a in np.argwhere(good != 0)
              if (good[tuple(a[:4])] == 0).any() and (good[tuple(a[:3])][:, a[4]] == 0).any())
    x = int(good[at])

    moved = good.copy()
    free = next(c for c in range(case.E) if moved[at[:4] + (c,)] == 0)
    moved[at[:4] + (free,)], moved[at] = x, 0
    bad = hm.invariants(ref["tab"], ref["items"], moved, *shape)
    assert len(bad) == 1 and "whose column" in bad[0]

    # the same item under the other outer function's inner table is a wrong place too
    other = good.copy()
    other[at] = 0
    p = next(p for p in range(case.e) if p != at[1])
    hole = tuple(np.argwhere(other[at[0], p] == 0)[0])
    other[(at[0], p) + hole] = x
    bad = hm.invariants(ref["tab"], ref["items"], other, *shape)
    assert len(bad) == 1 and "whose inner table" in bad[0]

    dropped = good.copy()
    dropped[at] = 0
    bad = hm.invariants(ref["tab"], ref["items"], dropped, *shape)
    assert bad == ["outer %d: item %d is missing" % (at[0], x)]

    doubled = good.copy()
    free = next(bn for bn in range(case.b) if doubled[at[:3] + (bn, at[4])] == 0)  # same column, another bin: a legal place
    doubled[at[:3] + (free, at[4])] = x
    bad = hm.invariants(ref["tab"], ref["items"], doubled, *shape)
    assert len(bad) == 1 and "a second time" in bad[0]

    stranger = good.copy()
    stranger[tuple(np.argwhere(good == 0)[0])] = case.t - 2 if case.t - 2 not in set(ref["items"].tolist()) else case.t - 3
    bad = hm.invariants(ref["tab"], ref["items"], stranger, *shape)
    assert len(bad) == 1 and "no server item" in bad[0]


def test_generator_below_is_mask_and_rejection():
    """below(bound) keeps the low bits that cover bound - 1 and redraws until the value is below bound; one stream, so the
    accepted values are the first stream words that pass"""
    for bound in (1, 2, 3, 64, 70, 100, 1 << 32):
        a, b = hm.Rng(12345), hm.Rng(12345)
        mask = 1
        while mask < bound:
            mask <<= 1
        mask -= 1
        for _ in range(50):
            v = a.below(bound)
            while True:
                w = b.next() & mask
                if w < bound:
                    break
            assert v == w < bound
    # splitmix64 / xoshiro256** reference values: seed 0 gives the well-known first splitmix64 outputs as state
    assert hm.Rng(0).s == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]


def test_launch_rule_is_the_one_in_the_source():
    """launch() restates two lines of launch_hash_build; when they change, it has to follow"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "nested_hashing_psi_amd", "csrc", "kernels_hash.hip")) as f:
        src = f.read()
    assert "table_bytes = ((size_t)K * b * E + (K * 64 + 1) / 2) * sizeof(u64);" in src
    assert "if (table_bytes <= 64 * 1024) {" in src
    assert "std::max<size_t>(1, std::min<size_t>(4, (64 * 1024) / table_bytes))" in src
    assert hm.launch(2, 7, 7) == ("wave", 4)        # the headline shape's kind: a few KiB
    assert hm.launch(2, 128, 31) == ("wave", 1)     # (7936 + 64) * 8 = 64000 bytes
    assert hm.launch(2, 128, 32) == ("global", 0)   # (8192 + 64) * 8 = 66048 bytes
    assert hm.launch(2, 64, 31) == ("wave", 2)      # 32256 bytes
    assert hm.launch(3, 20, 40) == ("wave", 3)      # 19968 bytes
