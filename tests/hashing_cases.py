"""The offline-phase cases of tests/test_hashing_model.py (CPU) and tests/test_gpu_offline_hashing.py (GPU), each with the
branch of kernels_hash.hip it is there for, stated as conditions.  TEST INFRASTRUCTURE, not a test.

A case is a shape (t, nS, k, e, K, E, b), a rule for its items and its conditions.  The CPU test reads the conditions off
tests/hashing_model.py (launch() and the statistics of build()) and fails where a case no longer reaches one, so that the GPU
test, which compares tables only, cannot pass on walks that stopped going deep.  Where a condition is missed after a change
to the items, move nS or the seed, never the condition.

Contexts are N = 1024, L = 2, so k * e <= 1024.  These are the smallest shapes that still reach what they name.
"""
import numpy as np

T16 = 65537
T32 = 4296540161
N, L = 1024, 2
SEEDS = dict(hash_seed=987654321, evict_seed=11, shuffle_seed=22, mask_seed=33)

# What a case can declare; a condition that is absent is not required.  Counts are summed over the outer functions,
# min_run is the highest index of the 1000-retry loop that any insertion reached.
CONDITIONS = {
    "kernel",            # "wave" (cuckoo_build_wave_kernel) or "global" (cuckoo_build_kernel)
    "wpb",               # waves per workgroup of the wave kernel
    "idle_wave",         # e is no multiple of wpb: the last workgroup has a wave without a table
    "b_over_64",         # more bin layers than lanes: the wave kernel's column scan takes two steps
    "min_evictions",
    "min_run",
    "min_dups",          # lookUp found a nonzero item that was already in the table
    "min_dups_later_batch",  # ... in a later batch of 64 items of its inner table than its first copy
    "min_zero_hits",     # item 0 taken for present
    "full",              # every cell of the table nonzero
    "empty_inner",       # an inner table without an item, and one with exactly one
    "contains",          # item values that must be in the set
    "fails",             # the build must fail
}


class Case:
    def __init__(self, name, t, nS, k, e, K, E, b, seed=0, base=None, edge=False, repeat=0, zeros=0, online=False, **conditions):
        self.name, self.t, self.nS, self.k, self.e, self.K, self.E, self.b = name, t, nS, k, e, K, E, b
        self.seed = seed        # moves the item set
        self.base = base        # take the items of this case instead of drawing nS
        self.edge = edge        # put 1, t//2, t//2 + 1 and t - 1 among the items
        self.repeat = repeat    # this many of the items a second time,
        self.zeros = zeros      # item 0 this many times, all shuffled
        self.online = online    # small K b E: the GPU test also compares a run() over the gathered, encoded database
        assert set(conditions) <= CONDITIONS, set(conditions) - CONDITIONS
        self.conditions = conditions

    @property
    def fails(self):
        return bool(self.conditions.get("fails"))

    def hash_params(self):
        return dict(k=self.k, e=self.e, K=self.K, b=self.b, E=self.E, **SEEDS)

    def __repr__(self):
        return self.name


def distinct(rng, t, n):
    """n distinct nonzero values below t, in random order"""
    out = np.unique(rng.integers(1, t, 2 * n + 16, dtype=np.uint64))
    rng.shuffle(out)
    assert len(out) >= n
    return out[:n].copy()


def items_of(case):
    """the case's server set in insertion order (uint64)"""
    if case.base is not None:
        items = items_of(BY_NAME[case.base])
        rng = np.random.default_rng(case.seed + 1000)
    else:
        rng = np.random.default_rng(case.seed + case.nS)
        items = distinct(rng, case.t, case.nS)
    if case.edge:
        edge = np.array([1, case.t // 2, case.t // 2 + 1, case.t - 1], dtype=np.uint64)
        items = np.concatenate([edge, items[~np.isin(items, edge)][:case.nS - len(edge)]])
        rng.shuffle(items)
    if case.repeat or case.zeros:
        again = rng.choice(items, case.repeat, replace=False)
        items = np.concatenate([items, again, np.zeros(case.zeros, dtype=np.uint64)])
        rng.shuffle(items)
    return np.ascontiguousarray(items, dtype=np.uint64)


CASES = [
    # cuckoo_build_kernel, one thread per table with the table in global memory: 66 and 70 KiB per inner table
    Case("global-loaded", T32, 16300, 1, 2, 2, 60, 70, kernel="global", b_over_64=True, min_evictions=1000, min_run=1),
    Case("global-K3", T32, 26000, 2, 3, 3, 100, 30, kernel="global", min_evictions=1000, min_run=1),
    Case("global-full", T32, 8400, 1, 1, 2, 60, 70, kernel="global", full=True, min_run=10),
    # cuckoo_build_wave_kernel at 1, 2 and 3 waves per workgroup (tables of 16 to 64 KiB): the LDS carving, the p >= e exit
    Case("wave-1", T32, 14800, 1, 3, 2, 40, 64, kernel="wave", wpb=1, min_evictions=1000, min_run=1),
    Case("wave-1-b100", T32, 23200, 1, 3, 2, 40, 100, kernel="wave", wpb=1, b_over_64=True, min_evictions=1000, min_run=1),
    Case("wave-2-e5", T32, 16000, 1, 5, 2, 50, 33, kernel="wave", wpb=2, idle_wave=True, min_evictions=1000, min_run=1),
    Case("wave-3-e7", T32, 15000, 1, 7, 3, 40, 20, kernel="wave", wpb=3, idle_wave=True, min_evictions=1000, min_run=1),
    # small tables (4 waves per workgroup) walked until they are full or nearly so
    Case("wave-full", T16, 112, 1, 1, 2, 7, 8, online=True, kernel="wave", wpb=4, full=True, min_run=10),
    Case("wave-b70", T16, 1080, 2, 2, 2, 4, 70, online=True, kernel="wave", wpb=4, b_over_64=True, min_evictions=1000, min_run=10),
    # lookUp before insert: repeats (the ballot over the column / the scan to the first empty cell) and the empty-cell sentinel
    Case("wave-dups", T16, 200, 2, 1, 2, 16, 8, repeat=50, zeros=3, online=True, kernel="wave", wpb=4, min_dups=100,
         min_dups_later_batch=20, min_zero_hits=1, min_evictions=1),
    Case("global-dups", T32, 16300, 1, 2, 2, 60, 70, base="global-loaded", repeat=500, zeros=1, kernel="global", min_dups=500,
         min_zero_hits=1, min_evictions=1000),
    Case("empty-inner", T16, 20, 2, 64, 2, 2, 3, online=True, kernel="wave", wpb=4, empty_inner=True),
    # gather_slots_kernel centres v > t/2 to v - t
    Case("edge-values", T16, 60, 2, 3, 2, 8, 4, edge=True, online=True, kernel="wave", wpb=4,
         contains=(1, T16 // 2, T16 // 2 + 1, T16 - 1)),
    # one item more than the table has cells, and a table of several that overflows
    Case("fails-wave", T16, 113, 1, 1, 2, 7, 8, kernel="wave", wpb=4, fails=True),
    Case("fails-global", T32, 8401, 1, 1, 2, 60, 70, kernel="global", fails=True),
    Case("fails-wave-3-e7", T32, 16100, 1, 7, 3, 40, 20, kernel="wave", wpb=3, idle_wave=True, fails=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) == 16

SUCCEEDING = [c for c in CASES if not c.fails]
FAILING = [c for c in CASES if c.fails]


_reference = {}


def reference(ob, case):
    """the oracle's answer for a case, computed once per session and read-only: dict(items, tab, built, shuffled); built and
    shuffled are None where the oracle's build fails"""
    if case.name not in _reference:
        items = items_of(case)
        tab = ob.Tabulation(SEEDS["hash_seed"], case.k + case.K)
        try:
            built = ob.hct_build(tab, items, case.k, case.e, case.K, case.b, case.E, evict_seed=SEEDS["evict_seed"])
        except RuntimeError:
            built = shuffled = None
        else:
            shuffled = built.copy()
            ob.hct_shuffle_bins(shuffled, SEEDS["shuffle_seed"])
            built.setflags(write=False)
            shuffled.setflags(write=False)
        items.setflags(write=False)
        _reference[case.name] = dict(items=items, tab=tab, built=built, shuffled=shuffled)
    return _reference[case.name]
