"""Query slices without a GPU: the partition of the K L (inner hash function, limb) units over G ranks.

piehip_query_slice (host only, no device is opened) and shard.query_slice give rank r of G the units [K L r / G, K L (r + 1) / G) --
the rule of piehip_rccl_bin_slice.  Over all r they tile 0 .. K L exactly once, in order, also when G > K L (some slices are then
empty), and the two agree."""
import ctypes as C

import pytest

from nested_hashing_psi_amd import _lib, shard


def _c_slice(K, L, G, r):
    lo, hi = C.c_uint32(7), C.c_uint32(7)
    assert _lib.lib().piehip_query_slice(K, L, G, r, C.byref(lo), C.byref(hi)) == 0
    return lo.value, hi.value


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_slices_tile_the_units_once_in_order(K):
    for L in range(1, 8):
        for G in range(1, 17):
            at = 0
            sizes = []
            for r in range(G):
                lo, hi = _c_slice(K, L, G, r)
                assert (lo, hi) == shard.query_slice(K, L, G, r)
                assert lo == at and hi >= lo
                at = hi
                sizes.append(hi - lo)
            assert at == K * L
            assert max(sizes) - min(sizes) <= 1
            if G > K * L:
                assert sizes.count(0) == G - K * L


def test_a_unit_is_a_hash_function_and_a_limb():
    """u = h L + l: a slice of K L / G = L units is one inner hash function, every limb"""
    K, L = 3, 4
    for r in range(K):
        assert shard.query_slice(K, L, K, r) == (r * L, (r + 1) * L)


def test_bad_ranks_are_refused():
    lo, hi = C.c_uint32(), C.c_uint32()
    lib = _lib.lib()
    for G, r in [(0, 0), (4, 4), (4, -1)]:
        assert lib.piehip_query_slice(2, 2, G, r, C.byref(lo), C.byref(hi)) == -1
        assert lib.piehip_last_error()
    assert lib.piehip_query_slice(2, 2, 1, 0, None, C.byref(hi)) == -1
