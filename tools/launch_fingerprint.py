"""What run() launches, per kernel class, on every route of the product chain:
    python tools/launch_fingerprint.py [--lib PATH] [--out FILE]

For each shape below and each setting of it (chain limbs, result relinearisation, result limbs) one profiled run() on one queue
(set_profiling(1), set_run_streams(1)) and PieContext.profile() with its `ms` field dropped: launches and algorithmic bytes per kernel
class.  One JSON object per (shape, setting), one per line.  Two builds of the library that enqueue the same schedule write the same
file byte for byte; --lib PATH takes another build than this tree's (a parent commit's, to compare a host-side change against).
The shapes are the smallest at which each route of the chain is taken (RUNS in tests/test_gpu_chain_limbs.py): the chain at L, a level
context with the fused conversion, with the drop kernel, a level that folds under a parent that does not, K = 1; a chain schedule
whose second product takes X from a level between the handle's and its own; a folded ring with moduli below 2^59 (folded kernels off
the column-accumulator path).  Behind them piehip_base_convert, kinds 0, 1 and 2, on a 60-bit chain and on a mixed one: no run(), one
line each with what profile() counted (nothing, where the call is not profiled; a kernel trace of this program shows the launches).
Inputs are uniform residues; the results are not looked at (the tests compare them with the exact definition).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T16, T32 = 65537, 4296540161
# (N, L, chain, t, K, b, nq, key per query, [(Lc or a chain schedule, result relinearisation, result limbs or None = L)])
# chain: None = the default 60-bit chain, a name of tests/param_chains.named_chain, or "below_2^k" = uniform_chain(.., below=1 << k)
SHAPES = [
    (2048, 4, None, T16, 2, 3, 1, False, [(4, 1, None), (3, 1, None), (2, 1, None)]),   # radix-2 ring: drop kernel, plain conversions
    (4096, 4, None, T16, 3, 3, 3, True, [(4, 1, None), (3, 1, None)]),
    (16384, 4, None, T32, 3, 2, 2, False,                                                # fused; the second product drops Y alone
     [(4, 1, None), (3, 1, None), (4, 0, None), (3, 0, None), (4, 1, 1), (3, 1, 1)]),
    (16384, 5, None, T32, 3, 1, 1, False, [(2, 1, None)]),                               # folded ring, a pair the fused kernel is not built for
    (16384, 3, "one_p_61", T32, 2, 1, 1, False, [(2, 1, None)]),                         # the parent context does not fold, the level does
    (4096, 3, None, T16, 1, 3, 1, False, [(3, 1, None), (2, 1, None)]),                  # K = 1: nothing may change
    (16384, 6, None, T32, 3, 1, 1, False, [([5, 4], 1, None), ([6, 4], 1, None)]),       # chain schedule, fused: X from level 5 (triple), from L (pair)
    (16384, 2, "below_2^50", T32, 2, 1, 1, False, [(2, 1, None), (1, 1, None), (2, 0, None)]),   # folded, moduli below 2^59
]
# piehip_base_convert: (N, L, chain, t)
CONVERT_SHAPES = [(2048, 3, None, T16), (2048, 3, "q0_wide", T16)]


def chain_moduli(N, L, chain):
    from tests.param_chains import named_chain, uniform_chain
    if not chain:
        return None, None
    if chain.startswith("below_2^"):
        return uniform_chain(N, L, below=1 << int(chain[8:]))
    return named_chain(N, L, chain)


def rand_limbs(rng, moduli, shape_prefix, N):
    out = np.zeros(tuple(shape_prefix) + (len(moduli), N), dtype=np.uint64)
    for i, m in enumerate(moduli):
        out[..., i, :] = rng.integers(0, int(m), tuple(shape_prefix) + (N,), dtype=np.uint64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libpiehip.so")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    from nested_hashing_psi_amd import _lib, pie
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        import ctypes
        other = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SYMBOLS if not hasattr(other, n)]:   # an older build: the entry points it lacks are not used here
            del _lib.SYMBOLS[name]
    lines = []
    for N, L, chain, t, K, b, nq, key_per_query, settings in SHAPES:
        q, p = chain_moduli(N, L, chain)
        cc = pie.PieContext(N, L, t, q, p)
        Q = cc.moduli[:L]
        E = 2 + (N // 64 + K) % 2
        rng = np.random.default_rng(N + 100 * K + 10 * b + nq + L)
        op = pie.BatchedFHEHIPPIE(cc, vectorizedHCT=rand_limbs(rng, Q, (K, b, E), N), preCalcRandomMask=rand_limbs(rng, Q, (b,), N))
        if nq > 1:
            op.setQueryBatch(nq)
        for i in range(nq):
            op.setMinusCompareElement(rand_limbs(rng, Q, (2,), N), query=i)
            op.setIndex(rand_limbs(rng, Q, (K, E, 2), N), query=i)
        if key_per_query:
            for i in range(nq):
                cc.load_relin_key(rand_limbs(rng, Q, (L, 2), N), query=i)
        elif K > 1:
            cc.load_relin_key(rand_limbs(rng, Q, (L, 2), N))
        cc.set_run_streams(1)
        for Lc, relin, keep in settings:
            op.setResultRelin(bool(relin))
            op.setResultLimbs(keep or L)
            if isinstance(Lc, list):
                op.setChainSchedule(Lc)
            else:
                op.setChainLimbs(Lc)
            cc.set_profiling(True)
            op.run()
            prof = cc.profile()
            cc.set_profiling(False)
            lines.append(json.dumps({
                "shape": {"N": N, "L": L, "chain": chain or "default", "K": K, "b": b, "E": E, "nq": nq, "key_per_query": key_per_query},
                "setting": {"chain_limbs": Lc, "result_relin": relin, "result_limbs": keep or L},
                "launches": {k: {"launches": v["launches"], "alg_bytes": v["alg_bytes"]} for k, v in sorted(prof.items())}}, sort_keys=True))
        cc.close()
    for N, L, chain, t in CONVERT_SHAPES:
        q, p = chain_moduli(N, L, chain)
        cc = pie.PieContext(N, L, t, q, p)
        rng = np.random.default_rng(N + L)
        for which in (0, 1, 2):
            polys = rand_limbs(rng, cc.moduli[:cc.M if which == 2 else L], (3 if which == 2 else 2,), N)   # a triple; a pair
            cc.set_profiling(True)
            cc.base_convert(which, polys)
            prof = cc.profile()
            cc.set_profiling(False)
            lines.append(json.dumps({
                "shape": {"N": N, "L": L, "chain": chain or "default"}, "base_convert": which,
                "launches": {k: {"launches": v["launches"], "alg_bytes": v["alg_bytes"]} for k, v in sorted(prof.items())}}, sort_keys=True))
        cc.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
