// pie_kernel_common.h -- what the files of coefficient-wise kernels share (kernels_stage_a.hip, kernels_convert.hip,
// kernels_chain_drop.hip, kernels_keyswitch.hip, kernels_pie.hip): the block size, run-time values as template arguments, the
// per-iteration constant loads of the unrolled limb loops, and the outer-stage folding.  (kernels_slice.hip has a TPB of its own.)
#pragma once
#include <stdlib.h>

#include <cassert>

#include <algorithm>
#include <type_traits>

#include "kernels.hpp"
#include "madasm.h"
#include "stage_a_common.h"
#include "pie_arith.h"

namespace piehip {

static const u32 TPB = 256;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// Run-time values as template arguments.  with_u32<LO, HI>(v, f) (stage_a_common.h) calls f(std::integral_constant<u32, v>) for v in
// [LO, HI] and says whether it did; with_bools(f, b...) calls f(std::bool_constant<b>...).  The callers' generic lambdas read the
// arguments as constants (L_(), F_()) and guard with `if constexpr` whatever combination no kernel is built for.  with_arith(ar, f)
// calls f(std::integral_constant<ArithKind, ar.kind>): the arithmetic kind every kernel here takes as ONE template argument (K_()).
template <class F>
static void with_bools(F &&f)
{
    f();
}
template <class F, class... Bs>
static void with_bools(F &&f, bool b, Bs... rest)
{
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
template <class F>
static void with_arith(Arith ar, F &&f)
{
    switch (ar.kind) {
        case ArithKind::wide: f(std::integral_constant<ArithKind, ArithKind::wide>{}); break;
        case ArithKind::barrett: f(std::integral_constant<ArithKind, ArithKind::barrett>{}); break;
        case ArithKind::fold: f(std::integral_constant<ArithKind, ArithKind::fold>{}); break;
    }
}

// The per-limb iterations of the base conversions are unrolled (the residue arrays must stay in registers), and each
// iteration needs its own dozen table entries: moduli, Barrett and Shoup constants, one column of a conversion matrix.
// Left alone, the compiler loads all of them at the top of the kernel -- 200+ scalar registers' worth -- and spills them
// into vector lanes (a third of the instructions of these kernels were v_readlane / v_writelane / v_mov).  So every
// iteration starts with a scheduling fence and reads its constants through a freshly laundered pointer into the
// constant address space: scalar loads, issued in that iteration, dead at its end.
#define PIE_ITER_FENCE() __builtin_amdgcn_sched_barrier(0)
typedef const __attribute__((address_space(4))) DevConsts *DcC;
__device__ __forceinline__ DcC dc_iter(const DevConsts *dc)
{
    u64 v = (u64)dc;
    asm volatile("" : "+s"(v));
    return (DcC)v;
}
__device__ __forceinline__ Mod ld_mod(DcC c, u32 i)
{
    Mod m;
    m.q = c->mod[i].q, m.r0 = c->mod[i].r0, m.r1 = c->mod[i].r1, m.n_inv = 0, m.n_inv_sh = 0;
    m.fconst = c->mod[i].fconst, m.fshift = c->mod[i].fshift, m.pad = 0;
    return m;
}

// Outer-stage folding.  For N >= 2^14 the transforms next to these kernels run as two half-size slices per limb
// (two workgroups per CU, finer scheduling granularity) and the outermost radix-2 stage moves here, where both
// coefficients n and n + N/2 of every limb pass through registers anyway:
//   load side  (input comes from an inverse transform):  (u, v) -> ((u + v) N^-1, (u - v) psi^{-N/2} N^-1)
//   store side (output goes to a forward transform):     (u, v) -> (u + v psi^{N/2}, u - v psi^{N/2})
// The folded inverse transform hands over unnormalised residues in [0, 4q) and the forward transform takes anything
// below 8q, so neither side reduces sums or differences: the Shoup product accepts any 64-bit operand.
__device__ __forceinline__ void fold_load(const DevConsts *dc, u32 a, u64 u, u64 v, u64 &x0, u64 &x1)
{
    PIE_ITER_FENCE();
    const DcC c = dc_iter(dc);
    const u64 q = c->mod[a].q, nq = neg_u(q);
    x0 = shoup63(u + v, c->fold_ia[a], c->fold_ia_sh[a], nq);            // (folding implies q < 2^60)
    x1 = shoup63(u + (4 * q - v), c->fold_ib[a], c->fold_ib_sh[a], nq);
}
// u in [0, 4q) (canonical, or left unreduced by the base conversions: LZ); results in (0, 8q)
__device__ __forceinline__ void fold_store(const DevConsts *dc, u32 a, u64 u, u64 v, u64 &y0, u64 &y1)
{
    const DcC c = dc_iter(dc);
    const u64 q = c->mod[a].q;
    const u64 t = shoup63_lazy(v, c->fold_w[a], c->fold_w_sh[a], neg_u(q));  // [0, 4q)
    y0 = u + t;
    y1 = u + (4 * q - t);
}

}  // namespace piehip
