// kernels_convert.hip -- the HPS base conversions in front of a ciphertext multiplication (row A6): one conversion as a launch of
// its own, and both operands of a product in one launch.  The cores are pie_convert.h's; the forms of a level context (plain operands,
// a limb drop in front) are kernels_chain_drop.hip's.
#include "pie_convert.h"

namespace piehip {

// (The kind is a template argument of every conversion kernel: a context with NttPlan::fold_moduli runs the instantiations at ArithKind::fold.)
template <bool SCALE, bool FOLD, u32 L, ArithKind K, bool SKIPQ>
__global__ void __launch_bounds__(TPB) expand_kernel(const DevConsts *__restrict__ dc, u32 N, const u64 *__restrict__ in,
                                                     size_t so, size_t si, u64 *__restrict__ out, u32 out_polys, u32 out_slot)
{
    expand_body<SCALE, FOLD, L, K, SKIPQ>(dc, dc, N, in, so, si, out, out_polys, out_slot, blockIdx.y);
}
// Both operands of a ciphertext multiplication in one launch: rows [0, 2 n) of the grid scale operand Y (P/Q scaling, the
// longer body: first, so that the shorter rows fill in behind it), rows [2 n, 4 n) lift operand X.  As two launches each was
// a single round of 3.5 / 1.75 waves per SIMD with every wave in the same load - compute - store phase; together the rounds
// interleave (12.4 + 20.6 us -> one launch).  Writes out[n][4][M][N]: X into slots 0, 1, Y into slots 2, 3.
template <bool FOLD, u32 L, ArithKind K, bool SKIPQ>
__global__ void __launch_bounds__(TPB) expand_both_kernel(const DevConsts *__restrict__ dc, u32 N, const u64 *__restrict__ x, size_t sx,
                                                          const u64 *__restrict__ y, size_t sy, size_t si, u64 *__restrict__ out,
                                                          u32 n_outer)
{
    if (blockIdx.y < 2 * n_outer)
        expand_body<true, FOLD, L, K, false>(dc, dc, N, y, sy, si, out, 4, 2, blockIdx.y);
    else
        expand_body<false, FOLD, L, K, SKIPQ>(dc, dc, N, x, sx, si, out, 4, 0, blockIdx.y - 2 * n_outer);
}
// One conversion as a launch of its own (piehip_base_convert): plain operands of a context without folding in the call, nothing in place
static void launch_expand_common(bool scale, const DevConsts *dc, u32 N, u32 L, const u64 *in, size_t so, size_t si, u32 n_outer, u64 *out,
                                 u32 out_polys, u32 out_slot, hipStream_t st, Arith ar)
{
    dim3 grid((N + TPB - 1) / TPB, n_outer * 2);
    with_u32<1, 7>(L, [&](auto L_) {
        with_arith(ar, [&](auto K_) {
            with_bools([&](auto S_) {
                hipLaunchKernelGGL((expand_kernel<S_(), false, L_(), K_(), false>), grid, dim3(TPB), 0, st, dc, N, in, so, si, out, out_polys, out_slot);
            }, scale);
        });
    });
}
void launch_expand_q_to_qp(const DevConsts *dc, u32 N, u32 L, const u64 *in, size_t so, size_t si, u32 n_outer, u64 *out,
                           u32 out_polys, u32 out_slot, hipStream_t st, Arith ar)
{
    launch_expand_common(false, dc, N, L, in, so, si, n_outer, out, out_polys, out_slot, st, ar);
}
void launch_scale_pq_expand(const DevConsts *dc, u32 N, u32 L, const u64 *in, size_t so, size_t si, u32 n_outer, u64 *out,
                            u32 out_polys, u32 out_slot, hipStream_t st, Arith ar)
{
    launch_expand_common(true, dc, N, L, in, so, si, n_outer, out, out_polys, out_slot, st, ar);
}

// Both conversions of a product (kernels.hpp): the kernel follows from how the two operands arrive
bool launch_expand_pair(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y, u32 n_outer, u64 *out,
                        hipStream_t st, Arith ar, bool fold)
{
    const bool ydrop = y.src_L > L, xdrop = x.src_L > L;
    const dim3 grid(((fold ? N / 2 : N) + TPB - 1) / TPB, n_outer * 4), block(TPB);
    if (ydrop) return launch_expand_pair_drop(dc, N, L, x, y, n_outer, out, st, ar, fold);   // (kernels_chain_drop.hip)
    if (xdrop || x.plain != y.plain) return false;
    if (x.plain) return launch_expand_pair_plain(dc, N, L, x, y, n_outer, out, st, ar, fold);   // (kernels_chain_drop.hip)
    if (fold && !x.q_ready) return false;   // (a folded context has plan.xq_reuse: its X always arrives with the Q limbs in place)
    return x.poly == y.poly && with_u32<1, 7>(L, [&](auto L_) {
        with_arith(ar, [&](auto K_) {
            auto launch = [&](auto F_, auto Q_) {
                hipLaunchKernelGGL((expand_both_kernel<F_(), L_(), K_(), Q_()>), grid, block, 0, st, dc, N, x.p, x.row, y.p, y.row, y.poly, out, n_outer);
            };
            if (fold) launch(std::true_type{}, std::true_type{});
            else with_bools([&](auto Q_) { launch(std::false_type{}, Q_); }, x.q_ready);
        });
    });
}

}  // namespace piehip
