// kernels_ntt16.hip -- launch side of the 16-coefficients-per-thread NTT (ntt16_kernel.h) for slices of 2^13 coefficients:
// ring 2^13 as one slice per limb, ring 2^14 as two slices with the outermost stage folded into the neighbouring kernels.
// Replaces DCRTPoly::SetFormat under EvalMult(ct, ct) (reference BatchedFHEHIPPIE.cpp:123).
#include <cassert>

#include "kernels.hpp"
#include "ntt16_kernel.h"

namespace piehip {

void build_twk16_table(const u64 *nat_pairs, u32 s0, u32 slice_log, std::vector<u64> &out)
{
    if (slice_log == 14)
        ntt16::build_twk_table_t<14>(nat_pairs, s0, out);
    else
        ntt16::build_twk_table_t<13>(nat_pairs, s0, out);
}

void ntt16_sigma_inverse_map(u32 logN, u32 s0, std::vector<u32> &map)
{
    const u32 N = 1u << logN, n = N >> s0;
    map.resize(N);
    for (u32 p = 0; p < N; p++) map[p] = (p / n) * n + ntt16::lane_to_std_t(p % n, n / 16);
}

// one launch of one instantiation: its dynamic LDS limit is raised where it first runs on a device
template <u32 LOGNS, auto KERNEL>
static void launch_ntt16_k(const ntt16::Args &a, u32 num_cus, hipStream_t st)
{
    typedef ntt16::Geo<LOGNS> G;
    constexpr size_t lds = (size_t)G::LDS_WORDS * sizeof(u64);
    static PerDeviceOnce attr;
    if (attr.first_on_current_device()) (void)hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // resident workgroups per CU: two of 512 threads (68 KiB of LDS, 128 VGPRs each) or one of 1024 (136 KiB); persistent beyond
    const u32 slots = (LOGNS == 13 ? 2u : 1u) * num_cus;
    const u32 grid = a.nitems < slots ? a.nitems : slots;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(G::T), lds, st, a);
}
// the four launch kinds of a slice length at one arithmetic kind: forward, forward with the digit lift, inverse, and the inverse with the
// tensor load phase
template <u32 LOGNS, ArithKind KIND>
static void launch_ntt16_kind(const ntt16::Args &a, bool inverse, bool lift, u32 num_cus, hipStream_t st, bool tensor)
{
    using ntt16::ntt16_kernel_t;
    if (tensor) launch_ntt16_k<LOGNS, ntt16_kernel_t<LOGNS, true, false, true, KIND>>(a, num_cus, st);
    else if (inverse) launch_ntt16_k<LOGNS, ntt16_kernel_t<LOGNS, true, false, false, KIND>>(a, num_cus, st);
    else if (lift) launch_ntt16_k<LOGNS, ntt16_kernel_t<LOGNS, false, true, false, KIND>>(a, num_cus, st);
    else launch_ntt16_k<LOGNS, ntt16_kernel_t<LOGNS, false, false, false, KIND>>(a, num_cus, st);
}
// fd: every modulus of the launch is 2^60 - d with d < COLACC_FOLD_MAX_D -- ArithKind::fold (the butterflies, the canonical forward store, the
// column sums of the tensor load phase)
template <u32 LOGNS>
static void launch_ntt16_t(const ntt16::Args &a, bool inverse, bool lift, u32 num_cus, hipStream_t st, bool tensor = false, bool fd = false)
{
    if (fd) return launch_ntt16_kind<LOGNS, ArithKind::fold>(a, inverse, lift, num_cus, st, tensor);
    launch_ntt16_kind<LOGNS, ArithKind::barrett>(a, inverse, lift, num_cus, st, tensor);
}
// A plan with fold_moduli speaks of its Q and P moduli [0, fold_mod_count); the plaintext modulus behind them (the client's transforms
// mod t) is of another shape and keeps the Barrett kind.
static bool launch_folds(const NttPlan &pl, u32 mod_base, u32 mod_count) { return pl.fold_moduli && mod_base + mod_count <= pl.fold_mod_count; }

void launch_ntt16(const NttPlan &pl, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inverse, bool sigma, hipStream_t st,
                  const NttExtra *ex, const Ntt16Digits *dg)
{
    const bool folded = pl.fold;
    const u32 s0 = folded ? 1u : 0u;
    assert(ntt_route(pl, inverse, sigma, folded).kernel == NttKernel::blocked16 && (!dg || pl.digits_with_d01));
    ntt16::Args a;
    a.data = data;
    a.twp = reinterpret_cast<const ntt16::u64x2 *>(pl.twp);
    a.twk = reinterpret_cast<const ntt16::u64x2 *>(pl.twk16);
    a.dc = pl.dc;
    a.N = pl.N;
    a.s0 = s0;
    a.nitems = nlimbs << s0;
    a.mod_base = mod_base;
    a.mod_count = mod_count;
    a.flags = 0;
    if (inverse && !sigma) a.flags |= ntt16::F_STD_IN;
    if (inverse && folded) a.flags |= ntt16::F_FOLDED;
    if (inverse && !sigma && ex && ex->copy_out && ex->x_lane_in) a.flags |= ntt16::F_X_LANE_IN;
    if (!inverse && ex && ex->lazy_out) a.flags |= ntt16::F_LAZY_OUT;
    a.skip_L = (ex && !inverse) ? ex->skip_L : 0;
    a.skip_M = ex ? ex->skip_M : 0;
    a.copy_out = (ex && inverse && !sigma) ? ex->copy_out : nullptr;
    a.copy_K = ex ? ex->copy_K : 1;
    a.copy_L = ex ? ex->copy_L : 1;
    a.copy_M = ex ? ex->copy_M : 1;
    a.lift_first = ~0u;
    a.data2 = nullptr;
    a.lift_src = nullptr;
    a.lift_stride = 0;
    a.lift_L = 1;
    a.tsrc = nullptr;
    a.tq_L = 0;
    a.tq_first = 0;
    if (dg && !inverse) {  // the key-switch digits ride in the same launch: nb * L * L more limbs, lifted in the load phase
        a.lift_first = a.nitems;
        a.nitems += (dg->nb * dg->L * dg->L) << s0;
        a.data2 = dg->dig;
        a.lift_src = dg->d2;
        a.lift_stride = dg->stride2;
        a.lift_L = dg->L;
    }
    const bool lift = a.lift_first != ~0u;
    const bool fd = launch_folds(pl, mod_base, mod_count) && (!dg || dg->L <= pl.fold_mod_count);
    if (pl.lane_logn == 14)
        launch_ntt16_t<14>(a, inverse, lift, pl.transform_cus(), st, false, fd);
    else
        launch_ntt16_t<13>(a, inverse, lift, pl.transform_cus(), st, false, fd);
}

void launch_ntt16_tensor(const NttPlan &pl, const u64 *e, u64 *d, u32 nb, u32 M, hipStream_t st, u32 eval_q_L, bool eval_q_d2)
{
    assert(pl.fused_tensor && (!eval_q_L || ((eval_q_d2 ? pl.result_eval_q : pl.d01_eval_q) && eval_q_L < M)) && (!eval_q_d2 || eval_q_L));
    const bool folded = pl.fold;
    const u32 s0 = folded ? 1u : 0u;
    ntt16::Args a = {};
    a.data = d;
    a.twp = reinterpret_cast<const ntt16::u64x2 *>(pl.twp);
    a.twk = reinterpret_cast<const ntt16::u64x2 *>(pl.twk16);
    a.dc = pl.dc;
    a.N = pl.N;
    a.s0 = s0;
    a.tq_L = eval_q_L;
    a.tq_first = (nb * 3 * (M - eval_q_L)) << s0;
    a.nitems = a.tq_first + (eval_q_d2 ? 0u : (nb * eval_q_L) << s0);  // 3 M - 2 eval_q_L limbs per row; eval_q_d2: the P limbs' triples alone
    a.mod_base = 0;
    a.mod_count = M;
    a.flags = folded ? ntt16::F_FOLDED : 0;
    a.copy_K = a.copy_L = a.copy_M = 1;
    a.lift_first = ~0u;
    a.lift_L = 1;
    a.tsrc = e;
    if (pl.lane_logn == 14)
        launch_ntt16_t<14>(a, true, false, pl.transform_cus(), st, true, pl.fold_moduli);
    else
        launch_ntt16_t<13>(a, true, false, pl.transform_cus(), st, true, pl.fold_moduli);
}

}  // namespace piehip
