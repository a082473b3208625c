// kernels_ntt.hip -- negacyclic NTT / inverse NTT over 60-bit RNS primes for gfx950.
//
// Replaces DCRTPoly::SetFormat (OpenFHE) under EvalMult(ct,ct), reference call site
// src/Common/Crypto/PrivateIndexedEqualityCheck/BatchedFHEHIPPIE.cpp:123.
// Forward: Cooley-Tukey, natural order in, bit-reversed order out, twiddles psi^bitrev(k).
// Inverse: Gentleman-Sande, bit-reversed in, natural out, scaled by N^-1.
// Harvey lazy butterflies with Shoup twiddles; canonical residues in and out.
//
// One workgroup owns one limb (or one 2^-s0 slice of it) and keeps it in LDS for all of its
// stages: one coalesced HBM read and one write per limb-NTT (16 N bytes, the algorithmic minimum).
// A limb of N = 16384 is 128 KiB of the CU's 160 KiB LDS; N = 32768 runs its outermost stage as a
// streaming pass over global memory and the rest as two 16384-point LDS transforms.
#include "kernels.hpp"

#include <algorithm>
#include <cassert>

namespace piehip {

static const u32 NTT_LDS_MAX_LOG = 14;  // 2^14 coefficients * 8 B = 128 KiB

struct NttArgs {
    u64 *data;
    const u64 *tables;
    const DevConsts *dc;
    u32 N, logN;
    u32 s0;  // log2 of the number of LDS slices per limb (stages m < 2^s0 run in global memory)
    u32 mod_base, mod_count;
};

// ---------------------------------------------------------------------------------------------
// generic LDS kernel: radix-2 stages with a barrier per stage.  Works for every N >= 64; the
// specialised radix-16 register kernels below take over for the production sizes.
// ---------------------------------------------------------------------------------------------
template <bool INV>
__global__ void __launch_bounds__(1024) ntt_lds_generic(NttArgs a)
{
    extern __shared__ u64 s[];
    const u32 tid = threadIdx.x, nthr = blockDim.x;
    const u32 nl = a.N >> a.s0;                       // coefficients in this slice
    const u32 limb = blockIdx.x >> a.s0, blk = blockIdx.x & ((1u << a.s0) - 1);
    const u32 mod = a.mod_base + limb % a.mod_count;
    const Mod m = a.dc->mod[mod];
    const u64 q = m.q, q2 = 2 * m.q;
    const u64 *tw = a.tables + (size_t)mod * 4 * a.N + (INV ? 2 * (size_t)a.N : 0);
    const u64 *tws = tw + a.N;
    u64 *g = a.data + (size_t)limb * a.N + (size_t)blk * nl;

    for (u32 i = tid; i < nl; i += nthr) s[i] = g[i];
    __syncthreads();

    if (!INV) {
        u32 logt = a.logN - a.s0 - 1;
        for (u32 ml = 1; ml < nl; ml <<= 1, logt--) {
            const u32 t = 1u << logt;
            for (u32 bi = tid; bi < nl / 2; bi += nthr) {
                const u32 i = bi >> logt, j = bi & (t - 1);
                const u32 x = (i << (logt + 1)) + j;
                const u32 k = (ml << a.s0) + blk * ml + i;
                const u64 w = tw[k], ws = tws[k];
                u64 u = s[x];
                u = u >= q2 ? u - q2 : u;
                const u64 v = mul_shoup_lazy(s[x + t], w, ws, q);
                s[x] = u + v;
                s[x + t] = u - v + q2;
            }
            __syncthreads();
        }
        for (u32 i = tid; i < nl; i += nthr) {
            u64 v = s[i];
            v = v >= q2 ? v - q2 : v;
            g[i] = v >= q ? v - q : v;
        }
    } else {
        u32 logt = 0;
        for (u32 hl = nl >> 1; hl >= 1; hl >>= 1, logt++) {
            const u32 t = 1u << logt;
            for (u32 bi = tid; bi < nl / 2; bi += nthr) {
                const u32 i = bi >> logt, j = bi & (t - 1);
                const u32 x = (i << (logt + 1)) + j;
                const u32 k = (hl << a.s0) + blk * hl + i;
                const u64 w = tw[k], ws = tws[k];
                const u64 u = s[x], v = s[x + t];
                const u64 sm = u + v;
                s[x] = sm >= q2 ? sm - q2 : sm;
                s[x + t] = mul_shoup_lazy(u - v + q2, w, ws, q);
            }
            __syncthreads();
        }
        if (a.s0 == 0) {
            for (u32 i = tid; i < nl; i += nthr) g[i] = mul_shoup(s[i], m.n_inv, m.n_inv_sh, q);
        } else {
            for (u32 i = tid; i < nl; i += nthr) {
                u64 v = s[i];
                g[i] = v >= q ? v - q : v;
            }
        }
    }
}

// one outer stage in global memory (only N > 2^14 needs it): forward stage with m groups, or the
// matching inverse stage; canonical in and out.  The last inverse stage also applies N^-1.
template <bool INV>
__global__ void __launch_bounds__(256) ntt_global_stage(NttArgs a, u32 mstage, u32 last_inverse)
{
    const u32 half = a.N >> 1;
    const u32 bi = blockIdx.x * 256 + threadIdx.x;  // butterfly within the limb
    const u32 limb = blockIdx.y;
    if (bi >= half) return;
    const u32 mod = a.mod_base + limb % a.mod_count;
    const Mod m = a.dc->mod[mod];
    const u64 q = m.q;
    const u64 *tw = a.tables + (size_t)mod * 4 * a.N + (INV ? 2 * (size_t)a.N : 0);
    const u64 *tws = tw + a.N;
    u32 logm = 0;
    while ((1u << logm) < mstage) logm++;
    const u32 logt = a.logN - 1 - logm, t = 1u << logt;
    const u32 i = bi >> logt, j = bi & (t - 1);
    const size_t x = (size_t)limb * a.N + ((size_t)i << (logt + 1)) + j;
    const u64 w = tw[mstage + i], ws = tws[mstage + i];
    const u64 u = a.data[x], v = a.data[x + t];
    if (!INV) {
        const u64 p = mul_shoup(v, w, ws, q);
        a.data[x] = addmod(u, p, q);
        a.data[x + t] = submod(u, p, q);
    } else {
        u64 sm = addmod(u, v, q);
        u64 df = mul_shoup(submod(u, v, q), w, ws, q);
        if (last_inverse) {
            sm = mul_shoup(sm, m.n_inv, m.n_inv_sh, q);
            df = mul_shoup(df, m.n_inv, m.n_inv_sh, q);
        }
        a.data[x] = sm;
        a.data[x + t] = df;
    }
}

static PerDeviceOnce g_attr_set[2];

// The one place that knows which kernel a call takes
NttRoute ntt_route(const NttPlan &pl, bool inverse, bool sigma, bool folded)
{
    assert((!sigma || pl.lane_order) && (!folded || pl.fold));
    const u32 s0 = pl.logN > NTT_LDS_MAX_LOG ? pl.logN - NTT_LDS_MAX_LOG : 0;  // slices that fit the LDS; the stages above run in global memory
    if (!pl.lane_order) return {NttKernel::radix2, s0, s0};
    // the 16-coefficient kernel: the calls of its own slicing whose EVALUATION side is in lane order, and every inverse among them
    if (pl.lane_kernel == NttKernel::blocked16 && folded == pl.fold && (inverse || sigma)) return {NttKernel::blocked16, folded ? 1u : 0u, 0};
    if (folded) return {NttKernel::blocked32, 1, 0};
    return {NttKernel::blocked32, s0, s0};
}

void ntt_plan_decide(NttPlan &pl, bool lazy_ok, bool small_moduli, bool fold_moduli)
{
    pl.lane_order = lazy_ok && pl.logN >= 12;
    pl.small_moduli = small_moduli;
    pl.fold_moduli = small_moduli && fold_moduli;
    if (!pl.lane_order) return;
    const bool k16 = pl.logN >= 13 && pl.logN <= 15;
    pl.lane_kernel = k16 ? NttKernel::blocked16 : NttKernel::blocked32;
    pl.fold = pl.logN == 14 || pl.logN == 15;
    pl.lane_logn = pl.logN - ntt_route(pl, true, true, pl.fold).s0;
    pl.lane_T = (1u << pl.lane_logn) / (k16 ? 16 : 32);
    pl.lane_kp = k16 ? 8 : 16;
    pl.xq_reuse = ntt_route(pl, true, false, pl.fold).extra();
    pl.fused_tensor = PIEHIP_FUSE_TENSOR && k16 && small_moduli;
    // (the transform of the own-limb term is added where d01 and the QP operands have the same order: the lane order of one kernel)
    pl.d01_eval_q = PIEHIP_D01_EVAL_Q && pl.fused_tensor;
    // (... and a product that is not relinearised leaves d2's Q limbs there as well: launch_deg2_finish writes its three components)
    pl.result_eval_q = PIEHIP_RESULT_EVAL_Q && pl.fused_tensor && deg2_finish_applies(pl.N, pl.lane_T, pl.lane_kp);
    pl.digits_with_d01 = k16 && small_moduli;  // equal-width primes only: the kernel's lift is a conditional subtraction
    pl.x_direct = pl.xq_reuse && k16 && small_moduli;
    const NttRoute std_fwd = ntt_route(pl, false, false, false);  // the digit lift is in the 32-coefficient kernel, one slice per limb
    pl.digit_lift_std = std_fwd.kernel == NttKernel::blocked32 && std_fwd.s0 == 0;
    pl.digit_lift_lane = pl.digit_lift_std && !k16;  // a 16-coefficient lane order: digits kernel + transform (or digits_with_d01)
}

void launch_ntt_digits(const NttPlan &pl, const u64 *d2, u64 *dig, u32 nb, u32 L, bool sigma, hipStream_t st)
{
    assert(sigma ? pl.digit_lift_lane : pl.digit_lift_std);
    launch_ntt_fast(pl, pl.twc, 0, dig, nb * L * L, 0, L, false, sigma, st, d2, L);
}

void launch_ntt(const NttPlan &pl, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inverse, hipStream_t st, bool sigma,
                bool folded, const NttExtra *ex)
{
    if (!nlimbs) return;
    const NttRoute r = ntt_route(pl, inverse, sigma, folded);
    // A route with global stages does not honour the copy or the compact enumeration (the stages walk every limb, and the plan has
    // no xq_reuse there): a caller that passes them all the same gets the plain transform.  lazy_out stays: the slice kernel stores last
    NttExtra plain;
    if (ex && !r.extra()) {
        plain.lazy_out = ex->lazy_out;
        ex = &plain;
    }
    if (r.kernel == NttKernel::blocked16) {
        launch_ntt16(pl, data, nlimbs, mod_base, mod_count, inverse, sigma, st, ex);
        return;
    }
    if (folded) {  // two half-size slices per limb, outer stage done by the neighbouring kernels (forward, standard order: see ntt_route)
        launch_ntt_fast(pl, pl.twc_fold, 1, data, nlimbs, mod_base, mod_count, inverse, sigma, st, nullptr, 0, ex);
        return;
    }
    NttArgs a;
    a.data = data;
    a.tables = pl.tables;
    a.dc = pl.dc;
    a.N = pl.N;
    a.logN = pl.logN;
    a.s0 = r.s0;
    a.mod_base = mod_base;
    a.mod_count = mod_count;
    const u32 nl = pl.N >> a.s0;
    const size_t lds = (size_t)nl * sizeof(u64);
    const u32 threads = std::min(std::max(nl / 2, 64u), 1024u);
    const bool radix2 = r.kernel == NttKernel::radix2;
    // a workgroup may use up to 160 KiB of LDS on gfx950; raise the dynamic-LDS cap once
    if (radix2 && g_attr_set[inverse ? 1 : 0].first_on_current_device())
        (void)hipFuncSetAttribute(inverse ? (const void *)ntt_lds_generic<true> : (const void *)ntt_lds_generic<false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (1 << NTT_LDS_MAX_LOG) * 8);
    const dim3 ggrid((pl.N / 2 + 255) / 256, nlimbs);
    if (!inverse) {
        for (u32 ms = 1; ms < (1u << r.global_stages); ms <<= 1)
            hipLaunchKernelGGL(ntt_global_stage<false>, ggrid, dim3(256), 0, st, a, ms, 0u);
        if (radix2) hipLaunchKernelGGL(ntt_lds_generic<false>, dim3(nlimbs << a.s0), dim3(threads), lds, st, a);
    } else if (radix2) {
        hipLaunchKernelGGL(ntt_lds_generic<true>, dim3(nlimbs << a.s0), dim3(threads), lds, st, a);
    }
    if (!radix2) launch_ntt_fast(pl, pl.twc, r.s0, data, nlimbs, mod_base, mod_count, inverse, sigma, st, nullptr, 0, ex);
    if (inverse)
        for (u32 ms = (1u << r.global_stages) >> 1; ms >= 1; ms >>= 1)
            hipLaunchKernelGGL(ntt_global_stage<true>, ggrid, dim3(256), 0, st, a, ms, ms == 1 ? 1u : 0u);
}

}  // namespace piehip
