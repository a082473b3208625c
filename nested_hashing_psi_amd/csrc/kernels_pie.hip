// kernels_pie.hip -- the small element-wise kernels around BatchedFHEHIPPIE::run() for gfx950: the host flag, EvalAdd and
// EvalMult(ct, pt), automorphism permutation, the rotation-based sibling operator's helpers, packed encoding.  The families that
// used to live here: kernels_stage_a.hip, kernels_convert.hip, kernels_chain_drop.hip, kernels_keyswitch.hip (pie_kernel_common.h
// holds what they share).
#include "pie_kernel_common.h"

namespace piehip {

// One word for the host: `value` lands in page-locked host memory when everything queued on the stream before it is done
// (piehip_host.cpp: "the uploads of this query have left host memory" -- an event cannot say that once kernels are queued
// behind the uploads: hipEventSynchronize on an earlier event waits for the stream's whole backlog).
__global__ void host_flag_kernel(volatile u64 *flag, u64 value)
{
    *flag = value;
    __threadfence_system();
}
void launch_host_flag(u64 *flag_dev, u64 value, hipStream_t st)
{
    hipLaunchKernelGGL(host_flag_kernel, dim3(1), dim3(1), 0, st, (volatile u64 *)flag_dev, value);
}

// ---------------------------------------------------------------------------------------------
// EvalAdd / EvalMult(ct,pt) as stand-alone element-wise kernels (rows A3, A4)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) ct_add_kernel(const DevConsts *dc, u32 N, u32 L, const u64 *__restrict__ x,
                                                     const u64 *__restrict__ y, u64 *__restrict__ out)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const u32 l = blockIdx.y % L;
    const size_t o = ((size_t)blockIdx.z * 2 * L + blockIdx.y) * N + n;
    out[o] = addmod(x[o], y[o], dc->mod[l].q);
}
void launch_ct_add(const DevConsts *dc, u32 N, u32 L, const u64 *x, const u64 *y, u64 *out, u32 nct, hipStream_t st)
{
    dim3 grid((N + TPB - 1) / TPB, 2 * L, nct);
    hipLaunchKernelGGL(ct_add_kernel, grid, dim3(TPB), 0, st, dc, N, L, x, y, out);
}
__global__ void __launch_bounds__(TPB) ct_mul_plain_kernel(const DevConsts *dc, u32 N, u32 L, const u64 *__restrict__ x,
                                                           const u64 *__restrict__ pt, size_t pt_stride,
                                                           u64 *__restrict__ out, u32 pt_div)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const u32 l = blockIdx.y % L;
    const size_t o = ((size_t)blockIdx.z * 2 * L + blockIdx.y) * N + n;
    out[o] = mulmod(x[o], pt[(size_t)(blockIdx.z / pt_div) * pt_stride + (size_t)l * N + n], dc->mod[l]);
}
// ... of `comps` components per ciphertext (3: a product that was not relinearised)
__global__ void __launch_bounds__(TPB) ctn_mul_plain_kernel(const DevConsts *dc, u32 N, u32 L, const u64 *__restrict__ x,
                                                            const u64 *__restrict__ pt, size_t pt_stride,
                                                            u64 *__restrict__ out, u32 pt_div, u32 comps)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const u32 l = blockIdx.y % L;
    const size_t o = ((size_t)blockIdx.z * comps * L + blockIdx.y) * N + n;
    out[o] = mulmod(x[o], pt[(size_t)(blockIdx.z / pt_div) * pt_stride + (size_t)l * N + n], dc->mod[l]);
}
void launch_ct_mul_plain(const DevConsts *dc, u32 N, u32 L, const u64 *x, const u64 *pt, size_t pt_stride, u64 *out,
                         u32 nct, hipStream_t st, u32 pt_div, u32 comps)
{
    dim3 grid((N + TPB - 1) / TPB, comps * L, nct);
    if (comps == 2)
        hipLaunchKernelGGL(ct_mul_plain_kernel, grid, dim3(TPB), 0, st, dc, N, L, x, pt, pt_stride, out, pt_div ? pt_div : 1);
    else
        hipLaunchKernelGGL(ctn_mul_plain_kernel, grid, dim3(TPB), 0, st, dc, N, L, x, pt, pt_stride, out, pt_div ? pt_div : 1, comps);
}

// ---------------------------------------------------------------------------------------------
// Automorphism permutation in EVALUATION format (row A9): out[r][p] = in[r][map[p]]
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) permute_kernel(u32 N, const u64 *__restrict__ in, const u32 *__restrict__ map,
                                                      u64 *__restrict__ out)
{
    const u32 p = blockIdx.x * TPB + threadIdx.x;
    if (p >= N) return;
    const size_t r = (size_t)blockIdx.y * N;
    out[r + p] = in[r + map[p]];
}
void launch_permute(u32 N, const u64 *in, const u32 *map, u64 *out, u32 nrows, hipStream_t st)
{
    dim3 grid((N + TPB - 1) / TPB, nrows);
    hipLaunchKernelGGL(permute_kernel, grid, dim3(TPB), 0, st, N, in, map, out);
}

// ---------------------------------------------------------------------------------------------
// Rotation-based PIE (FHEHIPPIE.cpp:61-77): EvalInnerProduct = ct x pt + log2 rotate-and-add steps, EvalMerge =
// mask slot 0, rotate ciphertext i by -i, add.  All steps batched over (PIE, bin).
// ---------------------------------------------------------------------------------------------
// out[i] = x[i / group] (.) pt[i / group][i % group]      (one index ciphertext against a group of plaintexts)
__global__ void __launch_bounds__(TPB) bcast_mul_plain_kernel(const DevConsts *dc, u32 N, u32 L, const u64 *__restrict__ x,
                                                              size_t xs, u32 group, const u64 *__restrict__ pt, size_t ps_outer,
                                                              size_t ps_inner, u64 *__restrict__ out)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const u32 l = blockIdx.y % L, i = blockIdx.z, g = i / group, r = i % group;
    const size_t LN = (size_t)L * N;
    const size_t o = (size_t)blockIdx.y * N + n;
    out[(size_t)i * 2 * LN + o] = mulmod(x[(size_t)g * xs + o], pt[(size_t)g * ps_outer + (size_t)r * ps_inner + (size_t)l * N + n], dc->mod[l]);
}
void launch_bcast_mul_plain(const DevConsts *dc, u32 N, u32 L, const u64 *x, size_t xs, u32 group, const u64 *pt, size_t ps_outer,
                            size_t ps_inner, u64 *out, u32 nct, hipStream_t st)
{
    dim3 grid((N + TPB - 1) / TPB, 2 * L, nct);
    hipLaunchKernelGGL(bcast_mul_plain_kernel, grid, dim3(TPB), 0, st, dc, N, L, x, xs, group, pt, ps_outer, ps_inner, out);
}
// Automorphism of ciphertext i with the EVALUATION index map maps[i % map_group]:
//   d01[i] = (acc ? x.c0 : 0) + x.c0 o map,  (acc ? x.c1 : 0)       (stays in EVALUATION format)
//   d2[i]  = x.c1 o map                                              (goes through the key switch)
// identity_first: position 0 of every group is not rotated (EvalMerge's first term): d01 = x, d2 = 0.
__global__ void __launch_bounds__(TPB) rot_prepare_kernel(const DevConsts *dc, u32 N, u32 L, const u64 *__restrict__ x,
                                                          const u32 *__restrict__ maps, u32 map_group, u32 acc, u32 identity_first,
                                                          u64 *__restrict__ d01, u64 *__restrict__ d2)
{
    const u32 p = blockIdx.x * TPB + threadIdx.x;
    if (p >= N) return;
    const u32 l = blockIdx.y, i = blockIdx.z, r = i % map_group;
    const size_t LN = (size_t)L * N;
    const u64 *c0 = x + (size_t)i * 2 * LN + (size_t)l * N, *c1 = c0 + LN;
    u64 *o0 = d01 + (size_t)i * 2 * LN + (size_t)l * N, *o1 = o0 + LN, *o2 = d2 + (size_t)i * LN + (size_t)l * N;
    if (identity_first && r == 0) {
        o0[p] = c0[p];
        o1[p] = c1[p];
        o2[p] = 0;
        return;
    }
    const u32 s = maps[(size_t)r * N + p];
    const u64 q = dc->mod[l].q;
    o0[p] = acc ? addmod(c0[p], c0[s], q) : c0[s];
    o1[p] = acc ? c1[p] : 0;
    o2[p] = c1[s];
}
void launch_rot_prepare(const DevConsts *dc, u32 N, u32 L, const u64 *x, const u32 *maps, u32 map_group, bool acc, bool identity_first,
                        u64 *d01, u64 *d2, u32 nct, hipStream_t st)
{
    dim3 grid((N + TPB - 1) / TPB, L, nct);
    hipLaunchKernelGGL(rot_prepare_kernel, grid, dim3(TPB), 0, st, dc, N, L, x, maps, map_group ? map_group : 1u, acc ? 1u : 0u,
                       identity_first ? 1u : 0u, d01, d2);
}
// out[g] = (sum_{r < group} x[g * group + r]) (.) pt[g]
__global__ void __launch_bounds__(TPB) sum_mul_plain_kernel(const DevConsts *dc, u32 N, u32 L, const u64 *__restrict__ x, u32 group,
                                                            const u64 *__restrict__ pt, size_t pt_stride, u64 *__restrict__ out,
                                                            size_t out_stride)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const u32 l = blockIdx.y % L, g = blockIdx.z;
    const size_t LN = (size_t)L * N;
    const size_t o = (size_t)blockIdx.y * N + n;
    const Mod m = dc->mod[l];
    u64 s = 0;
    for (u32 r = 0; r < group; r++) s = addmod(s, x[((size_t)g * group + r) * 2 * LN + o], m.q);
    out[(size_t)g * out_stride + o] = mulmod(s, pt[(size_t)g * pt_stride + (size_t)l * N + n], m);
}
void launch_sum_mul_plain(const DevConsts *dc, u32 N, u32 L, const u64 *x, u32 group, const u64 *pt, size_t pt_stride, u64 *out,
                          size_t out_stride, u32 ngroups, hipStream_t st)
{
    dim3 grid((N + TPB - 1) / TPB, 2 * L, ngroups);
    hipLaunchKernelGGL(sum_mul_plain_kernel, grid, dim3(TPB), 0, st, dc, N, L, x, group, pt, pt_stride, out, out_stride);
}

// ---------------------------------------------------------------------------------------------
// Packed encoding (row A2; MakePackedPlaintext at BatchedFHEHIPPIE.cpp:68,81)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) encode_scatter_kernel(const DevConsts *dc, u32 N, u32 M,
                                                             const int64_t *__restrict__ slots, u32 B,
                                                             const u32 *__restrict__ inv_pos, u64 *__restrict__ u)
{
    const u32 p = blockIdx.x * TPB + threadIdx.x;
    if (p >= N) return;
    const u64 t = dc->mod[M].q;
    const u32 s = inv_pos[p];
    u64 val = 0;
    if (s < B) {
        const int64_t v = slots[(size_t)blockIdx.y * B + s];
        const u64 mag = v < 0 ? (u64)(-v) : (u64)v;
        val = v < 0 ? (mag ? t - mag : 0) : mag;
    }
    u[(size_t)blockIdx.y * N + p] = val;
}
void launch_encode_scatter(const DevConsts *dc, u32 N, u32 M, const int64_t *slots, u32 B, const u32 *inv_pos, u64 *u,
                           u32 npt, hipStream_t st)
{
    dim3 grid((N + TPB - 1) / TPB, npt);
    hipLaunchKernelGGL(encode_scatter_kernel, grid, dim3(TPB), 0, st, dc, N, M, slots, B, inv_pos, u);
}
__global__ void __launch_bounds__(TPB) encode_lift_kernel(const DevConsts *dc, u32 N, u32 L, u32 M,
                                                          const u64 *__restrict__ u, u64 *__restrict__ out, u32 l0)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const u64 t = dc->mod[M].q;
    const u64 v = u[(size_t)blockIdx.z * N + n];
    const u64 q = dc->mod[l0 + blockIdx.y].q;
    out[((size_t)blockIdx.z * L + blockIdx.y) * N + n] = v > t / 2 ? q - (t - v) : v;  // centred lift
}
void launch_encode_lift(const DevConsts *dc, u32 N, u32 L, u32 M, const u64 *u, u64 *out, u32 npt, hipStream_t st, u32 l0)
{
    dim3 grid((N + TPB - 1) / TPB, L, npt);
    hipLaunchKernelGGL(encode_lift_kernel, grid, dim3(TPB), 0, st, dc, N, L, M, u, out, l0);
}

}  // namespace piehip
