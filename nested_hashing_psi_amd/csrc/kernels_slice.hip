// kernels_slice.hip -- query-sliced stage A for gfx950 (include/piehip.h "Query slices"; DESIGN.md section 6 "Query slices"): the inner products of
// BatchedFHEHIPPIE.cpp:96-116 for one handle's (inner hash function, limb) units, over one-limb arrays, and the placement of
// accumulator limbs that arrive from the handles that computed them into the arrays the product chain reads (.cpp:117-126).
// The term loop, the launch rules and the instruction blocks are those of kernels_stage_a.hip's tiled stage A (stage_a_common.h, madasm.h).
#include "kernels.hpp"
#include "madasm.h"
#include "stage_a_common.h"

namespace piehip {

static const u32 TPB = 256;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------
// Sliced stage A: acc[beta][q][u][c][n] = sum_j idx_q[u][j][c][n] * db[u][beta][j][n] + minus_q[u][c][n]   mod q_{(u_lo + u) % L}
//
// A thread owns one coefficient of one unit, Q queries and BPT bin layers; the term loop is stage_a_terms (stage_a_common.h) over
// one-limb arrays, for both arithmetics (MAD: every modulus in (2^59, 2^60)).  The handle sees ALL bin layers of its units, so the
// layer groups of a tile are many: the block -> tile map keeps them on one XCD (stage_a_tile with the unit in the limb's place).
// ---------------------------------------------------------------------------------------------
template <int BPT, int Q, int DEPTH, bool MAD>
__global__ void __launch_bounds__(TPB) stage_a_slice_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, u32 u_lo, u32 un, u32 b, u32 E,
                                                            StageAQueries qs, const u64 *__restrict__ db, u64 *__restrict__ acc, u32 nq,
                                                            u32 q0, u32 tiles)
{
    StageATile tl;
    if (!stage_a_tile((N + TPB - 1) / TPB, un, tiles, (b + BPT - 1) / BPT, tl)) return;
    const u32 nl = threadIdx.x, n0 = tl.bx * TPB, u = tl.l, beta0 = tl.grp * BPT;
    const u32 n = n0 + nl;
    if (n >= N) return;
    const u32 tmax = __builtin_amdgcn_readfirstlane(min((u32)BPT, b - beta0) - 1);   // (the last layer group may be ragged)
    const Mod m = dc->mod[(u_lo + u) % L];
    const size_t ioff = ((size_t)u * E) * 2 * N + n0;            // idx is [un][E][2][N]
    const u64 *pd = db + (((size_t)u * b + beta0) * E) * N + n0;  // db is [un][b][E][N]
    const size_t bin_stride = (size_t)E * N;
    StageAAcc<MAD> a[Q][BPT][2];
    stage_a_terms<BPT, Q, DEPTH, MAD>(qs, ioff, N, pd, bin_stride, tmax, nl, E, m, a);
#pragma unroll
    for (int q = 0; q < Q; q++) {
        u64 mi[2];
#pragma unroll
        for (int c = 0; c < 2; c++) mi[c] = qs.minus[q][((size_t)u * 2 + c) * N + n];   // minus is [un][2][N]
#pragma unroll
        for (int t = 0; t < BPT; t++) {
            if ((u32)t > tmax) continue;   // (uniform: a layer the ragged last group does not have)
            u64 *const po = acc + ((((size_t)(beta0 + t) * nq + q0 + q) * un + u) * 2) * N + n;   // acc is [b][nq][un][2][N]
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if constexpr (MAD)
                    po[(size_t)c * N] = addmod_nb(colacc_reduce<true>(a[q][t][c].v, m, 0 - m.q), mi[c], m.q);
                else
                    po[(size_t)c * N] = addmod(reduce128(a[q][t][c].v, m), mi[c], m.q);
            }
        }
    }
}

template <bool MAD>
static void launch_slice_groups(const DevConsts *dc, u32 N, u32 L, u32 u_lo, u32 un, u32 b, u32 E, const StageAQueries &qs, u32 nq,
                                const u64 *db, u64 *acc, hipStream_t st)
{
    const u32 nx = (N + TPB - 1) / TPB;
    stage_a_for_groups<MAD>(qs, nq, b, [&](auto Q_, auto B_, auto D_, const StageAQueries &sub, u32 q0) {
        hipLaunchKernelGGL((stage_a_slice_kernel<(int)B_(), (int)Q_(), (int)D_(), MAD>), stage_a_grid(nx, un, 1, (b + B_() - 1) / B_()), dim3(TPB), 0,
                           st, dc, N, L, u_lo, un, b, E, sub, db, acc, nq, q0, nx * un);
    });
}
void launch_stage_a_slice(const DevConsts *dc, u32 N, u32 L, u32 u_lo, u32 un, u32 b, u32 E, const StageAQueries &qs, u32 nq, const u64 *db,
                          u64 *acc, hipStream_t st, bool small_moduli)
{
    if (!un || !b || !nq) return;
    if (small_moduli) launch_slice_groups<true>(dc, N, L, u_lo, un, b, E, qs, nq, db, acc, st);
    else launch_slice_groups<false>(dc, N, L, u_lo, un, b, E, qs, nq, db, acc, st);
}

// ---------------------------------------------------------------------------------------------
// Placement.  One thread moves one pair of adjacent coefficients (16-byte lanes) of one polynomial (row, unit, component):
// src[bin_lo + beta][q][u][c][n] -> acc[beta][q][h][c][l][n], or -- units of inner hash function 0 when stage A of this batch hands
// operand X over in lane order (StageAXOut) -- into the Q limb l of slot c of the QP operand array, at the coefficient's lane-ordered
// home.  lane_home keeps an even / odd pair together, so the pair stays one 16-byte store.  Base and stride are uniform choices and
// the lane offset is blended with a mask (no per-lane selects: see addmod_nb).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) place_accumulators_kernel(u32 N, u32 L, u32 K, u32 u_lo, u32 un, u32 bin_lo, u32 nq,
                                                                 const u64 *__restrict__ src, u64 *__restrict__ acc, StageAXOut xo)
{
    const u32 n = 2 * (blockIdx.x * TPB + threadIdx.x);
    if (n >= N) return;
    const u32 u = blockIdx.y, row = blockIdx.z >> 1, c = blockIdx.z & 1;   // row = beta * nq + q of the chain side
    const u32 h = (u_lo + u) / L, l = (u_lo + u) % L;
    const bool xdir = h == 0 && xo.out != nullptr;
    const u32 noff = n + ((xdir ? ~0u : 0u) & (lane_home(n, xo.logns) - n));
    const u64 *ps = src + ((((size_t)bin_lo * nq + row) * un + u) * 2 + c) * N + n;
    u64 *const base = xdir ? xo.out + (((size_t)row * 4 + c) * xo.M + l) * N : acc + ((((size_t)row * K + h) * 2 + c) * L + l) * N;
    *reinterpret_cast<u64x2 *>(base + noff) = *reinterpret_cast<const u64x2 *>(ps);
}
void launch_place_accumulators(u32 N, u32 L, u32 K, u32 u_lo, u32 un, u32 bin_lo, u32 bn, u32 nq, const u64 *src, u64 *acc,
                               const StageAXOut *xop, hipStream_t st)
{
    if (!un || !bn || !nq) return;
    StageAXOut xo;
    if (xop) xo = *xop;
    // rows * 2 in z: bin layers x queries x components (z <= 65535: 4095 layers of eight queries)
    dim3 grid((N / 2 + TPB - 1) / TPB, un, bn * nq * 2);
    hipLaunchKernelGGL(place_accumulators_kernel, grid, dim3(TPB), 0, st, N, L, K, u_lo, un, bin_lo, nq, src, acc, xo);
}

// ---------------------------------------------------------------------------------------------
// Placement of every unit at once (piehip_rccl_exchange_accumulators): the chain side's rows of all K L units in one launch, each
// unit from the block that holds it -- the handle's own acc_slice or a block received from the rank that computed the unit.  The
// table of sources comes by value and is indexed by the unit, which is uniform over a workgroup (blockIdx.y): the look-up is scalar
// loads from the kernel arguments.  A block is src[rows from row0][un][2][N] with its units from u_lo; loads, stores and the lane
// order of operand X are those of place_accumulators_kernel.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) place_units_kernel(u32 N, u32 L, u32 K, PlaceSources src, u64 *__restrict__ acc, StageAXOut xo)
{
    const u32 n = 2 * (blockIdx.x * TPB + threadIdx.x);
    if (n >= N) return;
    const u32 u = blockIdx.y, row = blockIdx.z >> 1, c = blockIdx.z & 1;   // row = beta * nq + q of the chain side
    const PlaceSource s = src.of[u];
    const u32 h = u / L, l = u % L;
    const bool xdir = h == 0 && xo.out != nullptr;
    const u32 noff = n + ((xdir ? ~0u : 0u) & (lane_home(n, xo.logns) - n));
    const u64 *ps = s.base + ((((size_t)s.row0 + row) * s.un + (u - s.u_lo)) * 2 + c) * N + n;
    u64 *const base = xdir ? xo.out + (((size_t)row * 4 + c) * xo.M + l) * N : acc + ((((size_t)row * K + h) * 2 + c) * L + l) * N;
    *reinterpret_cast<u64x2 *>(base + noff) = *reinterpret_cast<const u64x2 *>(ps);
}
void launch_place_units(u32 N, u32 L, u32 K, u32 rows, const PlaceSources &src, u64 *acc, const StageAXOut *xop, hipStream_t st)
{
    if (!rows || K * L > PLACE_MAX_UNITS) return;
    StageAXOut xo;
    if (xop) xo = *xop;
    dim3 grid((N / 2 + TPB - 1) / TPB, K * L, rows * 2);   // (z <= 65535, as above)
    hipLaunchKernelGGL(place_units_kernel, grid, dim3(TPB), 0, st, N, L, K, src, acc, xo);
}

}  // namespace piehip
