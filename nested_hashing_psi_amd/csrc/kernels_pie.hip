// kernels_pie.hip -- the coefficient-wise kernels of BatchedFHEHIPPIE::run() for gfx950:
// fused ct x pt multiply-accumulate (stage A), HPS base conversions, tensor product, BV digit
// decomposition and key-switch accumulation, mask multiply, automorphism permutation, packed
// encoding.  All are streaming u64 modular arithmetic: one thread per coefficient, consecutive
// lanes on consecutive coefficients (coalesced 8-byte or 16-byte lanes), constants scalar-loaded
// from one DevConsts block.  Reference call sites: BatchedFHEHIPPIE.cpp:101-127.
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

// ---------------------------------------------------------------------------------------------
// Stage A (rows A3+A4): acc[beta][h][c][l][n] = sum_j idx[h][j][c][l][n] * db[h][beta][j][l][n] + minus[c][l][n]
//
// HBM-bound: every database plaintext limb is read exactly once per run() (b K E L W bytes, 196 MiB at C3).
// A thread owns two adjacent coefficients (16-byte lanes) of one (h, limb) and BPT bin layers: the two index
// ciphertext components are loaded once per j and reused for all BPT layers, so index traffic is
// (b / BPT) K E 2L W instead of b K E 2L W; the BPT database loads per j are independent streams in flight.
// 128-bit lazy accumulation: moduli may be up to 61 bits (HostParams::init), so products are < 2^122 and the
// accumulator is reduced every 32 terms (2^61 + 32 * 2^122 < 2^128); one more Barrett reduction at the end.
// ---------------------------------------------------------------------------------------------
template <int BPT>
__global__ void __launch_bounds__(TPB) stage_a_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, u32 K, u32 b, u32 E,
                                                      const u64 *__restrict__ idx, const u64 *__restrict__ minus,
                                                      const u64 *__restrict__ db, u64 *__restrict__ acc, u32 bstride, u32 h0,
                                                      u32 nq, u32 q)
{
    const u32 n = 2 * (blockIdx.x * TPB + threadIdx.x);
    const u32 l = blockIdx.y;
    const u32 groups = b / BPT;
    const u32 h = h0 + blockIdx.z / groups, beta0 = (blockIdx.z % groups) * BPT;
    if (n >= N) return;
    const Mod m = dc->mod[l];
    const size_t LN = (size_t)L * N;
    const u64 *pi = idx + ((size_t)h * E) * 2 * LN + (size_t)l * N + n;
    const u64 *pd = db + (((size_t)h * bstride + beta0) * E) * LN + (size_t)l * N + n;  // db is [K][bstride][E][L][N]
    const size_t bin_stride = (size_t)E * LN;
    U128 a[BPT][2][2];
#pragma unroll
    for (int t = 0; t < BPT; t++)
#pragma unroll
        for (int c = 0; c < 2; c++) a[t][c][0] = a[t][c][1] = U128{0, 0};
    for (u32 j = 0; j < E; j++) {
        const u64x2 i0 = *reinterpret_cast<const u64x2 *>(pi + (size_t)j * 2 * LN);
        const u64x2 i1 = *reinterpret_cast<const u64x2 *>(pi + (size_t)j * 2 * LN + LN);
        u64x2 d[BPT];
#pragma unroll
        for (int t = 0; t < BPT; t++) {  // streamed once per run(): non-temporal (see stage_a_mad_kernel)
            typedef u64 u64v2 __attribute__((ext_vector_type(2)));
            const u64v2 v = __builtin_nontemporal_load(reinterpret_cast<const u64v2 *>(pd + (size_t)t * bin_stride + (size_t)j * LN));
            d[t].x = v.x, d[t].y = v.y;
        }
#pragma unroll
        for (int t = 0; t < BPT; t++) {
            mac128(a[t][0][0], i0.x, d[t].x);
            mac128(a[t][0][1], i0.y, d[t].y);
            mac128(a[t][1][0], i1.x, d[t].x);
            mac128(a[t][1][1], i1.y, d[t].y);
        }
        if ((j & 31) == 31) {
#pragma unroll
            for (int t = 0; t < BPT; t++)
#pragma unroll
                for (int c = 0; c < 2; c++)
#pragma unroll
                    for (int e = 0; e < 2; e++) a[t][c][e] = U128{reduce128(a[t][c][e], m), 0};
        }
    }
    const u64x2 m0 = *reinterpret_cast<const u64x2 *>(minus + (size_t)l * N + n);
    const u64x2 m1 = *reinterpret_cast<const u64x2 *>(minus + LN + (size_t)l * N + n);
#pragma unroll
    for (int t = 0; t < BPT; t++) {
        u64 *po = acc + ((((size_t)(beta0 + t) * nq + q) * K + h) * 2) * LN + (size_t)l * N + n;
        u64x2 r0, r1;
        r0.x = addmod(reduce128(a[t][0][0], m), m0.x, m.q);
        r0.y = addmod(reduce128(a[t][0][1], m), m0.y, m.q);
        r1.x = addmod(reduce128(a[t][1][0], m), m1.x, m.q);
        r1.y = addmod(reduce128(a[t][1][1], m), m1.y, m.q);
        *reinterpret_cast<u64x2 *>(po) = r0;
        *reinterpret_cast<u64x2 *>(po + LN) = r1;
    }
}

// Same work with carry-free column accumulators on v_mad_u64_u32 (madasm.h): the 128-bit form above is bound by
// its 64x64->128 multiplies (46 SIMD cycles each, 3.9 TB/s at C3), this one by HBM.  Needs every modulus
// < 2^60 (a carry sweep every 8 terms keeps the low columns from overflowing, a reduction every 15 the top one).
// One coefficient per thread and SA_DEPTH terms in flight behind the one being accumulated: a term is 2 + BPT loads of
// 8 bytes per lane against microseconds of HBM latency and ~80 instructions of arithmetic.  tools/microbench_stage_a.hip
// runs this kernel over a rotation of databases (every launch from HBM): 49 us for the 196 MiB of the headline workload
// with seven layers per thread (168 registers, three waves per SIMD), the same with 16-byte lanes and one term ahead, 63 us
// when it is forced to four waves per SIMD (spills) -- and 35 us for a plain read of the same bytes.
static const int SA_DEPTH = 4;
template <int BPT>
__global__ void __launch_bounds__(TPB) stage_a_mad_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, u32 K, u32 b, u32 E,
                                                          const u64 *__restrict__ idx, const u64 *__restrict__ minus,
                                                          const u64 *__restrict__ db, u64 *__restrict__ acc, u32 bstride, u32 h0,
                                                          u32 nq, u32 q, StageAXOut xo)
{
    const u32 nl = threadIdx.x;  // lane part of the coefficient index: every stream is a uniform base plus this
    const u32 n = blockIdx.x * TPB + nl;
    const u32 l = blockIdx.y;
    const u32 groups = b / BPT;
    const u32 h = h0 + blockIdx.z / groups, beta0 = (blockIdx.z % groups) * BPT;
    if (n >= N) return;
    const Mod m = dc->mod[l];
    const size_t LN = (size_t)L * N;
    // uniform stream bases (scalar registers where the compiler can; the loads take base + lane offset)
    const u64 *pi = idx + ((size_t)h * E) * 2 * LN + (size_t)l * N + blockIdx.x * TPB;
    const u64 *pd = db + (((size_t)h * bstride + beta0) * E) * LN + (size_t)l * N + blockIdx.x * TPB;  // db is [K][bstride][E][L][N]
    const size_t bin_stride = (size_t)E * LN;
    ColAcc a[BPT][2];
#pragma unroll
    for (int t = 0; t < BPT; t++) a[t][0] = a[t][1] = ColAcc{0, 0, 0};
    auto load_term = [&](u32 j, u64 (&vi)[2], u64 (&vd)[BPT]) {
        const u64 *pij = pi + (size_t)j * 2 * LN, *pdj = pd + (size_t)j * LN;
        vi[0] = pij[nl];
        vi[1] = (pij + LN)[nl];
#pragma unroll
        // the database is read once per run() and is as large as the infinity cache: non-temporal loads keep it from evicting
        // the (dirty) intermediate arrays the neighbouring kernels hand to each other there -- 59 -> 50 us for this kernel
        // inside a run(), where it otherwise also paid for those write-backs (alone on the GPU it took 49 us either way)
        for (int t = 0; t < BPT; t++) vd[t] = __builtin_nontemporal_load(pdj + (size_t)t * bin_stride + nl);
    };
    // a ring of SA_DEPTH term buffers; the term loop is unrolled SA_DEPTH times so that the ring needs no register moves
    u64 qiv[SA_DEPTH][2], qdv[SA_DEPTH][BPT];
#pragma unroll
    for (int d = 0; d < SA_DEPTH; d++)
        if ((u32)d < E) load_term(d, qiv[d], qdv[d]);
    auto term = [&](u32 j, u64 (&vi)[2], u64 (&vd)[BPT]) {
        const Split30 i0 = split30(vi[0]), i1 = split30(vi[1]);
#pragma unroll
        for (int t = 0; t < BPT; t++) colacc_mac2(a[t][0], a[t][1], i0, i1, vd[t]);
        if (j + SA_DEPTH < E) load_term(j + SA_DEPTH, vi, vd);  // refill this ring slot (the other slots are in flight)
        if ((j % COLACC_MAX_TERMS) == COLACC_MAX_TERMS - 1 && j + 1 < E) {  // more terms follow: make room in the low columns
#pragma unroll
            for (int t = 0; t < BPT; t++) colacc_carry(a[t][0]), colacc_carry(a[t][1]);
        }
        if ((j % COLACC_MAX_TOTAL) == COLACC_MAX_TOTAL - 1 && j + 1 < E) {  // the top column is full: reduce and start over
#pragma unroll
            for (int t = 0; t < BPT; t++)
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const u64 r = reduce124(colacc_value(a[t][c]), m);  // (the epilogue's instruction block here would cost this kernel, at seven
                                                                       // layers per thread, its third wave per SIMD: 176 registers)
                    a[t][c] = ColAcc{r & 0x3FFFFFFFull, r >> 30, 0};
                }
        }
    };
    for (u32 j = 0; j < E; j += SA_DEPTH) {
#pragma unroll
        for (int d = 0; d < SA_DEPTH; d++)
            if (j + d < E) term(j + d, qiv[d], qdv[d]);
    }
    const bool xdir = h == 0 && xo.out != nullptr;
    const u32 noff = n + ((xdir ? ~0u : 0u) & (lane_home(n, xo.logns) - n));
#pragma unroll
    for (int t = 0; t < BPT; t++) {
        const size_t row = (size_t)(beta0 + t) * nq + q;
        // operand X of the first product goes straight to the QP operand array, lane-ordered (StageAXOut).  Uniform choices of
        // base and stride, and the lane offset blended with a mask: no per-lane selects (v_cndmask on VCC: see addmod_nb)
        u64 *const base = xdir ? xo.out + ((row * 4) * xo.M + l) * N : acc + ((row * K + h) * 2) * LN + (size_t)l * N;
        const size_t cstride = xdir ? (size_t)xo.M * N : LN;
        u64 *const po = base + noff;
#pragma unroll
        for (int c = 0; c < 2; c++)
            po[(size_t)c * cstride] = addmod_nb(colacc_reduce<true>(a[t][c], m, 0 - m.q), minus[(size_t)c * LN + (size_t)l * N + n], m.q);
    }
}

// A batch of Q >= 2 queries against one database (piehip_set_query_batch): the thread holds the accumulators of Q queries x BPT bin
// layers, so a database word is loaded once for the whole batch -- the database is 196 of the 253 MiB stage A moves for one
// query at the headline shape -- and an index-ciphertext word once per BPT layers as before.  A term is 2 Q + BPT loads for
// 2 Q BPT multiply-accumulates (one query, seven layers: 9 for 14; two queries, four layers: 8 for 16).  The term loop is
// stage_a_terms (stage_a_common.h) for both arithmetics -- MAD: the column accumulators of stage_a_mad_kernel, otherwise the 128-bit
// ones of stage_a_kernel -- with DEPTH terms in flight and a last layer group that may be ragged.
// acc rows: [bin layer][query][K][2][L][N] (the product chain treats (layer, query) as one batch index).
// 27-31 us per query at the headline shape against 46-49 for one query per launch; what bounds it then is issue time plus
// memory latency at three waves per SIMD, not HBM bytes -- profiles/r03/stage_a_batch_microbench.txt, with the cuts that were
// tried on top (index words shared through L1 or LDS) and dropped.  One query stays on the two kernels above: through this one
// (Q = 1, same tiling) a C3 step was 0.7-2 % slower on the column accumulators and stage A 9 us of 50 slower on the 128-bit ones
// (profiles/stage_a_one_kernel).
template <int BPT, int Q, int DEPTH, bool MAD>
__global__ void __launch_bounds__(TPB) stage_a_tiled_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, u32 K, u32 b, u32 E,
                                                            StageAQueries qs, const u64 *__restrict__ db, u64 *__restrict__ acc,
                                                            u32 bstride, u32 h0, u32 nq, u32 q0, u32 tiles, StageAXOut xo)
{
    StageATile tl;
    if (!stage_a_tile((N + TPB - 1) / TPB, L, tiles, (b + BPT - 1) / BPT, tl)) return;
    const u32 nl = threadIdx.x, n0 = tl.bx * TPB, l = tl.l, h = h0 + tl.hz, beta0 = tl.grp * BPT;
    const u32 n = n0 + nl;
    if (n >= N) return;
    const u32 tmax = __builtin_amdgcn_readfirstlane(min((u32)BPT, b - beta0) - 1);   // (the last layer group may be ragged)
    const Mod m = dc->mod[l];
    const size_t LN = (size_t)L * N;
    const size_t ioff = ((size_t)h * E) * 2 * LN + (size_t)l * N + n0;
    const u64 *pd = db + (((size_t)h * bstride + beta0) * E) * LN + (size_t)l * N + n0;   // db is [K][bstride][E][L][N]
    const size_t bin_stride = (size_t)E * LN;
    StageAAcc<MAD> a[Q][BPT][2];
    stage_a_terms<BPT, Q, DEPTH, MAD>(qs, ioff, LN, pd, bin_stride, tmax, nl, E, m, a);
    const bool xdir = MAD && h == 0 && xo.out != nullptr;   // (the 128-bit arithmetic writes acc only)
    const u32 noff = n + ((xdir ? ~0u : 0u) & (lane_home(n, xo.logns) - n));
#pragma unroll
    for (int q = 0; q < Q; q++) {
        u64 mi[2];
#pragma unroll
        for (int c = 0; c < 2; c++) mi[c] = qs.minus[q][(size_t)c * LN + (size_t)l * N + n];
#pragma unroll
        for (int t = 0; t < BPT; t++) {
            if ((u32)t > tmax) continue;   // (uniform: a layer the ragged last group does not have)
            const size_t row = (size_t)(beta0 + t) * nq + q0 + q;
            // operand X of the first product goes straight to the QP operand array, lane-ordered (StageAXOut).  Uniform choices
            // of base and stride, and the lane offset blended with a mask: no per-lane selects (v_cndmask on VCC: see addmod_nb)
            // (This epilogue is written out again in the resident kernel and in stage_a_slice_kernel.  As device functions, the
            // destination compiles to other code and the reduction plus sum to a sum with its operands the other way round:
            // profiles/stage_a_one_kernel/README.txt.)
            u64 *const base = xdir ? xo.out + ((row * 4) * xo.M + l) * N : acc + ((row * K + h) * 2) * LN + (size_t)l * N;
            const size_t cstride = xdir ? (size_t)xo.M * N : LN;
            u64 *const po = base + noff;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if constexpr (MAD)
                    po[(size_t)c * cstride] = addmod_nb(colacc_reduce<true>(a[q][t][c].v, m, 0 - m.q), mi[c], m.q);
                else
                    po[(size_t)c * cstride] = addmod(reduce128(a[q][t][c].v, m), mi[c], m.q);
            }
        }
    }
}

// The other loop order for a batch of Q queries: layers outside, index words resident.  A thread -- one coefficient of one limb
// of one inner hash function, as above -- loads the 2 Q E index words of its coefficient ONCE, keeps them in registers as 30-bit
// halves, and lets the database words of its block's layers stream past them, one layer's 2 Q accumulators at a time.  Index and
// database words are then each read exactly once per launch (the tiled kernel re-reads the index words from the L2 once per
// group of BPT layers), at the price of 4 Q E registers: Q = 3, E = 14 is what a thread of 256 registers holds, two waves per SIMD.
// The database words of a (h, l, coefficient block) over consecutive layers are ONE strided stream (word layer E + j at
// pd + (layer E + j) L N): a ring of D words runs over it across the layer boundaries, so the first words of layer beta + 1 are
// in flight under the epilogue of layer beta.  D divides E: the ring slot of a term is then a compile-time constant.  Every refill
// is unconditional; past the last word of the block's layers the stream repeats that word (an address inside the array, an L2 hit
// nobody consumes).  E <= COLACC_MAX_TOTAL - 1 terms: one carry sweep after term COLACC_MAX_TERMS, no mid-sum reduction.
// The block-to-tile map is stage_a_tile with `groups` = partitions of the layer range (lpp layers each, the last one shorter).
template <int Q, int E, int D>
__global__ void __launch_bounds__(TPB) stage_a_resident_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, u32 K, u32 b, u32 lpp,
                                                               StageAQueries qs, const u64 *__restrict__ db, u64 *__restrict__ acc,
                                                               u32 bstride, u32 h0, u32 nq, u32 q0, u32 tiles, StageAXOut xo)
{
    static_assert(E % D == 0 && E >= 1 && (u32)E < COLACC_MAX_TOTAL && (u32)E <= 2 * COLACC_MAX_TERMS, "ring slots and sweep periods");
    StageATile tl;
    if (!stage_a_tile((N + TPB - 1) / TPB, L, tiles, (b + lpp - 1) / lpp, tl)) return;
    const u32 nl = threadIdx.x, n0 = tl.bx * TPB, l = tl.l, h = h0 + tl.hz, beta0 = tl.grp * lpp;
    const u32 n = n0 + nl;
    if (n >= N) return;
    const u32 nlay = __builtin_amdgcn_readfirstlane(min(lpp, b - beta0));
    const Mod m = dc->mod[l];
    const size_t LN = (size_t)L * N;
    const size_t ioff = ((size_t)h * E) * 2 * LN + (size_t)l * N + n0;
    const u64 *pw = db + (((size_t)h * bstride + beta0) * E) * LN + (size_t)l * N + n0;   // the next word the ring fetches
    u32 left = nlay * E - 1;   // words behind the one pw points to; at 0 the stream repeats its last word
    // the ring first: its words are the oldest loads in flight when the first term asks for one
    u64 r[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        r[d] = __builtin_nontemporal_load(pw + nl);
        pw += left ? LN : 0, left -= left ? 1 : 0;
    }
    Split30 ix[Q][E][2];
    u64 mi[Q][2];
#pragma unroll
    for (int q = 0; q < Q; q++) {
#pragma unroll
        for (int j = 0; j < E; j++)
#pragma unroll
            for (int c = 0; c < 2; c++) ix[q][j][c] = split30((qs.idx[q] + ioff + (size_t)(2 * j + c) * LN)[nl]);
#pragma unroll
        for (int c = 0; c < 2; c++) mi[q][c] = qs.minus[q][(size_t)c * LN + (size_t)l * N + n];
    }
    const bool xdir = h == 0 && xo.out != nullptr;
    const u32 noff = n + ((xdir ? ~0u : 0u) & (lane_home(n, xo.logns) - n));
    const size_t cstride = xdir ? (size_t)xo.M * N : LN;
    for (u32 t = 0; t < nlay; t++) {
        ColAcc a[Q][2];
#pragma unroll
        for (int j = 0; j < E; j++) {
            const u64 d = r[j % D];
            const u32 dl = (u32)d & 0x3FFFFFFFu, dh = (u32)(d >> 30);
            r[j % D] = __builtin_nontemporal_load(pw + nl);   // refill the slot: the other D - 1 words stay in flight
            pw += left ? LN : 0, left -= left ? 1 : 0;
            PIE_STAGE_A_FENCE();
#pragma unroll
            for (int q = 0; q < Q; q++) {
                if (j == 0) colacc_mac2_cut<true>(a[q][0], a[q][1], ix[q][j][0], ix[q][j][1], dl, dh);
                else colacc_mac2_cut<false>(a[q][0], a[q][1], ix[q][j][0], ix[q][j][1], dl, dh);
            }
            if (j == (int)COLACC_MAX_TERMS - 1 && j + 1 < E) {   // more terms follow: make room in the low columns
#pragma unroll
                for (int q = 0; q < Q; q++) colacc_carry(a[q][0]), colacc_carry(a[q][1]);
            }
            PIE_STAGE_A_FENCE();
        }
        // the epilogue of the tiled kernel.  Its stores are younger than the D ring words in flight: the next term waits for its
        // own word with the stores still outstanding
#pragma unroll
        for (int q = 0; q < Q; q++) {
            // (row base from scratch per layer and query, all scalar: carried across the layers as a pointer it went into vector
            // registers -- 258 with the index words, one wave per SIMD)
            const size_t row = (size_t)(beta0 + t) * nq + q0 + q;
            u64 *const base = xdir ? xo.out + ((row * 4) * xo.M + l) * N : acc + ((row * K + h) * 2) * LN + (size_t)l * N;
            u64 *const po = base + noff;
#pragma unroll
            for (int c = 0; c < 2; c++) po[(size_t)c * cstride] = addmod_nb(colacc_reduce<true>(a[q][c], m, 0 - m.q), mi[q][c], m.q);
        }
        PIE_STAGE_A_FENCE();
    }
}

// One query (row q of nq) through stage_a_mad_kernel or stage_a_kernel.  Bin layers per thread: a thread re-reads the two
// index-ciphertext limbs once per group of layers, so groups should be as large as the accumulators allow (cap).  A divisor of b in
// [4, cap] gives one uniform launch; otherwise (b = 17, 23, ...: one queue's share of an odd split) groups of `cap` layers plus one
// launch for the remainder -- never one layer per thread, which read the index matrix b times.
template <bool MAD>
static void launch_stage_a_one(const DevConsts *dc, u32 N, u32 L, u32 K, u32 b, u32 E, const u64 *idx, const u64 *minus, const u64 *db,
                               u64 *acc, hipStream_t st, u32 bstride, u32 h0, u32 hn, u32 nq, u32 q, StageAXOut xo)
{
    constexpr u32 cap = MAD ? 7 : 8;
    auto uniform = [&](u32 first, u32 nb, u32 bpt) {   // layers [first, first + nb), nb a multiple of bpt
        const size_t LN = (size_t)L * N;
        const u64 *dbf = db + (size_t)first * E * LN;
        u64 *accf = acc + (size_t)first * nq * K * 2 * LN;
        const dim3 grid((N / (MAD ? 1 : 2) + TPB - 1) / TPB, L, hn * (nb / bpt));
        with_u32<1, cap>(bpt, [&](auto B_) {
            if constexpr (MAD) {
                StageAXOut xf = xo;
                if (xf.out) xf.out += (size_t)first * nq * 4 * xf.M * N;
                hipLaunchKernelGGL(stage_a_mad_kernel<(int)B_()>, grid, dim3(TPB), 0, st, dc, N, L, K, nb, E, idx, minus, dbf, accf, bstride, h0, nq, q, xf);
            } else {
                hipLaunchKernelGGL(stage_a_kernel<(int)B_()>, grid, dim3(TPB), 0, st, dc, N, L, K, nb, E, idx, minus, dbf, accf, bstride, h0, nq, q);
            }
        });
    };
    u32 bpt = b <= cap ? b : 0;
    for (u32 c = cap; c >= 4 && !bpt; c--)
        if (b % c == 0) bpt = c;
    if (bpt) return uniform(0, b, bpt);
    uniform(0, b / cap * cap, cap);
    uniform(b / cap * cap, b % cap, b % cap);
}

// Stage A of nq >= 1 queries on one handle: acc[b][nq][K][2][L][N].  Groups of two to four queries, ONE launch per group whatever
// the layer count (a layer count that is no multiple of the per-thread layer count leaves a ragged last group), each reading the
// database once.  Query groups, layers per thread and terms in flight by the rules of stage_a_common.h (stage_a_for_groups); a group
// of three on a ring that fills the chip keeps its index words resident instead (stage_a_resident_lpp said so: one partition of
// `lpp` layers per block), and a single query goes to the one-query kernels.
template <bool MAD>
static void launch_stage_a_groups(const DevConsts *dc, u32 N, u32 L, u32 K, u32 b, u32 E, const StageAQueries &qs, u32 nq, const u64 *db,
                                  u64 *acc, hipStream_t st, u32 bstride, u32 h0, u32 hn, StageAXOut xo)
{
    const u32 nx = (N + TPB - 1) / TPB, tiles = nx * L * hn;
    stage_a_for_groups<MAD>(qs, nq, b, [&](auto Q_, auto B_, auto D_, const StageAQueries &sub, u32 q0) {
        if constexpr (Q_() == 1) {   // (BPT and DEPTH are the tiled kernel's)
            launch_stage_a_one<MAD>(dc, N, L, K, b, E, sub.idx[0], sub.minus[0], db, acc, st, bstride, h0, hn, nq, q0, xo);
        } else {
            if constexpr (MAD && Q_() == 3) {
                const u32 lpp = stage_a_resident_lpp(3, E, b, (u64)N * L * hn);
                auto resident = [&](auto E_) {
                    hipLaunchKernelGGL((stage_a_resident_kernel<3, E_(), stage_a_resident_ring(E_())>), stage_a_grid(nx, L, hn, (b + lpp - 1) / lpp),
                                       dim3(TPB), 0, st, dc, N, L, K, b, lpp, sub, db, acc, bstride, h0, nq, q0, tiles, xo);
                };
                if (lpp && E == 14) return resident(std::integral_constant<int, 14>{});
                if (lpp && E == 12) return resident(std::integral_constant<int, 12>{});
            }
            hipLaunchKernelGGL((stage_a_tiled_kernel<(int)B_(), (int)Q_(), (int)D_(), MAD>), stage_a_grid(nx, L, hn, (b + B_() - 1) / B_()), dim3(TPB),
                               0, st, dc, N, L, K, b, E, sub, db, acc, bstride, h0, nq, q0, tiles, xo);
        }
    });
}
void launch_stage_a_batch(const DevConsts *dc, u32 N, u32 L, u32 K, u32 b, u32 E, const StageAQueries &qs, u32 nq, const u64 *db,
                          u64 *acc, hipStream_t st, bool small_moduli, u32 bstride, u32 h0, u32 hn, const StageAXOut *xop)
{
    StageAXOut xo;
    if (xop && small_moduli) xo = *xop;   // (the 128-bit arithmetic keeps writing acc: callers check small_moduli before they rely on xo)
    if (!bstride) bstride = b;
    if (!hn) hn = K - h0;
    if (small_moduli) launch_stage_a_groups<true>(dc, N, L, K, b, E, qs, nq, db, acc, st, bstride, h0, hn, xo);
    else launch_stage_a_groups<false>(dc, N, L, K, b, E, qs, nq, db, acc, st, bstride, h0, hn, xo);
}

// ---------------------------------------------------------------------------------------------
// Base conversions (row A6).  One thread per coefficient reads its L (or 2L+1) residues at limb
// stride N and writes every output limb.  Rounding terms use the 60-bit fixed-point rule of
// modarith.h (identical to oracle/pie_oracle.c: po_expand_q_to_qp, po_scale_pq_expand, po_scale_round_tp).
// ---------------------------------------------------------------------------------------------
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

// The limb drop of limb_drop_kernel (below) on the NP coefficient columns a thread holds, with the constants of the block that has all
// L limbs, read per dropped limb through the laundered pointer (the convention above).  S63 (every modulus below 2^60): the shoup63
// instruction block; otherwise limb_drop_kernel's own product.  Only c[..][0 .. KEEP) are meaningful afterwards.
template <u32 L, u32 KEEP, int NP, bool S63>
__device__ __forceinline__ void drop_limbs(const DevConsts *dc, u64 (&c)[NP][L])
{
#pragma unroll
    for (u32 l = L - 1; l >= KEEP; l--) {
        PIE_ITER_FENCE();
        const DcC k = dc_iter(dc);
        const u64 ql = k->mod[l].q;
        u64 v[NP], s[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            v[p] = c[p][l];
            s[p] = (u64)((int64_t)((ql >> 1) - v[p]) >> 63);  // all ones when the centred residue is negative
        }
#pragma unroll
        for (u32 i = 0; i < l; i++) {
            const u64 off = k->drop_off[l][i], w = k->drop_inv[l][i], wsh = k->drop_inv_sh[l][i], qi = k->mod[i].q;
            const u64 nq = S63 ? neg_u(qi) : k->drop_negq[i];
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const u64 x = c[p][i] - v[p] + off + (s[p] & (ql - off));
                c[p][i] = S63 ? shoup63(x, w, wsh, nq) : mul_shoup_u(x, w, wsh, qi, nq);
            }
        }
    }
}

// The RNS width L is a template parameter: with run-time trip counts hipcc indexes the per-coefficient residue
// arrays dynamically and spills them to scratch.  NP coefficients (1, or the 2 of a folded pair) go through every
// iteration together and share its constants.
// x[L] (mod Q) -> out[M]: Q limbs copied, P limbs = centred CRT lift
// YIN: x[] already holds the CRT digits y_i = [x_i (Q/q_i)^-1]_{q_i} (folded load with the merged constants); the Q
// limbs of the output are then not produced
// K (here and in every template below): the arithmetic kind (ArithKind, modarith.h).  MAD: one of the two column-accumulator kinds
template <u32 L, ArithKind K, bool YIN, int NP, bool LZ = false>
__device__ __forceinline__ void expand_core(const DevConsts *dc, const u64 (&x)[NP][L], u64 (&out)[NP][2 * L + 1])
{
    constexpr bool MAD = colacc(K);
    constexpr u32 Lp = L + 1;
    u64 y[NP][L];
    u64 fsum[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) fsum[p] = 0;
#pragma unroll
    for (u32 i = 0; i < L; i++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod mi = ld_mod(c, i);
        const u64 w = c->qhat_inv[i], wsh = c->qhat_inv_sh[i], nq = neg_u(mi.q);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            out[p][i] = x[p][i];
            y[p][i] = YIN ? x[p][i] : mshoup<MAD>(x[p][i], w, wsh, mi.q, nq);
            fsum[p] += mfixfrac<MAD>(y[p][i], mi);
        }
    }
#pragma unroll
    for (u32 j = 0; j < Lp; j++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod pj = ld_mod(c, L + j);
        u64 hat[L];
#pragma unroll
        for (u32 i = 0; i < L; i++) hat[i] = c->qhat_modp[i][j];
        const u64 prodmod = c->Q_modp[j], nq = neg_u(pj.q), n2q = neg_u(2 * pj.q);
#pragma unroll
        for (int p = 0; p < NP; p++) out[p][L + j] = crt_out<L, K, LZ>(y[p], hat, (fsum[p] + FIX_HALF) >> 60, prodmod, pj, nq, n2q);
    }
}

// x[L] (mod Q) -> out[M]: P limbs = round(P x / Q), Q limbs = centred CRT lift of that
template <u32 L, ArithKind K, bool YIN, int NP, bool LZ = false>
__device__ __forceinline__ void scale_pq_core(const DevConsts *dc, const u64 (&x)[NP][L], u64 (&out)[NP][2 * L + 1])
{
    constexpr bool MAD = colacc(K), FD = K == ArithKind::fold;
    constexpr u32 Lp = L + 1;
    u64 y[NP][L];
    u64 fsum[NP];
    U128 itot[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) fsum[p] = 0, itot[p] = U128{0, 0};
#pragma unroll
    for (u32 i = 0; i < L; i++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod mi = ld_mod(c, i);
        const u64 w = c->qhat_inv[i], wsh = c->qhat_inv_sh[i], pw = c->P_modq[i], pwsh = c->P_modq_sh[i], nq = neg_u(mi.q);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            y[p][i] = YIN ? x[p][i] : mshoup<MAD>(x[p][i], w, wsh, mi.q, nq);
            // y_i P / q_i = y_i floor(P/q_i) + floor(y_i w_i / q_i) + (y_i w_i mod q_i) / q_i
            u64 fl, z;
            mdivmod<MAD>(y[p][i], pw, pwsh, mi.q, nq, fl, z);
            add128(itot[p], U128{fl, 0});
            fsum[p] += mfixfrac<MAD>(z, mi);
        }
    }
    u64 yp[NP][Lp];
    u64 fs2[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        add128(itot[p], U128{(fsum[p] + FIX_HALF) >> 60, 0});
        fs2[p] = 0;
    }
#pragma unroll
    for (u32 j = 0; j < Lp; j++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod pj = ld_mod(c, L + j);
        u64 col[L];
#pragma unroll
        for (u32 i = 0; i < L; i++) col[i] = c->PI_modp[i][j];
        const u64 w = c->phat_inv[j], wsh = c->phat_inv_sh[j], nq = neg_u(pj.q);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            u64 r;
            if (MAD) {   // L <= 7 products + the integer parts (< (L + 1) 2^60, in column 0): below 2^123
                ColAcc a = {itot[p].lo, 0, 0};
#pragma unroll
                for (u32 i = 0; i < L; i++) colacc_mac(a, split30(y[p][i]), split30(col[i]));
                r = LZ ? colacc_red_lazy<FD>(a, pj, nq) : colacc_red<FD, false>(a, pj, nq);  // (LZ: feeds a Shoup product and fold_store)
            } else {
                U128 acc = dot128<L, MAD>(y[p], col);
                add128(acc, itot[p]);
                r = reduce128(acc, pj);
            }
            out[p][L + j] = r;
            yp[p][j] = mshoup<MAD>(r, w, wsh, pj.q, nq);
            fs2[p] += mfixfrac<MAD>(yp[p][j], pj);
        }
    }
#pragma unroll
    for (u32 i = 0; i < L; i++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod mi = ld_mod(c, i);
        u64 hat[Lp];
#pragma unroll
        for (u32 j = 0; j < Lp; j++) hat[j] = c->phat_modq[j][i];
        const u64 prodmod = c->P_modq[i], nq = neg_u(mi.q), n2q = neg_u(2 * mi.q);
#pragma unroll
        for (int p = 0; p < NP; p++) out[p][i] = crt_out<Lp, K, LZ>(yp[p], hat, (fs2[p] + FIX_HALF) >> 60, prodmod, mi, nq, n2q);
    }
}

// How the L input residues of a conversion reach registers
enum class ExpandIn {
    pending,  // as the context's inverse transform left them.  FOLD: outer stage pending, residues in [0, 4q) (fold_load, or the
              // merged-constant load where YIN)
    plain,    // canonical, nothing pending (what chain_drop_kernel and an unfolded inverse transform leave): both halves are read as
              // they are and FOLD is the store side alone -- the forward transform that follows is a folded one
    drop,     // chain limbs, fused (folded rings, every modulus in (2^59, 2^60)): the polynomial has LSRC > L limbs as the SOURCE level's
              // folded inverse transform left them.  fold_load and drop_limbs<LSRC, L> with that level's constants (dcs), then the
              // conversion with this level's (dc): no pass over the operand, no buffer
};
// One conversion of polynomial (o, c) = (by / 2, by % 2): read at in + o so + c si, written to out[o][out_polys][M][N] at slot out_slot + c
// SKIPQ (centred lift only): leave the Q limbs of the output alone, they already hold the operand's EVALUATION form
// K: at ArithKind::fold (NttPlan::fold_moduli) the column sums are reduced by the folded block (stage_a_common.h)
template <bool SCALE, bool FOLD, u32 L, ArithKind K, bool SKIPQ, ExpandIn IN = ExpandIn::pending, u32 LSRC = L>
__device__ __forceinline__ void expand_body(const DevConsts *__restrict__ dcs, const DevConsts *__restrict__ dc, u32 N,
                                            const u64 *__restrict__ in, size_t so, size_t si, u64 *__restrict__ out, u32 out_polys,
                                            u32 out_slot, u32 by)
{
    static_assert(IN == ExpandIn::pending || !SKIPQ, "Q limbs in place: an operand on this level's limbs, as its inverse transform left it");
    constexpr bool MAD = colacc(K);
    static_assert(IN == ExpandIn::drop ? (LSRC > L && FOLD && MAD) : LSRC == L, "the drop: folded rings at a column-accumulator kind");
    // the residues x_i themselves are not needed: the folded load multiplies by N^-1 (Q/q_i)^-1 in one go
    constexpr bool YIN = IN == ExpandIn::pending && FOLD && (SCALE || SKIPQ);
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    const u32 H = N / 2;
    if (n >= (FOLD ? H : N)) return;
    const u32 o = by >> 1, c = by & 1;
    constexpr u32 M = 2 * L + 1;
    const u64 *pin = in + (size_t)o * so + (size_t)c * si + n;
    u64 *pout = out + ((size_t)(o * out_polys + out_slot + c) * M) * N + n;
    constexpr int NP = FOLD ? 2 : 1;
    u64 x[NP][L], y[NP][M];
    if constexpr (IN == ExpandIn::drop) {
        u64 full[NP][LSRC];
#pragma unroll
        for (u32 i = 0; i < LSRC; i++) fold_load(dcs, i, pin[(size_t)i * N], pin[(size_t)i * N + H], full[0][i], full[NP - 1][i]);
        drop_limbs<LSRC, L, NP, true>(dcs, full);
#pragma unroll
        for (u32 i = 0; i < L; i++) x[0][i] = full[0][i], x[NP - 1][i] = full[NP - 1][i];
    } else {
#pragma unroll
        for (u32 i = 0; i < L; i++) {
            if (YIN) {
                PIE_ITER_FENCE();
                const DcC c = dc_iter(dc);
                const u64 q = c->mod[i].q, nq = neg_u(q), u = pin[(size_t)i * N], v = pin[(size_t)i * N + H];
                x[0][i] = shoup63(u + v, c->fold_iaq[i], c->fold_iaq_sh[i], nq);            // u, v in [0, 4q)
                x[NP - 1][i] = shoup63(u + (4 * q - v), c->fold_ibq[i], c->fold_ibq_sh[i], nq);
            } else if (FOLD && IN == ExpandIn::pending) {
                fold_load(dc, i, pin[(size_t)i * N], pin[(size_t)i * N + H], x[0][i], x[NP - 1][i]);
            } else {
                x[0][i] = pin[(size_t)i * N];
                if (FOLD) x[NP - 1][i] = pin[(size_t)i * N + H];
            }
        }
    }
    // folded output: every result passes through fold_store into a transform that takes [0, 8q) -- [0, 4q) will do (LZ)
    constexpr bool LZ = FOLD && MAD;
    if (SCALE)
        scale_pq_core<L, K, YIN, NP, LZ>(dc, x, y);
    else
        expand_core<L, K, YIN, NP, LZ>(dc, x, y);
#pragma unroll
    for (u32 a = 0; a < M; a++) {
        if (!SCALE && a < L && SKIPQ) continue;  // (NttExtra)
        PIE_ITER_FENCE();
        if (FOLD) {
            u64 y0, y1;
            fold_store(dc, a, y[0][a], y[NP - 1][a], y0, y1);
            pout[(size_t)a * N] = y0;
            pout[(size_t)a * N + H] = y1;
        } else {
            pout[(size_t)a * N] = y[0][a];
        }
    }
}

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

// ---------------------------------------------------------------------------------------------
// Tensor product over QP (row A5 step 4): d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1
// ---------------------------------------------------------------------------------------------
// MAD (every modulus in (2^59, 2^60)): the operands arrive lazily reduced (< 8q, from the forward transform); two sign-mask
// subtractions bring them below 2q < 2^61, the four products go through the carry-free column accumulators (30-bit low halves,
// <= 31-bit high halves: d1's two products keep every column below 2^63) and one reduction block each (z < 8 q^2 < 2^123):
// 170 VALU instructions per thread where three 128-bit products with two-word Barrett reductions took 297 -- the kernel
// was as much bound by them as by its 115 MB of traffic.
template <bool MAD>
__global__ void __launch_bounds__(TPB) tensor_kernel(const DevConsts *dc, u32 N, u32 M, const u64 *__restrict__ e,
                                                     u64 *__restrict__ d)
{
    // two adjacent coefficients per thread (16-byte lanes; the arrays are point-wise, any order): half the workgroups and waves of the
    // one-coefficient form for the same bytes -- beside the other queue group's transforms that is what counts (r05, relin_mac likewise)
    const u32 n = 2 * (blockIdx.x * TPB + threadIdx.x);
    if (n >= N) return;
    const u32 a = blockIdx.y, bin = blockIdx.z;
    const Mod m = dc->mod[a];
    const size_t MN = (size_t)M * N;
    const u64 *pe = e + (size_t)bin * 4 * MN + (size_t)a * N + n;
    u64 *pd = d + (size_t)bin * 3 * MN + (size_t)a * N + n;
    const u64x2 va0 = *reinterpret_cast<const u64x2 *>(pe), va1 = *reinterpret_cast<const u64x2 *>(pe + MN),
                vb0 = *reinterpret_cast<const u64x2 *>(pe + 2 * MN), vb1 = *reinterpret_cast<const u64x2 *>(pe + 3 * MN);
    u64x2 r0, r1, r2;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        u64 a0 = k ? va0.y : va0.x, a1 = k ? va1.y : va1.x, b0 = k ? vb0.y : vb0.x, b1 = k ? vb1.y : vb1.x;
        u64 d0, d1, d2;
        if (MAD) {
            const u64 nq = neg_u(m.q), n2q = neg_u(2 * m.q), n4q = neg_u(4 * m.q);
            a0 = csub_u(csub_u(a0, n4q), n2q), a1 = csub_u(csub_u(a1, n4q), n2q);
            b0 = csub_u(csub_u(b0, n4q), n2q), b1 = csub_u(csub_u(b1, n4q), n2q);
            const Split30 sa0 = split30(a0), sa1 = split30(a1), sb0 = split30(b0), sb1 = split30(b1);
            ColAcc c = {0, 0, 0};
            colacc_mac(c, sa0, sb0);
            d0 = colacc_reduce<false>(c, m, nq);
            c = ColAcc{0, 0, 0};
            colacc_mac(c, sa0, sb1);
            colacc_mac(c, sa1, sb0);
            d1 = colacc_reduce<false>(c, m, nq);
            c = ColAcc{0, 0, 0};
            colacc_mac(c, sa1, sb1);
            d2 = colacc_reduce<false>(c, m, nq);
        } else {
            d0 = mulmod(a0, b0, m);
            U128 x = mul128(a0, b1);
            mac128(x, a1, b0);
            d1 = reduce128(x, m);
            d2 = mulmod(a1, b1, m);
        }
        if (k) r0.y = d0, r1.y = d1, r2.y = d2;
        else r0.x = d0, r1.x = d1, r2.x = d2;
    }
    *reinterpret_cast<u64x2 *>(pd) = r0;
    *reinterpret_cast<u64x2 *>(pd + MN) = r1;
    *reinterpret_cast<u64x2 *>(pd + 2 * MN) = r2;
}
void launch_tensor(const DevConsts *dc, u32 N, u32 M, const u64 *e, u64 *d, u32 nb, hipStream_t st, bool small_moduli)
{
    dim3 grid((N / 2 + TPB - 1) / TPB, M, nb);   // (N is a power of two >= 8)
    if (small_moduli)
        hipLaunchKernelGGL(tensor_kernel<true>, grid, dim3(TPB), 0, st, dc, N, M, e, d);
    else
        hipLaunchKernelGGL(tensor_kernel<false>, grid, dim3(TPB), 0, st, dc, N, M, e, d);
}

// ---------------------------------------------------------------------------------------------
// Scale-and-round by t/P from QP into Q (row A6)
// ---------------------------------------------------------------------------------------------
// d[M] (mod QP) -> out[L]: round(t d / P) mod Q
// lz (MAD, L <= 5): the results stay in [0, 4q) (colacc_reduce123_lazy): for components that go through fold_store into a
// transform of the 16-coefficient kernel
// PRE: the inputs come from a folded load with the merged constants (DevConsts::fold_iap / fold_iat): the P limbs already hold
// yp_j = [d_j (QP/p_j)^-1]_{p_j}, the Q limbs [d_k t P^-1]_{q_k} -- the products this routine would form first
// PONLY: the own-limb term d_k [t P^-1]_{q_k} is left out and d[.][k < L] is not read.  The term is the only place a Q limb enters, one
// constant times the limb's own coefficients: it commutes with the transform of limb k, and the key-switch MAC adds it in EVALUATION
// form (relin_mac_kernel, EQ) -- components 0 and 1 of a relinearising product.  Every column sum below only loses a term.
// K at ArithKind::fold (NttPlan::fold_moduli): the folded reduction block; one block for z < 2^124, so L = 6 takes it as well
template <u32 L, ArithKind K, int NP, bool PRE = false, bool PONLY = false>
__device__ __forceinline__ void scale_round_core(const DevConsts *dc, const u64 (&d)[NP][2 * L + 1], u64 (&out)[NP][L], bool lz = false)
{
    constexpr bool MAD = colacc(K), FD = K == ArithKind::fold;
    constexpr u32 Lp = L + 1;
    u64 yp[NP][Lp];
    u64 fsum[NP];
    U128 itot[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) fsum[p] = 0, itot[p] = U128{0, 0};
#pragma unroll
    for (u32 j = 0; j < Lp; j++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod pj = ld_mod(c, L + j);
        const u64 w = c->qp_hat_inv[L + j], wsh = c->qp_hat_inv_sh[L + j], tw = c->tQ_modp[j], twsh = c->tQ_modp_sh[j], nq = neg_u(pj.q);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            yp[p][j] = PRE ? d[p][L + j] : mshoup<MAD>(d[p][L + j], w, wsh, pj.q, nq);
            u64 fl, z;
            mdivmod<MAD>(yp[p][j], tw, twsh, pj.q, nq, fl, z);
            add128(itot[p], U128{fl, 0});
            fsum[p] += mfixfrac<MAD>(z, pj);
        }
    }
#pragma unroll
    for (int p = 0; p < NP; p++) add128(itot[p], U128{(fsum[p] + FIX_HALF) >> 60, 0});
#pragma unroll
    for (u32 k = 0; k < L; k++) {
        PIE_ITER_FENCE();
        const DcC c = dc_iter(dc);
        const Mod qk = ld_mod(c, k);
        u64 col[Lp];
#pragma unroll
        for (u32 j = 0; j < Lp; j++) col[j] = c->tQF_modq[j][k];
        const u64 tp = c->tPinv_modq[k], nq = neg_u(qk.q);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            if (MAD && L <= 6) {   // L + 2 products + the integer parts (< (L + 2) 2^60, in column 0)
                ColAcc a = {itot[p].lo, 0, 0};
#pragma unroll
                for (u32 j = 0; j < Lp; j++) colacc_mac(a, split30(yp[p][j]), split30(col[j]));
                if (PONLY)
                    ;
                else if (PRE)
                    a.c0 += d[p][k];  // (canonical, < 2^60: column 0 holds L + 2 products' low parts and the integer parts besides)
                else
                    colacc_mac(a, split30(d[p][k]), split30(tp));
                out[p][k] = (L <= 5 && lz) ? colacc_red_lazy<FD>(a, qk, nq) : colacc_red<FD, (L > 5)>(a, qk, nq);
            } else {
                U128 acc = dot128<Lp, MAD>(yp[p], col);
                if (PONLY)
                    ;
                else if (PRE)
                    add128(acc, U128{d[p][k], 0});
                else
                    mac128(acc, d[p][k], tp);
                add128(acc, itot[p]);
                out[p][k] = reduce128(acc, qk);
            }
        }
    }
}

// FOLD: inverse outer stage on load; forward outer stage on the store of components 0 and 1 (they go to a
// forward transform); component 2 is stored as plain coefficients (the digit kernel folds it per target modulus)
// PONLY: this component takes its P limbs only (scale_round_core); the loads of the Q limbs and their folded-load products go with the term
template <bool FOLD, u32 L, ArithKind K, bool PONLY>
__device__ __forceinline__ void scale_round_comp(const DevConsts *__restrict__ dc, u32 N, u32 n, const u64 *__restrict__ pin,
                                                 u64 *__restrict__ pout, bool fold_out, bool lz)
{
    const u32 H = N / 2;
    constexpr u32 M = 2 * L + 1;
    constexpr int NP = FOLD ? 2 : 1;
    u64 x[NP][M], y[NP][L];
#pragma unroll
    for (u32 a = PONLY ? L : 0; a < M; a++) {
        if (FOLD) {
            // the folded load and the first product of scale-and-round in one Shoup multiplication (merged constants)
            PIE_ITER_FENCE();
            const DcC c = dc_iter(dc);
            const u32 ak = a < L ? a : 0, aj = a < L ? 0 : a - L;
            const u64 q = c->mod[a].q, nq = neg_u(q), u = pin[(size_t)a * N], v = pin[(size_t)a * N + H];
            const u64 wa = a < L ? c->fold_iat[ak] : c->fold_iap[aj], was = a < L ? c->fold_iat_sh[ak] : c->fold_iap_sh[aj];
            const u64 wb = a < L ? c->fold_ibt[ak] : c->fold_ibp[aj], wbs = a < L ? c->fold_ibt_sh[ak] : c->fold_ibp_sh[aj];
            x[0][a] = shoup63(u + v, wa, was, nq);                // u, v in [0, 4q)
            x[NP - 1][a] = shoup63(u + (4 * q - v), wb, wbs, nq);
        } else {
            x[0][a] = pin[(size_t)a * N];
        }
    }
    scale_round_core<L, K, NP, FOLD, PONLY>(dc, x, y, lz);
#pragma unroll
    for (u32 k = 0; k < L; k++) {
        PIE_ITER_FENCE();
        if (FOLD) {
            u64 y0 = y[0][k], y1 = y[NP - 1][k];
            if (fold_out) fold_store(dc, k, y[0][k], y[NP - 1][k], y0, y1);
            pout[(size_t)k * N] = y0;
            pout[(size_t)k * N + H] = y1;
        } else {
            pout[(size_t)k * N] = y[0][k];
        }
    }
}
// P01: components 0 and 1 are the PONLY variant (a uniform branch on the component: blockIdx.y), component 2 the full one
// P2 (with P01 and fold_comp2; NttPlan::result_eval_q): component 2 is the PONLY variant too -- a product that is not relinearised
template <bool FOLD, u32 L, ArithKind K, bool P01 = false, bool P2 = false>
__global__ void __launch_bounds__(TPB) scale_round_kernel(const DevConsts *__restrict__ dc, u32 N, const u64 *__restrict__ d,
                                                          u64 *__restrict__ out01, size_t stride01,
                                                          u64 *__restrict__ out2, size_t stride2, u32 fold_comp2)
{
    static_assert((colacc(K) || !P01) && (P01 || !P2), "P limbs only: a column-accumulator kind, component 2 with components 0 and 1");
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    if (n >= (FOLD ? N / 2 : N)) return;
    const u32 comp = blockIdx.y, bin = blockIdx.z;
    constexpr u32 M = 2 * L + 1;
    const u64 *pin = d + ((size_t)(bin * 3 + comp) * M) * N + n;
    u64 *pout = comp < 2 ? out01 + (size_t)bin * stride01 + (size_t)comp * L * N + n : out2 + (size_t)bin * stride2 + n;
    // d0, d1 of the key-switch path go on through fold_store into the forward transform ([0, 8q) in): [0, 4q) will do.  d2 feeds the
    // digit lift (canonical), and with fold_comp2 the three components leave the library's lane-ordered world
    const bool lz = FOLD && colacc(K) && comp < 2 && !fold_comp2;
    if (P01 && comp < 2)
        scale_round_comp<FOLD, L, K, true>(dc, N, n, pin, pout, true, lz);
    else if (P2 && comp == 2)
        scale_round_comp<FOLD, L, K, true>(dc, N, n, pin, pout, fold_comp2, lz);
    else
        scale_round_comp<FOLD, L, K, false>(dc, N, n, pin, pout, comp < 2 || fold_comp2, lz);
}
void launch_scale_round(const DevConsts *dc, u32 N, u32 L, const u64 *d, u32 nb, u64 *out01, size_t stride01, u64 *out2,
                        size_t stride2, hipStream_t st, Arith ar, bool fold, bool fold_comp2, bool p_only01, bool p_only2)
{
    assert(!p_only01 || (ar.mad && fold_comp2 == p_only2));
    assert(!p_only2 || p_only01);
    dim3 grid(((fold ? N / 2 : N) + TPB - 1) / TPB, 3, nb);
    const u32 fc2 = (fold_comp2 && fold) ? 1u : 0u;
    with_u32<1, 7>(L, [&](auto L_) {
        with_arith(ar, [&](auto K_) {
            with_bools([&](auto F_, auto P01_, auto P2_) {
                if constexpr ((colacc(K_()) || !P01_()) && (P01_() || !P2_()))   // (the asserts above)
                    hipLaunchKernelGGL((scale_round_kernel<F_(), L_(), K_(), P01_(), P2_()>), grid, dim3(TPB), 0, st, dc, N, d, out01, stride01,
                                       out2, stride2, fc2);
            }, fold, p_only01, p_only2);
        });
    });
}

// ---------------------------------------------------------------------------------------------
// BV relinearisation (row A7): digit decomposition and key-switch accumulation
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 digit_lift(const DevConsts *dc, u32 i, u32 j, u64 v)
{
    const Mod &mj = dc->mod[j];
    const u64 qi = dc->mod[i].q;
    u64 r = (qi < 2 * mj.q) ? (v >= mj.q ? v - mj.q : v) : barrett128(0, v, mj);
    if (v > qi / 2) r = submod(r, dc->qi_modqj[i][j], mj.q);  // centred lift of the residue mod q_i
    return r;
}
template <bool FOLD>
__global__ void __launch_bounds__(TPB) digits_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, const u64 *__restrict__ d2,
                                                     size_t stride2, u64 *__restrict__ dig)
{
    const u32 n = blockIdx.x * TPB + threadIdx.x;
    const u32 H = N / 2;
    if (n >= (FOLD ? H : N)) return;
    const u32 i = blockIdx.y / L, j = blockIdx.y % L, bin = blockIdx.z;
    const u64 *pin = d2 + (size_t)bin * stride2 + (size_t)i * N + n;
    u64 *pout = dig + (((size_t)bin * L + i) * L + j) * N + n;
    if (FOLD) {
        u64 y0, y1;
        fold_store(dc, j, digit_lift(dc, i, j, pin[0]), digit_lift(dc, i, j, pin[H]), y0, y1);
        pout[0] = y0;
        pout[H] = y1;
    } else {
        pout[0] = digit_lift(dc, i, j, pin[0]);
    }
}
void launch_digits(const DevConsts *dc, u32 N, u32 L, const u64 *d2, size_t stride2, u32 nb, u64 *dig, hipStream_t st, bool fold)
{
    dim3 grid(((fold ? N / 2 : N) + TPB - 1) / TPB, L * L, nb);
    if (fold)
        hipLaunchKernelGGL(digits_kernel<true>, grid, dim3(TPB), 0, st, dc, N, L, d2, stride2, dig);
    else
        hipLaunchKernelGGL(digits_kernel<false>, grid, dim3(TPB), 0, st, dc, N, L, d2, stride2, dig);
}

// The lane-order LDS tile of the key-switch MAC and the degree-2 finish.  Inputs in the lane order of a register-blocked transform with
// T threads per slice and KP coefficient pairs per thread: pair k of thread tau sits at k T + tau and belongs at KP tau + k.  A block takes
// the (256 / KP) x KP pairs of threads tau0 .. tau0 + 256 / KP - 1, i.e. KP contiguous runs of the lane order, and hands the results through
// LDS so that they leave as one contiguous 4 KiB run of the standard order; with a plain out_map scatter every 16-byte store lands in its
// own stretch.  KP = 16: kernels_ntt_fast.hip (32 coefficients per thread), KP = 8: ntt16_kernel.h.
struct LaneTile {
    u32 n;         // this thread's first coefficient, in lane order
    u32 std_pair;  // first standard-order pair of the block's tile
    u32 k, tt;     // the thread's place in the tile: pair k of the transform's thread tau0 + tt
};
template <int KP>
__device__ __forceinline__ LaneTile lane_tile(u32 T)
{
    constexpr u32 TT = TPB / KP;  // threads of the transform per tile
    const u32 tiles = T / TT, slice = blockIdx.x / tiles, tau0 = (blockIdx.x % tiles) * TT;
    const u32 k = threadIdx.x / TT, tt = threadIdx.x % TT;
    return {2 * (slice * KP * T + k * T + tau0 + tt), slice * KP * T + KP * tau0, k, tt};
}
// this thread's pair inside the tile, standard order: KP (tau - tau0) + k
template <int KP>
__device__ __forceinline__ u32 lane_tile_slot(const LaneTile &lt)
{
    return KP * lt.tt + lt.k;
}
// the host's side of it: a kernel built with KP = kp takes this lane order
static bool lane_tile_applies(u32 N, u32 T, u32 kp)
{
    return (kp == 16 || kp == 8) && T >= TPB / kp && T % (TPB / kp) == 0 && (N / 2) % TPB == 0;
}

// The own-limb terms of one coefficient at limb j: v[c] = [t P^-1]_{q_j} (a (x) b)_c in [0, 4q) for the first NT components of the tensor
// product (a0 b0, a0 b1 + a1 b0, a1 b1), formed as tensor_kernel<true> forms them: the operands ([0, 8q) residues) brought below 2q by
// own_limb_operand's two sign-mask subtractions, d1's two products keep every column below 2^63, z < 8 q^2 < 2^123; one lazy reduction
// block and one Shoup product with the constant each.
__device__ __forceinline__ Split30 own_limb_operand(u64 w, u64 n2q, u64 n4q) { return split30(csub_u(csub_u(w, n4q), n2q)); }
template <int NT>
__device__ __forceinline__ void own_limb_terms(const Split30 &sa0, const Split30 &sa1, const Split30 &sb0, const Split30 &sb1, const Mod &m,
                                               u64 nq, u64 tp, u64 tpsh, u64 (&v)[NT])
{
    ColAcc t = {0, 0, 0};
    colacc_mac(t, sa0, sb0);
    v[0] = shoup63_lazy(colacc_reduce123_lazy(t, m, nq), tp, tpsh, nq);
    t = ColAcc{0, 0, 0};
    colacc_mac(t, sa0, sb1);
    colacc_mac(t, sa1, sb0);
    v[1] = shoup63_lazy(colacc_reduce123_lazy(t, m, nq), tp, tpsh, nq);
    if constexpr (NT == 3) {
        t = ColAcc{0, 0, 0};
        colacc_mac(t, sa1, sb1);
        v[2] = shoup63_lazy(colacc_reduce123_lazy(t, m, nq), tp, tpsh, nq);
    }
}

// One thread: two adjacent coefficients (16-byte lanes) of one (bin, limb j), both ciphertext components, so a
// digit is loaded once for its two key products.  out_map (lane order -> standard) keeps pairs adjacent.
// KP > 0: lane-ordered inputs, the stores go through the LDS tile (lane_tile above).
// RPT = 2 (column-accumulator path only): one thread takes the same coefficient pair of TWO ciphertext rows that use the same key -- rows
// r and r + key_group -- and loads every key word once for both.  The kernel is bound by the traffic through the L1s (330 MB per step at
// the headline shape, more than half of it key words that every row re-reads from the L2: profiles/r05/stage_a_batch_layer_groups.txt
// has the model); a launch's last block of rows may have no second row (uniform branch).
// EQ (column-accumulator path only; NttPlan::d01_eval_q): d01 arrives without the own-limb term of scale-and-round (scale_round_core, PONLY).
// Its transform is [t P^-1]_{q_j} times limb j of the tensor product in EVALUATION form, which this kernel forms from the QP operands
// eqp[row][4][eqp_M][N] (a0 a1 b0 b1 at limb j, ordered like d01, [0, 8q) residues) as tensor_kernel<true> does: t0 = a0 b0 for component
// 0, t1 = a0 b1 + a1 b0 for component 1 (own_limb_terms).
template <bool MAD, int KP, int RPT = 1, bool EQ = false>
__global__ void __launch_bounds__(TPB) relin_mac_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, const u64 *__restrict__ d01,
                                                        size_t stride01, const u64 *__restrict__ dig,
                                                        const u64 *__restrict__ key0, const u64 *__restrict__ mask,
                                                        u64 *__restrict__ out, const u32 *__restrict__ out_map,
                                                        size_t key_stride, u32 key_group, u32 T, u32 mask_div, u32 nb,
                                                        const u64 *__restrict__ eqp, u32 eqp_M)
{
    static_assert(RPT == 1 || MAD, "two rows per thread: the column-accumulator path");
    static_assert(!EQ || MAD, "the own-limb term: the column-accumulator path");
    constexpr bool TILE = KP > 0;
    __shared__ u64x2 s_tile[TILE ? 2 * RPT : 1][TILE ? TPB : 1];
    u32 n = 2 * (blockIdx.x * TPB + threadIdx.x);
    LaneTile lt = {};
    if constexpr (TILE) {
        lt = lane_tile<KP>(T);
        n = lt.n;
    }
    if (n >= N) return;
    const u32 j = blockIdx.y;
    // rows of this thread: RPT = 1: row blockIdx.z; RPT = 2: rows 2 k G + q and (2 k + 1) G + q of key q (k = z / G, q = z % G)
    u32 rows[RPT];
    bool has[RPT];
    if (RPT == 1) {
        rows[0] = blockIdx.z, has[0] = true;
    } else {
        const u32 k = blockIdx.z / key_group, q = blockIdx.z % key_group;
        rows[0] = 2 * k * key_group + q, has[0] = rows[0] < nb;
        rows[RPT - 1] = rows[0] + key_group, has[RPT - 1] = rows[RPT - 1] < nb;
        if (!has[0]) return;
    }
    const u32 bin = rows[0];
    const u64 *key = key0 + (size_t)(bin % key_group) * key_stride;  // one key per position in a group (EvalMerge)
    const Mod m = dc->mod[j];
    const size_t LN = (size_t)L * N;
    const u32 po = TILE ? 0 : (out_map ? out_map[n] : n);
    u64x2 res[RPT][2];
    if (MAD) {
        // column accumulators end to end: the L products, then d01 (it may arrive unnormalised, < 2^63, from the forward
        // transform) into column 0 -- (L + 8) 2^60 < 2^64 -- and one reduction block; the mask product likewise.
        // EQ: the own-limb term v < 4q < 2^62 joins as its 30-bit halves, v mod 2^30 into column 0 and v >> 30 < 2^32 into column 1.
        // Column 0 then holds less than (L + 8) 2^60 + 2^30 <= 15 2^60 + 2^30 < 2^64 at L = 7 (whole, the term would make it
        // (L + 9) 2^60 = 2^64 there); column 1 less than 2 L 2^60 + 2^32; the value z grows by less than 2^62, far inside the reduction
        // block's 2^123 (L products below 2^120 each).
        ColAcc a[RPT][2][2];
#pragma unroll
        for (int r = 0; r < RPT; r++)
#pragma unroll
            for (int c = 0; c < 2; c++) a[r][c][0] = a[r][c][1] = ColAcc{0, 0, 0};
        for (u32 i = 0; i < L; i++) {
            const u64x2 k0 = *reinterpret_cast<const u64x2 *>(key + (((size_t)i * 2 + 0) * L + j) * N + n);
            const u64x2 k1 = *reinterpret_cast<const u64x2 *>(key + (((size_t)i * 2 + 1) * L + j) * N + n);
            const Split30 k0x = split30(k0.x), k0y = split30(k0.y), k1x = split30(k1.x), k1y = split30(k1.y);
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                if (r && !has[r]) continue;
                const u64x2 d = *reinterpret_cast<const u64x2 *>(dig + (((size_t)rows[r] * L + i) * L + j) * N + n);
                const Split30 dx = split30(d.x), dy = split30(d.y);
                colacc_mac(a[r][0][0], dx, k0x);
                colacc_mac(a[r][0][1], dy, k0y);
                colacc_mac(a[r][1][0], dx, k1x);
                colacc_mac(a[r][1][1], dy, k1y);
            }
        }
        const u64 nq = 0 - m.q;
        if (EQ) {
            const u64 n2q = neg_u(2 * m.q), n4q = neg_u(4 * m.q);
            const u64 tp = dc->tPinv_modq[j], tpsh = dc->tPinv_modq_sh[j];
            const size_t MN = (size_t)eqp_M * N;
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                if (r && !has[r]) continue;
                const u64 *pe = eqp + (size_t)rows[r] * 4 * MN + (size_t)j * N + n;
                const u64x2 va0 = *reinterpret_cast<const u64x2 *>(pe), va1 = *reinterpret_cast<const u64x2 *>(pe + MN),
                            vb0 = *reinterpret_cast<const u64x2 *>(pe + 2 * MN), vb1 = *reinterpret_cast<const u64x2 *>(pe + 3 * MN);
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const Split30 sa0 = own_limb_operand(k ? va0.y : va0.x, n2q, n4q), sa1 = own_limb_operand(k ? va1.y : va1.x, n2q, n4q);
                    const Split30 sb0 = own_limb_operand(k ? vb0.y : vb0.x, n2q, n4q), sb1 = own_limb_operand(k ? vb1.y : vb1.x, n2q, n4q);
                    u64 v[2];
                    own_limb_terms<2>(sa0, sa1, sb0, sb1, m, nq, tp, tpsh, v);
                    const u64 v0 = v[0], v1 = v[1];
                    a[r][0][k].c0 += v0 & 0x3FFFFFFFull, a[r][0][k].c1 += v0 >> 30;
                    a[r][1][k].c0 += v1 & 0x3FFFFFFFull, a[r][1][k].c1 += v1 >> 30;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            if (r && !has[r]) continue;
            u64x2 mk;
            if (mask) mk = *reinterpret_cast<const u64x2 *>(mask + (size_t)(rows[r] / mask_div) * LN + (size_t)j * N + n);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const u64x2 s = *reinterpret_cast<const u64x2 *>(d01 + (size_t)rows[r] * stride01 + (size_t)c * LN + (size_t)j * N + n);
                a[r][c][0].c0 += s.x;
                a[r][c][1].c0 += s.y;
                res[r][c].x = colacc_reduce<false>(a[r][c][0], m, nq);
                res[r][c].y = colacc_reduce<false>(a[r][c][1], m, nq);
                if (mask) {
                    ColAcc p0 = {0, 0, 0}, p1 = {0, 0, 0};
                    colacc_mac(p0, split30(res[r][c].x), split30(mk.x));
                    colacc_mac(p1, split30(res[r][c].y), split30(mk.y));
                    res[r][c].x = colacc_reduce<false>(p0, m, nq);
                    res[r][c].y = colacc_reduce<false>(p1, m, nq);
                }
            }
        }
    } else {
        u64x2 mk;
        if (mask) mk = *reinterpret_cast<const u64x2 *>(mask + (size_t)(bin / mask_div) * LN + (size_t)j * N + n);
        U128 acc[2][2];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int e = 0; e < 2; e++) acc[c][e] = U128{0, 0};
        for (u32 i = 0; i < L; i++) {
            const u64x2 d = *reinterpret_cast<const u64x2 *>(dig + (((size_t)bin * L + i) * L + j) * N + n);
            const u64x2 k0 = *reinterpret_cast<const u64x2 *>(key + (((size_t)i * 2 + 0) * L + j) * N + n);
            const u64x2 k1 = *reinterpret_cast<const u64x2 *>(key + (((size_t)i * 2 + 1) * L + j) * N + n);
            mac128(acc[0][0], d.x, k0.x);
            mac128(acc[0][1], d.y, k0.y);
            mac128(acc[1][0], d.x, k1.x);
            mac128(acc[1][1], d.y, k1.y);
        }
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const u64x2 s = *reinterpret_cast<const u64x2 *>(d01 + (size_t)bin * stride01 + (size_t)c * LN + (size_t)j * N + n);
            // d01 joins the sum before the reduction: it may arrive unnormalised (< 2^63) from the forward transform
            add128(acc[c][0], U128{s.x, 0});
            add128(acc[c][1], U128{s.y, 0});
            res[0][c].x = reduce128(acc[c][0], m);
            res[0][c].y = reduce128(acc[c][1], m);
            if (mask) {
                res[0][c].x = mulmod(res[0][c].x, mk.x, m);
                res[0][c].y = mulmod(res[0][c].y, mk.y, m);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (r && !has[r]) continue;
            const u64x2 v = res[r][c];
            if constexpr (TILE)
                // (lane_tile_slot, formed again from threadIdx at the store as this kernel always did: from lt.k and lt.tt its listing changes)
                s_tile[2 * r + c][KP * (threadIdx.x % (TPB / KP)) + threadIdx.x / (TPB / KP)] = v;
            else
                *reinterpret_cast<u64x2 *>(out + ((size_t)rows[r] * 2 + c) * LN + (size_t)j * N + po) = v;
        }
    if (TILE) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RPT; r++)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (r && !has[r]) continue;
                *reinterpret_cast<u64x2 *>(out + ((size_t)rows[r] * 2 + c) * LN + (size_t)j * N + 2 * (lt.std_pair + threadIdx.x)) = s_tile[2 * r + c][threadIdx.x];
            }
    }
}
void launch_relin_mac(const DevConsts *dc, u32 N, u32 L, const u64 *d01, size_t stride01, const u64 *dig, const u64 *key,
                      const u64 *mask, u64 *out, u32 nb, hipStream_t st, bool small_moduli, const u32 *out_map, size_t key_stride,
                      u32 key_group, u32 sigma_T, u32 sigma_kp, u32 mask_div, const u64 *eqp, u32 eqp_M)
{
    assert(!eqp || (small_moduli && eqp_M >= L));
    if (!key_group) key_group = 1;
    if (!mask_div) mask_div = 1;
    // sigma_T: out_map is the lane order of a register-blocked transform with sigma_T threads per slice, sigma_kp pairs per thread
    const bool tile = out_map && lane_tile_applies(N, sigma_T, sigma_kp);
    const int kp = tile ? (int)sigma_kp : 0;
    // two rows per thread where at least two rows share a key (the column-accumulator path)
    const bool two = small_moduli && nb >= 2 * key_group;
    const u32 zrows = two ? ((nb + 2 * key_group - 1) / (2 * key_group)) * key_group : nb;
    dim3 grid((N / 2 + TPB - 1) / TPB, L, zrows);
    auto launch = [&](auto KP_) {
        with_bools([&](auto M_, auto R2_, auto E_) {
            if constexpr (M_() || (!R2_() && !E_()))   // two rows per thread and the own-limb term: the column-accumulator path
                hipLaunchKernelGGL((relin_mac_kernel<M_(), KP_(), R2_() ? 2 : 1, E_()>), grid, dim3(TPB), 0, st, dc, N, L, d01, stride01, dig, key,
                                   mask, out, out_map, key_stride, key_group, sigma_T, mask_div, nb, eqp, eqp_M);
        }, small_moduli, two, eqp != nullptr);
    };
    if (kp == 16) launch(std::integral_constant<int, 16>{});
    else if (kp == 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 0>{});
}

// ---------------------------------------------------------------------------------------------
// Degree-2 results (include/piehip.h "Result relinearisation"; NttPlan::result_eval_q): the last product of run() is not relinearised.
// Its three components arrive as relin_mac_kernel<.., EQ> takes d0 and d1: d[row][3][L][N], the forward transform (lane order, [0, 8q)
// residues) of scale-and-round's P-limb part, without the own-limb term.  This kernel adds that term -- [t P^-1]_{q_j} times limb j of
// (a0 b0, a0 b1 + a1 b0, a1 b1), formed from the QP operands e[row][4][eqp_M][N] exactly as there -- multiplies by the mask and writes
// the result row out[row][3][L][N] in standard order through the LDS tile.  No digit, no key.  One thread: two adjacent coefficients
// of one (row, limb j), all three components: the four operand words are loaded once for their four products.
// Column 0 of a component's accumulator holds d (< 2^63) and v mod 2^30, column 1 v >> 30 < 2^32: one reduction block.
template <int KP>
__global__ void __launch_bounds__(TPB) deg2_finish_kernel(const DevConsts *__restrict__ dc, u32 N, u32 L, const u64 *__restrict__ d,
                                                          const u64 *__restrict__ eqp, u32 eqp_M, const u64 *__restrict__ mask,
                                                          u64 *__restrict__ out, u32 T, u32 mask_div)
{
    __shared__ u64x2 s_tile[3][TPB];
    const LaneTile lt = lane_tile<KP>(T);
    const u32 n = lt.n;
    const u32 j = blockIdx.y, row = blockIdx.z;
    const Mod m = dc->mod[j];
    const size_t LN = (size_t)L * N, MN = (size_t)eqp_M * N;
    const u64 nq = 0 - m.q, n2q = neg_u(2 * m.q), n4q = neg_u(4 * m.q);
    const u64 tp = dc->tPinv_modq[j], tpsh = dc->tPinv_modq_sh[j];
    const u64 *pe = eqp + (size_t)row * 4 * MN + (size_t)j * N + n;
    const u64x2 va0 = *reinterpret_cast<const u64x2 *>(pe), va1 = *reinterpret_cast<const u64x2 *>(pe + MN),
                vb0 = *reinterpret_cast<const u64x2 *>(pe + 2 * MN), vb1 = *reinterpret_cast<const u64x2 *>(pe + 3 * MN);
    const u64x2 mk = *reinterpret_cast<const u64x2 *>(mask + (size_t)(row / mask_div) * LN + (size_t)j * N + n);
    u64x2 s[3];
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] = *reinterpret_cast<const u64x2 *>(d + ((size_t)row * 3 + c) * LN + (size_t)j * N + n);
    u64 res[3][2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const Split30 sa0 = own_limb_operand(k ? va0.y : va0.x, n2q, n4q), sa1 = own_limb_operand(k ? va1.y : va1.x, n2q, n4q);
        const Split30 sb0 = own_limb_operand(k ? vb0.y : vb0.x, n2q, n4q), sb1 = own_limb_operand(k ? vb1.y : vb1.x, n2q, n4q);
        const Split30 smk = split30(k ? mk.y : mk.x);
        u64 v[3];
        own_limb_terms<3>(sa0, sa1, sb0, sb1, m, nq, tp, tpsh, v);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            ColAcc a = {(k ? s[c].y : s[c].x) + (v[c] & 0x3FFFFFFFull), v[c] >> 30, 0};
            ColAcc p = {0, 0, 0};
            colacc_mac(p, split30(colacc_reduce<false>(a, m, nq)), smk);
            res[c][k] = colacc_reduce<false>(p, m, nq);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) s_tile[c][lane_tile_slot<KP>(lt)] = u64x2{res[c][0], res[c][1]};
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; c++)
        *reinterpret_cast<u64x2 *>(out + ((size_t)row * 3 + c) * LN + (size_t)j * N + 2 * (lt.std_pair + threadIdx.x)) = s_tile[c][threadIdx.x];
}
bool deg2_finish_applies(u32 N, u32 sigma_T, u32 sigma_kp)
{
    // (the 16-coefficient kernel's lane order: the only one a plan with result_eval_q has)
    return sigma_kp == 8 && lane_tile_applies(N, sigma_T, sigma_kp);
}
void launch_deg2_finish(const DevConsts *dc, u32 N, u32 L, const u64 *d, const u64 *eqp, u32 eqp_M, const u64 *mask, u64 *out, u32 nb,
                        hipStream_t st, u32 sigma_T, u32 sigma_kp, u32 mask_div)
{
    assert(deg2_finish_applies(N, sigma_T, sigma_kp) && eqp_M >= L);
    dim3 grid(N / 2 / TPB, L, nb);
    hipLaunchKernelGGL(deg2_finish_kernel<8>, grid, dim3(TPB), 0, st, dc, N, L, d, eqp, eqp_M, mask, out, sigma_T, mask_div ? mask_div : 1);
}

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
// Limb drop (include/piehip.h "Result limbs"): in[npoly][L][N] -> out[npoly][KEEP][N], COEFFICIENT format, canonical residues.
// One thread holds the L residues of one coefficient and drops the limbs L - 1 .. KEEP one after the other:
//     r = c mod q_l centred,  c_i <- (c_i - r) q_l^-1 mod q_i  for i < l.
// With s = [c_l > (q_l - 1) / 2] as a 64-bit sign mask, c_i - r = c_i - c_l + (s ? q_l : off) where off is a multiple of q_i that
// is >= (q_l - 1) / 2 (DevConsts::drop_off): one non-negative word below 2^63 for moduli of any widths, which the Shoup product
// with q_l^-1 takes as it is.  (L - KEEP)(L + KEEP - 1) / 2 such products per coefficient; every constant is wave-uniform
// (scalar loads, the indices are compile-time), the conditional subtraction is csub_u's sign-mask block.
// ---------------------------------------------------------------------------------------------
template <int L, int KEEP>
__global__ void __launch_bounds__(TPB) limb_drop_kernel(const DevConsts *__restrict__ dc, u32 N, u32 blocks_per_poly,
                                                        const u64 *__restrict__ in, u64 *__restrict__ out)
{
    const u32 poly = blockIdx.x / blocks_per_poly;
    const u32 n = (blockIdx.x % blocks_per_poly) * TPB + threadIdx.x;
    if (n >= N) return;
    const u64 *pin = in + (size_t)poly * L * N + n;
    u64 c[L];
#pragma unroll
    for (int i = 0; i < L; i++) c[i] = pin[(size_t)i * N];
#pragma unroll
    for (int l = L - 1; l >= KEEP; l--) {
        const u64 ql = dc->mod[l].q;
        const u64 v = c[l];
        const u64 s = (u64)((int64_t)((ql >> 1) - v) >> 63);  // all ones when the centred residue is negative
#pragma unroll
        for (int i = 0; i < l; i++) {
            const u64 off = dc->drop_off[l][i];
            const u64 x = c[i] - v + off + (s & (ql - off));
            c[i] = mul_shoup_u(x, dc->drop_inv[l][i], dc->drop_inv_sh[l][i], dc->mod[i].q, dc->drop_negq[i]);
        }
    }
    u64 *pout = out + (size_t)poly * KEEP * N + n;
#pragma unroll
    for (int i = 0; i < KEEP; i++) pout[(size_t)i * N] = c[i];
}
// the 21 pairs 1 <= keep < L <= MAX_L = 7 a drop kernel is built for, as template arguments
template <class F>
static bool with_limb_pair(u32 L, u32 keep, F &&f)
{
    bool built = false;
    with_u32<2, 7>(L, [&](auto L_) { built = with_u32<1, L_() - 1>(keep, [&](auto K_) { f(L_, K_); }); });
    return built;
}
bool launch_limb_drop(const DevConsts *dc, u32 N, u32 L, u32 keep, const u64 *in, u64 *out, u32 npoly, hipStream_t st)
{
    if (keep < 1 || keep >= L || L > MAX_L || !npoly) return false;
    const u32 bpp = (N + TPB - 1) / TPB;
    const dim3 grid(bpp * npoly), block(TPB);
    return with_limb_pair(L, keep, [&](auto L_, auto K_) {
        hipLaunchKernelGGL((limb_drop_kernel<(int)L_(), (int)K_()>), grid, block, 0, st, dc, N, bpp, in, out);
    });
}

// ---------------------------------------------------------------------------------------------
// Chain limbs (include/piehip.h "Chain limbs"): the limb drop in front of the product chain.  The accumulators leave stage A and
// the inverse transform on the handle's L limbs; the chain runs on the level context of the first LC.
// ---------------------------------------------------------------------------------------------
// The drop as a launch of its own (the fallback of the fused kernel below): npoly polynomials data[npoly][L][N] in COEFFICIENT format,
// as the inverse transform left them -- FOLD: outer stage pending, residues in [0, 4q) -- are overwritten IN PLACE, at the parent's
// strides, by their first KEEP limbs after the drop: canonical, nothing pending.  Limbs KEEP .. L - 1 keep what they held.  A thread
// owns its coefficient's (FOLD: its coefficient pair's) column of every limb, so nothing it overwrites is read by another.
// The polynomials come in groups of `per` neighbours, `gstride` words from one group to the next: the accumulators of some inner hash
// functions out of rows [rows][K][2][L][N] (chain schedule: each product has its own level), or per = npoly for one packed array.
template <bool FOLD, u32 L, u32 KEEP>
__global__ void __launch_bounds__(TPB) chain_drop_kernel(const DevConsts *__restrict__ dc, u32 N, u32 blocks_per_poly, u64 *data, u32 per,
                                                         size_t gstride)
{
    constexpr int NP = FOLD ? 2 : 1;
    const u32 poly = blockIdx.x / blocks_per_poly;
    const u32 n = (blockIdx.x % blocks_per_poly) * TPB + threadIdx.x;
    const u32 H = N / 2;
    if (n >= (FOLD ? H : N)) return;
    u64 *p = data + (size_t)(poly / per) * gstride + (size_t)(poly % per) * L * N + n;
    u64 c[NP][L];
#pragma unroll
    for (u32 i = 0; i < L; i++) {
        if (FOLD)
            fold_load(dc, i, p[(size_t)i * N], p[(size_t)i * N + H], c[0][i], c[NP - 1][i]);
        else
            c[0][i] = p[(size_t)i * N];
    }
    drop_limbs<L, KEEP, NP, FOLD>(dc, c);  // (folding implies q < 2^60)
#pragma unroll
    for (u32 i = 0; i < KEEP; i++) {
        p[(size_t)i * N] = c[0][i];
        if (FOLD) p[(size_t)i * N + H] = c[NP - 1][i];
    }
}
bool launch_chain_drop(const DevConsts *dc, u32 N, u32 L, u32 keep, u64 *data, u32 npoly, hipStream_t st, bool fold, u32 per, size_t gstride)
{
    if (keep < 1 || keep >= L || L > MAX_L || !npoly) return false;
    if (!per) per = npoly, gstride = 0;   // one packed array
    if (npoly % per) return false;
    const u32 bpp = ((fold ? N / 2 : N) + TPB - 1) / TPB;
    const dim3 grid(bpp * npoly), block(TPB);
    return with_limb_pair(L, keep, [&](auto L_, auto K_) {
        with_bools([&](auto F_) { hipLaunchKernelGGL((chain_drop_kernel<F_(), L_(), K_()>), grid, block, 0, st, dc, N, bpp, data, per, gstride); }, fold);
    });
}

// Both conversions of a product on a level context whose operands are plain COEFFICIENT polynomials (ExpandIn::plain), X and Y each
// with its own distance between the two polynomials of a ciphertext -- the accumulators stay at the parent's strides, an intermediate
// product is packed.  expand_both_kernel's grid and row order.
template <bool FOLD, u32 L, ArithKind K>
__global__ void __launch_bounds__(TPB) expand_both_plain_kernel(const DevConsts *__restrict__ dc, u32 N, const u64 *__restrict__ x, size_t sx,
                                                                size_t six, const u64 *__restrict__ y, size_t sy, size_t siy,
                                                                u64 *__restrict__ out, u32 n_outer)
{
    if (blockIdx.y < 2 * n_outer)
        expand_body<true, FOLD, L, K, false, ExpandIn::plain>(dc, dc, N, y, sy, siy, out, 4, 2, blockIdx.y);
    else
        expand_body<false, FOLD, L, K, false, ExpandIn::plain>(dc, dc, N, x, sx, six, out, 4, 0, blockIdx.y - 2 * n_outer);
}

// The fused form (folded rings, every modulus in (2^59, 2^60)): expand_both_kernel of the level context with the drop from the parent's
// L limbs in front of its conversions (ExpandIn::drop; dcp: the parent's constants, dcl: the level's) into the level's QP operand rows
// [4][2 LC + 1][N].  The dropped X differs from what the QP array may hold in EVALUATION form, so X's Q limbs are written.
// XDROP false (later products of K >= 3): X is an intermediate product on the level's limbs, packed, as the level's folded inverse
// transform left it -- the pending load, Q limbs already in place (SKIPQ); Y is an accumulator and is dropped all the same.
template <u32 L, u32 LC, bool XDROP, ArithKind K>
__global__ void __launch_bounds__(TPB) expand_both_drop_kernel(const DevConsts *__restrict__ dcp, const DevConsts *__restrict__ dcl, u32 N,
                                                               const u64 *__restrict__ x, size_t sx, size_t six, const u64 *__restrict__ y,
                                                               size_t sy, size_t siy, u64 *__restrict__ out, u32 n_outer)
{
    if (blockIdx.y < 2 * n_outer)
        expand_body<true, true, LC, K, false, ExpandIn::drop, L>(dcp, dcl, N, y, sy, siy, out, 4, 2, blockIdx.y);
    else if (XDROP)
        expand_body<false, true, LC, K, false, ExpandIn::drop, L>(dcp, dcl, N, x, sx, six, out, 4, 0, blockIdx.y - 2 * n_outer);
    else
        expand_body<false, true, LC, K, true, ExpandIn::pending, LC>(dcl, dcl, N, x, sx, six, out, 4, 0, blockIdx.y - 2 * n_outer);
}
// Chain schedule (include/piehip.h): a product of K >= 3 whose level LC lies below the level LX of the product before it.  Y is an
// accumulator on the handle's LY limbs (dcy); X is that earlier product, packed on LX limbs as level LX's folded inverse transform
// left it, loaded and dropped with level LX's constants (dcx); both are converted with level LC's (dcl).  LX = LY -- the earlier
// product ran on every limb -- is expand_both_drop_kernel<LY, LC, true, K> itself, X at the product's strides.
template <u32 LY, u32 LX, u32 LC, ArithKind K>
__global__ void __launch_bounds__(TPB) expand_both_drop_xy_kernel(const DevConsts *__restrict__ dcy, const DevConsts *__restrict__ dcx,
                                                                  const DevConsts *__restrict__ dcl, u32 N, const u64 *__restrict__ x, size_t sx,
                                                                  size_t six, const u64 *__restrict__ y, size_t sy, size_t siy,
                                                                  u64 *__restrict__ out, u32 n_outer)
{
    if (blockIdx.y < 2 * n_outer)
        expand_body<true, true, LC, K, false, ExpandIn::drop, LY>(dcy, dcl, N, y, sy, siy, out, 4, 2, blockIdx.y);
    else
        expand_body<false, true, LC, K, false, ExpandIn::drop, LX>(dcx, dcl, N, x, sx, six, out, 4, 0, blockIdx.y - 2 * n_outer);
}
// the (L, Lc) pairs the fused kernel is built for: Lc = L - 1 for every L, and the further pairs that stay free of scratch; the
// (LY, LX, LC) triples of the chain schedule's form
#ifndef PIEHIP_CHAIN_DROP_FUSED
#define PIEHIP_CHAIN_DROP_FUSED 1
#endif
#define PIE_CHAIN_DROP_PAIRS(X_) X_(2, 1) X_(3, 2) X_(4, 3) X_(5, 4) X_(6, 5) X_(7, 6) X_(4, 2) X_(6, 4)
#define PIE_CHAIN_DROP_TRIPLES(X_) X_(4, 3, 2) X_(6, 5, 4) X_(6, 4, 3)
bool expand_drop_built(u32 Ly, u32 Lx, u32 Lc)
{
    if (!PIEHIP_CHAIN_DROP_FUSED) return false;
#define PAIR_(L_, C_) if (Ly == L_ && Lc == C_ && (Lx <= C_ || Lx == L_)) return true;
#define TRIPLE_(L_, X_, C_) if (Ly == L_ && Lx == X_ && Lc == C_) return true;
    PIE_CHAIN_DROP_PAIRS(PAIR_)
    PIE_CHAIN_DROP_TRIPLES(TRIPLE_)
#undef TRIPLE_
#undef PAIR_
    return false;
}

// Both conversions of a product (kernels.hpp): the kernel follows from how the two operands arrive
bool launch_expand_pair(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y, u32 n_outer, u64 *out,
                        hipStream_t st, Arith ar, bool fold)
{
    const bool ydrop = y.src_L > L, xdrop = x.src_L > L;
    const dim3 grid(((fold ? N / 2 : N) + TPB - 1) / TPB, n_outer * 4), block(TPB);
    if (ydrop) {   // fused limb drop: X is dropped too, or lies on this level with its Q limbs in place
        if (!fold || !ar.mad || x.plain || y.plain || x.q_ready == xdrop || !expand_drop_built(y.src_L, xdrop ? x.src_L : L, L)) return false;
        // the drop forms are built for the two column-accumulator kinds only (refused above for the other)
        auto with_colacc = [&](auto &&f) {
            with_arith(ar, [&](auto K_) {
                if constexpr (colacc(K_())) f(K_);
            });
        };
#define PAIR_(L_, C_)                                                                                                                          \
    if (y.src_L == L_ && L == C_ && (!xdrop || x.src_L == L_)) {   /* (an X on Y's limbs is under Y's constants) */                            \
        with_colacc([&](auto K_) {                                                                                                             \
            with_bools([&](auto XD_) {                                                                                                         \
                hipLaunchKernelGGL((expand_both_drop_kernel<L_, C_, XD_(), K_()>), grid, block, 0, st, y.src_dc, dc, N, x.p, x.row, x.poly,    \
                                   y.p, y.row, y.poly, out, n_outer);                                                                          \
            }, xdrop);                                                                                                                         \
        });                                                                                                                                    \
        return true;                                                                                                                           \
    }
#define TRIPLE_(L_, X_, C_)                                                                                                                    \
    if (y.src_L == L_ && x.src_L == X_ && L == C_) {                                                                                           \
        with_colacc([&](auto K_) {                                                                                                             \
            hipLaunchKernelGGL((expand_both_drop_xy_kernel<L_, X_, C_, K_()>), grid, block, 0, st, y.src_dc, x.src_dc, dc, N, x.p, x.row,      \
                               x.poly, y.p, y.row, y.poly, out, n_outer);                                                                      \
        });                                                                                                                                    \
        return true;                                                                                                                           \
    }
        PIE_CHAIN_DROP_PAIRS(PAIR_)
        PIE_CHAIN_DROP_TRIPLES(TRIPLE_)
#undef TRIPLE_
#undef PAIR_
        return false;
    }
    if (xdrop || x.plain != y.plain) return false;
    if (x.plain)   // (a level context has fewer limbs than MAX_L)
        return !x.q_ready && with_u32<1, 6>(L, [&](auto L_) {
            with_arith(ar, [&](auto K_) {
                with_bools([&](auto F_) {
                    hipLaunchKernelGGL((expand_both_plain_kernel<F_(), L_(), K_()>), grid, block, 0, st, dc, N, x.p, x.row, x.poly, y.p, y.row, y.poly,
                                       out, n_outer);
                }, fold);
            });
        });
    return x.poly == y.poly && with_u32<1, 7>(L, [&](auto L_) {
        with_arith(ar, [&](auto K_) {
            with_bools([&](auto F_, auto Q_) {
                hipLaunchKernelGGL((expand_both_kernel<F_(), L_(), K_(), Q_()>), grid, block, 0, st, dc, N, x.p, x.row, y.p, y.row, y.poly, out, n_outer);
            }, fold, x.q_ready);
        });
    });
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
