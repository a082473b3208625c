// kernels_stage_a.hip -- stage A of BatchedFHEHIPPIE::run() for gfx950: the fused ct x pt multiply-accumulate of a whole query (or a
// batch of queries) on one handle.  Streaming u64 modular arithmetic: one thread per coefficient, consecutive lanes on consecutive
// coefficients (coalesced 8-byte or 16-byte lanes), constants scalar-loaded from one DevConsts block.  Reference call sites:
// BatchedFHEHIPPIE.cpp:101-127.  The query-sliced form is kernels_slice.hip.
#include "pie_kernel_common.h"

namespace piehip {

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

}  // namespace piehip
