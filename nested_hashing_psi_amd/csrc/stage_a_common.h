// stage_a_common.h -- what the stage A kernels of kernels_stage_a.hip (the whole query on one handle) and kernels_slice.hip (one handle's
// (inner hash function, limb) units) share: the block -> tile map, the lane-ordered home of a coefficient, the instruction blocks of
// the epilogue (column accumulator -> residue, the sum with the minus word), the term loop of the tiled kernels (stage_a_terms:
// stage_a_tiled_kernel and stage_a_slice_kernel are a prologue and an epilogue around it), the multiply-add block of the
// resident kernel (colacc_mac2_cut) and, for the launchers, the rules that pick query groups, bin layers per thread, terms in flight
// and the resident or the tiled kernel (stage_a_query_group, stage_a_layers, stage_a_depth, stage_a_resident_lpp) and the one
// dispatch that turns them into template arguments (stage_a_for_groups).
#pragma once
#include <type_traits>

#include "kernels.hpp"
#include "madasm.h"

namespace piehip {

// fixed scratch registers of the instruction blocks here and in pie_arith.h ("constant-operand modular products")
#define PIE_ASM_CLOB "vcc", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71"

// Block -> (coefficient block, limb, inner hash function, group of bin layers).  The `groups` blocks of one tile read the same
// index-ciphertext words (and different database words): they should run on the same XCD, one after the other, so that all
// but the first take the index words from that XCD's L2.  Workgroups go to the eight XCDs round-robin by their linear id, so
// a one-dimensional grid is cut as id = 8 * slot + xcd, slot = tile_of_this_xcd * groups + group.  (With the layer group in
// blockIdx.z the blocks of a tile were `tiles` apart in dispatch order: every group fetched the index matrix from HBM again.)
struct StageATile {
    u32 bx, l, hz, grp;
};
__device__ __forceinline__ bool stage_a_tile(u32 nx, u32 L, u32 tiles, u32 groups, StageATile &t)
{
    const u32 id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    t.grp = slot % groups;
    const u32 tile = (slot / groups) * 8 + xcd;
    if (tile >= tiles) return false;
    t.bx = tile % nx;
    t.l = (tile / nx) % L;
    t.hz = tile / (nx * L);
    return true;
}
static dim3 stage_a_grid(u32 nx, u32 L, u32 hn, u32 groups) { return dim3(8 * ((nx * L * hn + 7) / 8) * groups); }

// Lane-ordered home of coefficient n of a limb (ntt16_kernel.h: slices of 2^logns coefficients, T = 2^logns / 16 threads, thread tau
// holds elements 16 tau .. 16 tau + 15 and stores pair j at 2 (T j + tau)): the offset inside the limb
__device__ __forceinline__ u32 lane_home(u32 n, u32 logns)
{
    const u32 ns = 1u << logns, e = n & (ns - 1);
    return (n & ~(ns - 1)) + 2 * ((ns >> 4) * ((e >> 1) & 7) + (e >> 4)) + (e & 1);
}

// a + b mod q for canonical a, b and q < 2^62, without the compare / select pair hipcc makes of addmod(): v_cndmask_b32 on VCC
// issues at a sixth of the rate of the other vector instructions here (profiles/r03/microbench_operands.txt: 23.7 cycles per
// wave against 4.2), and the epilogue of stage A has 24 of these sums per thread
__device__ __forceinline__ u64 addmod_nb(u64 a, u64 b, u64 q)
{
    // (as an instruction block: written in C the compiler turns the mask back into a compare and a select)
    const u64 s = a + b;
    u32 lo, hi;
    asm("v_lshl_add_u64 v[60:61], %[x], 0, %[nm]\n\t"  // s - q: negative iff s < q
        "v_ashrrev_i32 v62, 31, v61\n\t"
        "v_bfi_b32 %[lo], v62, %[xl], v60\n\t"
        "v_bfi_b32 %[hi], v62, %[xh], v61"
        : [lo] "=&v"(lo), [hi] "=&v"(hi)
        : [x] "v"(s), [xl] "v"((u32)s), [xh] "v"((u32)(s >> 32)), [nm] "s"(0 - q)
        : "v62", "v60", "v61");
    return ((u64)hi << 32) | lo;
}

// Column accumulator -> residue in one block (2^59 < q < 2^60).  The columns are carry-normalised (c1' = c1 + (c0 >> 30),
// c2' = c2 + (c1' >> 30)), after which z >> 59 = (c2' << 1) | bit 29 of c1' and the low word of z is three disjoint bit fields;
// one-word Barrett as reduce123 / reduce124 of modarith.h (same quotient estimate, same remainder), mulhi as mulhi_sb, the
// remainder z + qhat (2^64 - q) on one v_mad_u64_u32 chain, sign-mask subtractions.  32 instructions (35 with W124) where the
// compiler's colacc_value + reduce123 take ~65 (128-bit additions through v_cmp / v_cndmask carries, an 11-instruction mulhi).
// W124: z < 2^124 (eight products), otherwise z < 2^123 (seven).  (The estimate is at most 2 short, so the "4q" of the names
// below is really 3q, and the remainder of the W124 form is below 6q: modarith.h.)
// a three-column accumulator below 2^123 to v[66:67] in [0, 4q) (v60-v71, vcc, s[96:97] as scratch): the body of colacc_reduce<false>
#define PIE_COLACC123_TO_4Q \
    "v_lshrrev_b64 v[60:61], 30, %[c0]\n\t" \
    "v_lshl_add_u64 v[60:61], v[60:61], 0, %[c1]\n\t" \
    "v_lshrrev_b64 v[62:63], 30, v[60:61]\n\t" \
    "v_lshl_add_u64 v[62:63], v[62:63], 0, %[c2]\n\t" \
    "v_lshlrev_b64 v[64:65], 1, v[62:63]\n\t" \
    "v_bfe_u32 v68, v60, 29, 1\n\t" \
    "v_and_b32 v66, 0x3fffffff, %[c0l]\n\t" \
    "v_bfe_u32 v67, v60, 2, 28\n\t" \
    "v_or_b32 v64, v64, v68\n\t" \
    "v_lshl_or_b32 v66, v60, 30, v66\n\t" \
    "v_lshl_or_b32 v67, v62, 28, v67\n\t" \
    "v_mul_hi_u32 v68, v64, %[mul]\n\t" \
    "v_mov_b32 v69, 0\n\t" \
    "v_mad_u64_u32 v[68:69], vcc, v64, %[muh], v[68:69]\n\t" \
    "v_mad_u64_u32 v[68:69], vcc, v65, %[mul], v[68:69]\n\t" \
    "v_mad_u64_u32 v[70:71], s[96:97], v65, %[muh], 0\n\t" \
    "v_lshrrev_b64 v[68:69], 32, v[68:69]\n\t" \
    "v_addc_co_u32 v69, vcc, 0, v69, vcc\n\t" \
    "v_lshl_add_u64 v[68:69], v[70:71], 0, v[68:69]\n\t" \
    "v_mad_u64_u32 v[70:71], vcc, v68, %[nqh], 0\n\t" \
    "v_mad_u64_u32 v[70:71], vcc, v69, %[nql], v[70:71]\n\t" \
    "v_add_u32 v67, v67, v70\n\t" \
    "v_mad_u64_u32 v[66:67], vcc, v68, %[nql], v[66:67]\n\t"
// ... left there: [0, 4q).  For values that go on into a folded forward transform (fold_store adds a [0, 4q) product to them and the
// transform takes anything below 8q) or into a Shoup product (any operand below 2^63): eight instructions less than the canonical form
__device__ __forceinline__ u64 colacc_reduce123_lazy(const ColAcc &a, const Mod &m, u64 nq)
{
    const u64 mu = (m.r1 << 59) | (m.r0 >> 5);   // floor(2^123 / q)
    u64 r;
    asm(PIE_COLACC123_TO_4Q
        "v_lshl_add_u64 %[r], v[66:67], 0, 0"
        : [r] "=v"(r)
        : [c0] "v"(a.c0), [c1] "v"(a.c1), [c2] "v"(a.c2), [c0l] "v"((u32)a.c0), [mul] "s"((u32)mu), [muh] "s"((u32)(mu >> 32)),
          [nql] "s"((u32)nq), [nqh] "s"((u32)(nq >> 32))
        : PIE_ASM_CLOB, "s96", "s97");
    return r;
}
template <bool W124>
__device__ __forceinline__ u64 colacc_reduce(const ColAcc &a, const Mod &m, u64 nq)
{
    const u64 mu = (m.r1 << 59) | (m.r0 >> 5);   // floor(2^123 / q)
    const u64 n2q = 2 * nq, n4q = 4 * nq;
    u64 r;
    if (!W124) {
        asm(PIE_COLACC123_TO_4Q
            "v_lshl_add_u64 v[60:61], v[66:67], 0, %[n2q]\n\t"
            "v_ashrrev_i32 v62, 31, v61\n\t"
            "v_bfi_b32 v66, v62, v66, v60\n\t"
            "v_bfi_b32 v67, v62, v67, v61\n\t"
            "v_lshl_add_u64 v[60:61], v[66:67], 0, %[n1q]\n\t"
            "v_ashrrev_i32 v62, 31, v61\n\t"
            "v_and_b32 v64, %[ql], v62\n\t"
            "v_and_b32 v65, %[qh], v62\n\t"
            "v_lshl_add_u64 %[r], v[60:61], 0, v[64:65]"
            : [r] "=v"(r)
            : [c0] "v"(a.c0), [c1] "v"(a.c1), [c2] "v"(a.c2), [c0l] "v"((u32)a.c0), [mul] "s"((u32)mu), [muh] "s"((u32)(mu >> 32)),
              [nql] "s"((u32)nq), [nqh] "s"((u32)(nq >> 32)), [n2q] "s"(n2q), [n1q] "s"(nq), [ql] "s"((u32)m.q), [qh] "s"((u32)(m.q >> 32))
            : PIE_ASM_CLOB, "s96", "s97");
    } else {
        // z >> 60 = c2' after the normalisation; qhat = 2 floor(zh mu / 2^64); remainder in [0, 6q): one more subtraction
        asm("v_lshrrev_b64 v[60:61], 30, %[c0]\n\t"
            "v_lshl_add_u64 v[60:61], v[60:61], 0, %[c1]\n\t"
            "v_lshrrev_b64 v[64:65], 30, v[60:61]\n\t"
            "v_lshl_add_u64 v[64:65], v[64:65], 0, %[c2]\n\t"
            "v_and_b32 v66, 0x3fffffff, %[c0l]\n\t"
            "v_bfe_u32 v67, v60, 2, 28\n\t"
            "v_lshl_or_b32 v66, v60, 30, v66\n\t"
            "v_lshl_or_b32 v67, v64, 28, v67\n\t"
            "v_mul_hi_u32 v68, v64, %[mul]\n\t"
            "v_mov_b32 v69, 0\n\t"
            "v_mad_u64_u32 v[68:69], vcc, v64, %[muh], v[68:69]\n\t"
            "v_mad_u64_u32 v[68:69], vcc, v65, %[mul], v[68:69]\n\t"
            "v_mad_u64_u32 v[70:71], s[96:97], v65, %[muh], 0\n\t"
            "v_lshrrev_b64 v[68:69], 32, v[68:69]\n\t"
            "v_addc_co_u32 v69, vcc, 0, v69, vcc\n\t"
            "v_lshl_add_u64 v[68:69], v[70:71], 0, v[68:69]\n\t"
            "v_lshlrev_b64 v[68:69], 1, v[68:69]\n\t"
            "v_mad_u64_u32 v[70:71], vcc, v68, %[nqh], 0\n\t"
            "v_mad_u64_u32 v[70:71], vcc, v69, %[nql], v[70:71]\n\t"
            "v_add_u32 v67, v67, v70\n\t"
            "v_mad_u64_u32 v[66:67], vcc, v68, %[nql], v[66:67]\n\t"
            "v_lshl_add_u64 v[60:61], v[66:67], 0, %[n4q]\n\t"
            "v_ashrrev_i32 v62, 31, v61\n\t"
            "v_bfi_b32 v66, v62, v66, v60\n\t"
            "v_bfi_b32 v67, v62, v67, v61\n\t"
            "v_lshl_add_u64 v[60:61], v[66:67], 0, %[n2q]\n\t"
            "v_ashrrev_i32 v62, 31, v61\n\t"
            "v_bfi_b32 v66, v62, v66, v60\n\t"
            "v_bfi_b32 v67, v62, v67, v61\n\t"
            "v_lshl_add_u64 v[60:61], v[66:67], 0, %[n1q]\n\t"
            "v_ashrrev_i32 v62, 31, v61\n\t"
            "v_and_b32 v64, %[ql], v62\n\t"
            "v_and_b32 v65, %[qh], v62\n\t"
            "v_lshl_add_u64 %[r], v[60:61], 0, v[64:65]"
            : [r] "=v"(r)
            : [c0] "v"(a.c0), [c1] "v"(a.c1), [c2] "v"(a.c2), [c0l] "v"((u32)a.c0), [mul] "s"((u32)mu), [muh] "s"((u32)(mu >> 32)),
              [nql] "s"((u32)nq), [nqh] "s"((u32)(nq >> 32)), [n4q] "s"(n4q), [n2q] "s"(n2q), [n1q] "s"(nq), [ql] "s"((u32)m.q),
              [qh] "s"((u32)(m.q >> 32))
            : PIE_ASM_CLOB, "s96", "s97");
    }
    return r;
}

// The same reduction for a modulus q = 2^60 - d with d small (the default chains: the largest primes below 2^60 that are 1 mod 2N),
// without a quotient estimate: 2^60 = d (mod q), so the part of z above bit 60 folds into the low 60 bits by multiplications
// with d.  d is the low word of 2^64 - q (the high word is 0xf0000000).  With the columns carry-normalised as above,
//   z = lo60 + n2 2^60,  lo60 = z mod 2^60 (two words),  n2 = z >> 60 = c2' (two words n2l, n2h)
//   t = n2l d + lo60                                       one v_mad_u64_u32
//   u = n2h d                                              one more; n2 d = n2l d + u 2^32
//   u 2^32 = (u >> 28) 2^60 + (u mod 2^28) 2^32  =  (u >> 28) d + (u mod 2^28) 2^32  (mod q)
//   r = t + (u mod 2^28) 2^32 + (u >> 28) d                a 32-bit add into t's high word, the third v_mad_u64_u32
// Bounds for z < 2^B and d < 2^k:  t < 2^60 + 2^(32+k);  u < 2^(B-92+k);  t's high word < 2^28 + 2^k and u mod 2^28 < 2^28: the
// 32-bit add does not carry for k <= 30;  u >> 28 < 2^(B-120+k) fits one word;  (u >> 28) d < 2^(B-120+2k);
//   r < 2^60 + 2^(32+k) + 2^60 + 2^(B-120+2k)
//   B = 123 (seven products), k = 28:  r < 2^61 + 2^60 + 2^59 = 3.5 2^60 < 4q   (k = 29: 2^62, not below 4q)
//   B = 124 (eight products), k = 27:  r < 2^61 + 2^59 + 2^58 = 2.75 2^60 < 3q  (k = 28: 2^62)
// so ONE block serves both widths for d < 2^27 = COLACC_FOLD_MAX_D (kernels.hpp), the bound a context is selected by (NttPlan::fold_moduli), and
// leaves less than 3q as the Barrett block does.  Nothing reads VCC: no wait states.  13 instructions, 3 of them multiplier
// operations (the Barrett block: 23 and 7); no mu.  v60-v69 and vcc as scratch.
#define PIE_COLACC_FOLD_HEAD \
    "v_lshrrev_b64 v[60:61], 30, %[c0]\n\t" \
    "v_lshl_add_u64 v[60:61], v[60:61], 0, %[c1]\n\t" \
    "v_lshrrev_b64 v[62:63], 30, v[60:61]\n\t" \
    "v_lshl_add_u64 v[62:63], v[62:63], 0, %[c2]\n\t" \
    "v_and_b32 v66, 0x3fffffff, %[c0l]\n\t" \
    "v_bfe_u32 v67, v60, 2, 28\n\t" \
    "v_mad_u64_u32 v[64:65], vcc, v63, %[d], 0\n\t" \
    "v_lshl_or_b32 v66, v60, 30, v66\n\t" \
    "v_mad_u64_u32 v[66:67], vcc, v62, %[d], v[66:67]\n\t" \
    "v_and_b32 v68, 0xfffffff, v64\n\t" \
    "v_alignbit_b32 v69, v65, v64, 28\n\t" \
    "v_add_u32 v67, v67, v68\n\t"
// ... and the third product, into the result (lazy) or into v[66:67] (CANON).  CANON: one more fold, r' = (r mod 2^60) + (r >> 60) d
// with r >> 60 <= 2, so r' < 2^60 + 2d = q + 3d < 2q, and one sign-mask subtraction: 20 instructions (the Barrett forms: 32 and 35)
template <bool CANON>
__device__ __forceinline__ u64 colacc_fold(const ColAcc &a, u64 nq)
{
    if (!CANON) {
        u64 r;
        asm(PIE_COLACC_FOLD_HEAD
            "v_mad_u64_u32 %[r], vcc, v69, %[d], v[66:67]"
            : [r] "=v"(r)
            : [c0] "v"(a.c0), [c1] "v"(a.c1), [c2] "v"(a.c2), [c0l] "v"((u32)a.c0), [d] "s"((u32)nq)
            : PIE_ASM_CLOB);
        return r;
    }
    u32 lo, hi;
    asm(PIE_COLACC_FOLD_HEAD
        "v_mad_u64_u32 v[66:67], vcc, v69, %[d], v[66:67]\n\t"
        "v_lshrrev_b32 v68, 28, v67\n\t"
        "v_and_b32 v67, 0xfffffff, v67\n\t"
        "v_mad_u64_u32 v[66:67], vcc, v68, %[d], v[66:67]\n\t"
        "v_lshl_add_u64 v[60:61], v[66:67], 0, %[n1q]\n\t"
        "v_ashrrev_i32 v62, 31, v61\n\t"
        "v_bfi_b32 %[lo], v62, v66, v60\n\t"
        "v_bfi_b32 %[hi], v62, v67, v61"
        : [lo] "=v"(lo), [hi] "=v"(hi)
        : [c0] "v"(a.c0), [c1] "v"(a.c1), [c2] "v"(a.c2), [c0l] "v"((u32)a.c0), [d] "s"((u32)nq), [n1q] "s"(nq)
        : PIE_ASM_CLOB);
    return ((u64)hi << 32) | lo;
}
// the reduction of the two column-accumulator kinds: FD (ArithKind::fold) the folded block, otherwise (ArithKind::barrett) the Barrett block
template <bool FD, bool W124>
__device__ __forceinline__ u64 colacc_red(const ColAcc &a, const Mod &m, u64 nq)
{
    if constexpr (FD) return colacc_fold<true>(a, nq);
    else return colacc_reduce<W124>(a, m, nq);
}
template <bool FD>
__device__ __forceinline__ u64 colacc_red_lazy(const ColAcc &a, const Mod &m, u64 nq)
{
    if constexpr (FD) return colacc_fold<false>(a, nq);
    else return colacc_reduce123_lazy(a, m, nq);
}

// ---------------------------------------------------------------------------------------------
// The term loop of the tiled stage A kernels: a[q][t][c] = sum_j idx_q[j][c] * db[layer t][j] for the thread's coefficient, Q queries
// and BPT bin layers.  A database word is loaded once for the Q queries, an index word once per BPT layers, DEPTH terms are in flight
// behind the one being accumulated.
// MAD: every modulus in (2^59, 2^60) -- carry-free 30-bit column accumulators (madasm.h), swept every COLACC_MAX_TERMS terms and
// reduced every COLACC_MAX_TOTAL; otherwise (moduli up to 61 bits) 128-bit accumulators reduced every 32 terms, as stage_a_kernel.
// ---------------------------------------------------------------------------------------------
template <bool MAD>
struct StageAAcc;
template <>
struct StageAAcc<true> {
    ColAcc v;
    __device__ __forceinline__ void zero() { v = ColAcc{0, 0, 0}; }
};
template <>
struct StageAAcc<false> {
    U128 v;
    __device__ __forceinline__ void zero() { v = U128{0, 0}; }
};

// qs.idx[q] + ioff and pd are the uniform stream bases of the thread's block, nl its lane offset.  cs is the component stride of an
// index ciphertext (a term is 2 cs further) and the term stride of the database (a bin layer is bin_stride further): L N where the
// arrays hold whole ciphertexts, N over one-limb units.  The group holds layers 0 .. tmax <= BPT - 1.  Runs all E terms from zero
// and leaves the sums in `out` for the kernel's epilogue, unswept and unreduced since the last period boundary before E.
template <int BPT, int Q, int DEPTH, bool MAD, class S>
__device__ __forceinline__ void stage_a_terms(const StageAQueries &qs, size_t ioff, S cs, const u64 *pd, size_t bin_stride, u32 tmax, u32 nl,
                                              u32 E, const Mod &m, StageAAcc<MAD> (&out)[Q][BPT][2])
{
    // (accumulated in an array of its own and handed over after the last term: with the loop working on the caller's array, the
    // 128-bit form of three layers x four queries took 306 registers instead of 235 and lost its second wave per SIMD, four layers x
    // two queries 404 instead of 288; the column-accumulator forms compile the same either way -- profiles/stage_a_shared)
    StageAAcc<MAD> a[Q][BPT][2];
#pragma unroll
    for (int q = 0; q < Q; q++)
#pragma unroll
        for (int t = 0; t < BPT; t++) a[q][t][0].zero(), a[q][t][1].zero();
    auto load_term = [&](u32 j, u64 (&vi)[Q][2], u64 (&vd)[BPT]) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const u64 *pij = qs.idx[q] + ioff + (size_t)j * 2 * cs;
            vi[q][0] = pij[nl];
            vi[q][1] = (pij + cs)[nl];
        }
        const u64 *pdj = pd + (size_t)j * cs;
#pragma unroll
        // The last group of a launch may hold fewer than BPT layers (b no multiple of BPT): its missing layers repeat its last one --
        // the same loads again (L1 hits) and multiply-adds nobody stores -- so that the term loop stays free of per-layer branches
        // (skipping them under uniform branches instead was measured: 4-17 % slower, profiles/r05/stage_a_batch_layer_groups.txt).
        // The database is read once per run: non-temporal (see stage_a_mad_kernel).
        for (int t = 0; t < BPT; t++) vd[t] = __builtin_nontemporal_load(pdj + (size_t)min((u32)t, tmax) * bin_stride + nl);
    };
    // a ring of DEPTH term buffers; the term loop is unrolled DEPTH times so that the ring needs no register moves
    u64 qiv[DEPTH][Q][2], qdv[DEPTH][BPT];
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if ((u32)d < E) load_term(d, qiv[d], qdv[d]);
    auto term = [&](u32 j, u64 (&vi)[Q][2], u64 (&vd)[BPT]) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            if constexpr (MAD) {
                const Split30 i0 = split30(vi[q][0]), i1 = split30(vi[q][1]);
#pragma unroll
                for (int t = 0; t < BPT; t++) colacc_mac2(a[q][t][0].v, a[q][t][1].v, i0, i1, vd[t]);
            } else {
#pragma unroll
                for (int t = 0; t < BPT; t++) mac128(a[q][t][0].v, vi[q][0], vd[t]), mac128(a[q][t][1].v, vi[q][1], vd[t]);
            }
        }
        if (j + DEPTH < E) load_term(j + DEPTH, vi, vd);   // refill this ring slot (the other slots are in flight)
        if constexpr (MAD) {
            if ((j % COLACC_MAX_TERMS) == COLACC_MAX_TERMS - 1 && j + 1 < E) {   // more terms follow: make room in the low columns
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int t = 0; t < BPT; t++) colacc_carry(a[q][t][0].v), colacc_carry(a[q][t][1].v);
            }
            if ((j % COLACC_MAX_TOTAL) == COLACC_MAX_TOTAL - 1 && j + 1 < E) {   // the top column is full: reduce and start over
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int t = 0; t < BPT; t++)
#pragma unroll
                        for (int c = 0; c < 2; c++) {
                            const u64 r = colacc_reduce<true>(a[q][t][c].v, m, 0 - m.q);  // (the instruction block of the epilogue: no compare / select pairs)
                            a[q][t][c].v = ColAcc{r & 0x3FFFFFFFull, r >> 30, 0};
                        }
            }
        } else {
            if ((j & 31) == 31) {   // 2^61 + 32 * 2^122 < 2^128
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int t = 0; t < BPT; t++)
#pragma unroll
                        for (int c = 0; c < 2; c++) a[q][t][c].v = U128{reduce128(a[q][t][c].v, m), 0};
            }
        }
    };
    for (u32 j = 0; j < E; j += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (j + d < E) term(j + d, qiv[d], qdv[d]);
    }
#pragma unroll
    for (int q = 0; q < Q; q++)
#pragma unroll
        for (int t = 0; t < BPT; t++) out[q][t][0] = a[q][t][0], out[q][t][1] = a[q][t][1];
}

// ---------------------------------------------------------------------------------------------
// Pieces of the resident kernel (stage_a_resident_kernel of kernels_stage_a.hip): the other loop order.  The thread keeps the index
// words of its coefficient in registers, already cut into 30-bit halves, and the database words of the launch's layers stream
// past them -- so a database word arrives once for the Q queries and is cut once, not once per query as in colacc_mac2.
// ---------------------------------------------------------------------------------------------
// colacc_mac2 on a database word that is already cut (dl, dh).  FIRST: the term that opens a layer's sum -- the accumulators
// are written, not read, so the layer needs no zeroing moves.
// (between the terms: keeps each refill where it is written, at the top of its term, and the multiply-adds of a term together)
#define PIE_STAGE_A_FENCE() __builtin_amdgcn_sched_barrier(0)
template <bool FIRST>
__device__ __forceinline__ void colacc_mac2_cut(ColAcc &a, ColAcc &b, Split30 x0, Split30 x1, u32 dl, u32 dh)
{
    if (FIRST) {
        asm("v_mad_u64_u32 %[a0], vcc, %[x0l], %[dl], 0\n\t"
            "v_mad_u64_u32 %[a1], vcc, %[x0l], %[dh], 0\n\t"
            "v_mad_u64_u32 %[b0], vcc, %[x1l], %[dl], 0\n\t"
            "v_mad_u64_u32 %[b1], vcc, %[x1l], %[dh], 0\n\t"
            "v_mad_u64_u32 %[a2], vcc, %[x0h], %[dh], 0\n\t"
            "v_mad_u64_u32 %[b2], vcc, %[x1h], %[dh], 0\n\t"
            "v_mad_u64_u32 %[a1], vcc, %[x0h], %[dl], %[a1]\n\t"
            "v_mad_u64_u32 %[b1], vcc, %[x1h], %[dl], %[b1]\n\t"
            : [a0] "=&v"(a.c0), [a1] "=&v"(a.c1), [a2] "=&v"(a.c2), [b0] "=&v"(b.c0), [b1] "=&v"(b.c1), [b2] "=&v"(b.c2)
            : [dl] "v"(dl), [dh] "v"(dh), [x0l] "v"(x0.lo), [x0h] "v"(x0.hi), [x1l] "v"(x1.lo), [x1h] "v"(x1.hi)
            : "vcc");
    } else {
        asm("v_mad_u64_u32 %[a0], vcc, %[x0l], %[dl], %[a0]\n\t"
            "v_mad_u64_u32 %[a1], vcc, %[x0l], %[dh], %[a1]\n\t"
            "v_mad_u64_u32 %[b0], vcc, %[x1l], %[dl], %[b0]\n\t"
            "v_mad_u64_u32 %[b1], vcc, %[x1l], %[dh], %[b1]\n\t"
            "v_mad_u64_u32 %[a2], vcc, %[x0h], %[dh], %[a2]\n\t"
            "v_mad_u64_u32 %[b2], vcc, %[x1h], %[dh], %[b2]\n\t"
            "v_mad_u64_u32 %[a1], vcc, %[x0h], %[dl], %[a1]\n\t"
            "v_mad_u64_u32 %[b1], vcc, %[x1h], %[dl], %[b1]\n\t"
            : [a0] "+v"(a.c0), [a1] "+v"(a.c1), [a2] "+v"(a.c2), [b0] "+v"(b.c0), [b1] "+v"(b.c1), [b2] "+v"(b.c2)
            : [dl] "v"(dl), [dh] "v"(dh), [x0l] "v"(x0.lo), [x0h] "v"(x0.hi), [x1l] "v"(x1.lo), [x1h] "v"(x1.hi)
            : "vcc");
    }
}

// ---------------------------------------------------------------------------------------------
// Launch rules of the tiled kernels (launch_stage_a_batch, launch_stage_a_slice).
// ---------------------------------------------------------------------------------------------
// A run-time value as a template argument: with_u32<LO, HI>(v, f) calls f(std::integral_constant<u32, v>) for v in [LO, HI] and says
// whether it did.  The callers' generic lambdas read the argument as a constant (L_()).
template <u32 LO, u32 HI, class F>
static bool with_u32(u32 v, F &&f)
{
    if constexpr (LO <= HI) {
        if (v != LO) return with_u32<LO + 1, HI>(v, f);
        f(std::integral_constant<u32, LO>{});
        return true;
    }
    return false;
}

// Queries of the next launch, given the queries left: groups of four, three or two (five: 3 + 2; six: 3 + 3; seven: 4 + 3); a single
// one alone.
constexpr u32 stage_a_query_group(u32 left) { return left == 5 || left == 6 ? 3 : left < 4 ? left : 4; }
static_assert(stage_a_query_group(5) == 3 && stage_a_query_group(5 - 3) == 2, "five queries: 3 + 2");
static_assert(stage_a_query_group(7) == 4 && stage_a_query_group(7 - 4) == 3, "seven queries: 4 + 3");

// Bin layers per thread.  What bounds the kernel is the traffic through the L1s (profiles/r05/stage_a_batch_prefetch_really_in_flight.txt:
// ~8.6 TB/s of L1 misses chip-wide, three quarters of them index words that a thread re-reads from the L2 once per GROUP of layers), so
// groups should be as large as the registers allow: seven layers for one query (stage_a_mad_kernel's; the 128-bit accumulators of
// one query spill beyond five), four for two queries, three for three queries (164 VGPRs either way: three waves per SIMD), three
// for four (208: two waves -- still 4 % ahead of two layers).  r03-r04 had two layers for three queries: 81.7 us for twelve layers
// against 69.9 with groups of three (tools/microbench_stage_a_batch.hip, r05).
constexpr u32 stage_a_layer_cap(u32 Q, bool mad) { return Q == 1 ? (mad ? 7 : 5) : Q == 2 ? 4 : 3; }
// ONE launch whatever the layer count: the last group is ragged (stage_a_terms) -- a remainder launch of one or two layers is all
// latency (25 us for two layers alone), and two launches of half the groups each leave the chip a partial round of waves twice.  So:
// the group size that issues the fewest loads per term over the launch, ceil(b / g) groups of 2 Q index words + g database words (a
// ragged last group loads and multiplies its padding too: six layers of two queries are better off as 3 + 3 than as 4 + 2).
constexpr u32 stage_a_layers(u32 Q, u32 b, u32 cap)
{
    u32 bpt = 1, best = ~0u;
    for (u32 g = 1; g <= cap && g <= b; g++) {
        const u32 loads = ((b + g - 1) / g) * (2 * Q + g);
        if (loads <= best) best = loads, bpt = g;
    }
    return bpt;
}
static_assert(stage_a_layers(2, 6, stage_a_layer_cap(2, true)) == 3, "six layers of two queries: 3 + 3");
static_assert(stage_a_layers(3, 12, stage_a_layer_cap(3, true)) == 3, "twelve layers of three queries: groups of three");

// Terms in flight behind the one being accumulated (profiles/r03/stage_a_batch_microbench.txt; r05: two for the wide tilings).  One
// query: stage_a_mad_kernel's four, and three with seven layers (176 registers with four, 168 are the most that leave three waves
// per SIMD).
constexpr int stage_a_depth(int Q, int BPT) { return Q == 1 ? (BPT == 7 ? 3 : 4) : (Q == 4 || Q * BPT >= 9) ? 2 : 3; }

// The rules as ONE dispatch: walks the query groups of a batch and calls f(Q, BPT, DEPTH, sub, q0) per group -- queries per thread,
// layers per thread and terms in flight as std::integral_constant<u32, ...>, the group's queries and the index of its first one.
template <bool MAD, class F>
static void stage_a_for_groups(const StageAQueries &qs, u32 nq, u32 b, F &&f)
{
    for (u32 q0 = 0, g; q0 < nq; q0 += g) {
        g = stage_a_query_group(nq - q0);
        StageAQueries sub = {};
        for (u32 q = 0; q < g; q++) sub.idx[q] = qs.idx[q0 + q], sub.minus[q] = qs.minus[q0 + q];
        with_u32<1, 4>(g, [&](auto Q_) {
            constexpr u32 Q = Q_(), cap = stage_a_layer_cap(Q, MAD);
            with_u32<1, cap>(stage_a_layers(Q, b, cap), [&](auto B_) {
                f(Q_, B_, std::integral_constant<u32, (u32)stage_a_depth((int)Q, (int)B_())>{}, sub, q0);
            });
        });
    }
}

// The resident kernel (stage_a_resident_kernel) or the tiled one, for a launch of Q queries over b layers with `threads` = N L hn
// coefficients.  -DPIEHIP_STAGE_A_RESIDENT=0 keeps every launch on the tiled kernel (A/B builds).
#ifndef PIEHIP_STAGE_A_RESIDENT
#define PIEHIP_STAGE_A_RESIDENT 1
#endif
// Words in the database ring of the instantiation for E, 0 where there is none: E = 14 (C3) and E = 12 (C2) are built, every other
// E stays on the tiled kernel (4 Q E index registers: Q = 3, E = 14 is the cap, and Q = 4 does not fit at any E worth having).
constexpr int stage_a_resident_ring(u32 E) { return E == 14 ? 7 : E == 12 ? 6 : 0; }
// Layers per partition of the resident launch, 0 = the tiled kernel.  From tools/microbench_stage_a_batch.hip
// (profiles/stage_a_resident/microbench.txt), resident against the tiling it replaces:
//   131 072 threads (C3's ring, two waves on every SIMD): 14 layers 65.7 us against 82.0, 8 layers 46.3 / 52.6, 6 layers 39.4 / 40.6,
//   5 layers 35.8 / 40.0, 4 layers 32.4 / 34.1;
//   49 152 threads (C2's ring, E = 12: three quarters of ONE wave per SIMD): 33.1 us against 28.7, and 30.5 / 32.8 in partitions of
//   6 / 4 layers -- two waves of 250 registers hide less latency than the tiled kernel's three, and there are not enough of them.
// So: at least STAGE_A_RESIDENT_MIN_THREADS coefficients, one wave of 64 on each of the chip's 1024 SIMDs (nothing between the two
// rings was measured), and no partitions -- halving the layer range cost 2.7-7 us at every layer count of C3's ring (each partition
// loads the index words again).  A launch of one tiled layer group (b <= 3) reads its index words once there too and keeps three
// waves per SIMD.
constexpr u64 STAGE_A_RESIDENT_MIN_THREADS = 65536;
constexpr u32 stage_a_resident_lpp(u32 Q, u32 E, u32 b, u64 threads)
{
    if (!PIEHIP_STAGE_A_RESIDENT || Q != 3 || !stage_a_resident_ring(E) || b <= stage_a_layer_cap(3, true)) return 0;
    return threads >= STAGE_A_RESIDENT_MIN_THREADS ? b : 0;
}
#if PIEHIP_STAGE_A_RESIDENT
static_assert(stage_a_resident_lpp(3, 14, 14, 16384 * 4 * 2) == 14 && stage_a_resident_lpp(3, 14, 8, 16384 * 4 * 2) == 8 &&
                  stage_a_resident_lpp(3, 14, 6, 16384 * 4 * 2) == 6,
              "C3, three queries: resident on one queue (14 layers) and on two (8 + 6), one partition each");
#endif
static_assert(stage_a_resident_lpp(3, 15, 14, 16384 * 4 * 2) == 0 && stage_a_resident_lpp(4, 14, 14, 16384 * 4 * 2) == 0 &&
                  stage_a_resident_lpp(3, 14, 3, 16384 * 4 * 2) == 0 && stage_a_resident_lpp(2, 14, 14, 16384 * 4 * 2) == 0,
              "E = 15, four or two queries and a launch of one layer group stay on the tiled kernel");
static_assert(stage_a_resident_lpp(3, 12, 12, 8192 * 3 * 2) == 0, "C2 stays on the tiled kernel (under one wave per SIMD)");
}  // namespace piehip
