// stage_a_common.h -- device helpers shared by the stage A kernels of kernels_pie.hip (the whole query on one handle) and
// kernels_slice.hip (one handle's (inner hash function, limb) units): the block -> tile map, the lane-ordered home of a coefficient,
// and the instruction blocks of the epilogue (column accumulator -> residue, the sum with the minus word).  Moved here word for word:
// the kernels of kernels_pie.hip compile to the same instructions as before.
#pragma once
#include "kernels.hpp"
#include "madasm.h"

namespace piehip {

// fixed scratch registers of the instruction blocks here and in kernels_pie.hip ("constant-operand modular products")
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
}  // namespace piehip
