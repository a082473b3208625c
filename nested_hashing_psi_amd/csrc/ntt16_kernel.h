// ntt16_kernel.h -- negacyclic NTT of 2^13-coefficient slices, 16 coefficients per thread (device code, gfx950).
//
// The 60-bit Shoup butterfly is bound by the integer ALU (~100 SIMD cycles per wave64 butterfly), and a
// wave of a transform spends 40-50 % of its life parked at LDS hand-offs, barriers and twiddle loads.  A SIMD issues one VALU
// instruction every 2 cycles only when at least two of its waves have one ready, so two waves per SIMD (all that 32
// coefficients per thread leave room for: the LDS image of a slice is 8 bytes per coefficient) keep it about half busy.
// This kernel halves the per-thread footprint: 512 threads (8 waves) per slice, two slices per CU = 4 waves per SIMD.
//
// Forward (Cooley-Tukey, natural order in, bit-reversed out), stage s pairs elements that differ in bit 12 - s:
//   pass 1  stages 0-2   thread tau holds rows r (stride 1024) of the column pair (2 tau, 2 tau + 1): loaded straight from
//                        HBM with 16-byte lanes; twiddles depend on r only -> scalar loads
//   -- LDS transpose, the only workgroup barrier pair of a slice --
//   pass 2  stages 3-6   wave w, lane l holds e = 1024 w + 64 k + l: twiddles depend on (w, k) only -> scalar loads
//   -- LDS hand-off inside the wave (a wave's pass-2 elements are its pass-3 and pass-4 elements) --
//   pass 3  stages 7-10  lane (a, c) holds e = 1024 w + 64 a + 4 k + c; per-lane twiddles from a kernel-ordered table
//   -- LDS hand-off inside the wave --
//   pass 4  stages 11-12 lane l holds the 16 contiguous coefficients e = 1024 w + 16 l + k
// Inverse (Gentleman-Sande) is the mirror image.  HBM traffic: one coalesced read and one coalesced write of the slice.
// LDS image: element e at e + 2 (e >> 5) (16 bytes of padding per 256): every access pattern above is conflict-free.
//
// Lane order.  The evaluation side ends (forward) / starts (inverse) with 16 contiguous coefficients per thread; arrays
// that never leave the library keep them as the threads hold them: pair j (coefficients 2j, 2j + 1 of the 16) of thread
// tau at 2 (512 j + tau) -- coalesced 16-byte lanes, no transpose.  Standard (bit-reversed) order costs one more LDS
// round trip and is offered on the inverse's input side only (the accumulators of stage A arrive in it).
#pragma once
#include <vector>

#include "madasm.h"
#include "params.hpp"

namespace piehip {
namespace ntt16 {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// Slices of 2^13 (512 threads, two workgroups per CU) or 2^14 coefficients (1024 threads, one workgroup per CU: rings of
// 2^15 as two folded slices per limb).  The wave-local passes 2-4 are the same; pass 1 covers the stages above a wave's 1024
// elements: 3 stages on 8 rows x 2 columns per thread (16-byte lanes), or 4 stages on 16 rows x 1 column (8-byte lanes).
template <u32 LOGNS>
struct Geo {
    static constexpr u32 LOGN = LOGNS;
    static constexpr u32 NS = 1u << LOGNS;     // coefficients per slice
    static constexpr u32 T = NS / 16;          // threads per slice
    static constexpr u32 W = T / 64;           // waves per slice = 1024-element blocks
    static constexpr u32 R = NS / 1024;        // rows of pass 1 (stride 1024)
    static constexpr u32 LOGR = LOGNS - 10;    // stages of pass 1
    static constexpr u32 CPT = 16 / R;         // columns per thread in pass 1
    static constexpr u32 LDS_WORDS = NS + NS / 16;
    static constexpr u32 TWK_PER_SLICE = W * 15 * 16 + W * 12 * 64;  // kernel-ordered twiddle pairs of passes 3 and 4
};
// (the 2^13 geometry under its old names: tools/ntt_lab.hip)
static constexpr u32 LOGN = Geo<13>::LOGN, NS = Geo<13>::NS, T = Geo<13>::T, LDS_WORDS = Geo<13>::LDS_WORDS,
                     TWK_PER_SLICE = Geo<13>::TWK_PER_SLICE;

__device__ __forceinline__ u32 phi(u32 e) { return e + 2 * (e >> 5); }

struct Tw {  // {w, floor(w 2^63 / q)} split into 32-bit halves; sh2 = 2 sh (sh < 2^31) for the quotient estimate
    u32 wl, wh, sl, sh, sh2;
};
__device__ __forceinline__ Tw make_tw(u64x2 p)
{
    Tw t;
    t.wl = (u32)p.x, t.wh = (u32)(p.x >> 32), t.sl = (u32)p.y, t.sh = (u32)(p.y >> 32);
    t.sh2 = t.sh << 1;  // wave-uniform twiddles: a scalar shift; per-lane ones: one shift per twiddle, not per butterfly
    return t;
}

// per-modulus constants of the butterflies (wave-uniform: SGPRs)
struct ModC {
    u32 nql, nqh;  // 2^64 - q
    u64 nq4;       // 2^64 - 4q
    u64 q4;        // 4q
};

// ---- the 60-bit lazy butterfly as hand-scheduled instruction blocks ---------------------------------------------------------
// Shoup product b w mod q + {0,1,2,3} q with the 63-bit constant ws = floor(w 2^63 / q) (b < 2^63, w < q < 2^60):
//   quotient estimate  qe = 2 bh sh + ((bh sl + bl sh) >> 31)           3 multiplier ops (bl sl dropped, error <= 3)
//   remainder          b w + qe (2^64 - q)  mod 2^64                    6 multiplier ops on two accumulation chains
// (derivation in kernels_ntt_fast.hip).  Why assembly blocks (tools/gen_ntt16_bfly.py writes them): hipcc narrows multiplier
// ops whose high half is dead to v_mul_lo_u32 (half the rate), lowers conditional subtractions to compare + select chains
// through VCC (a VALU write of VCC or an SGPR needs two wait states before a VALU may read it on gfx950) and pads every short
// asm statement with s_nop.  19-20 instructions per inverse butterfly, 18-19 per forward one, 9 of them on the multiplier, 11
// (forward: 9) fixed scratch registers at the top of the 128-register budget.  Conditional subtraction x in [0, 2m) -> [0, m)
// as t = x - m followed by a select on the sign of t (v_bfi_b32 under an arithmetic-shift mask); the two 64-bit differences
// (u + 4q - v forward, a + 4q - b inverse) as v_sub_co_u32 / v_subb_co_u32 with two independent instructions between the
// halves (the wait states a VALU read of VCC needs after a VALU write); every other carry-out is discarded into VCC.
//
// The forward block is seeded (NTT16_CTS1 / NTT16_CTS1H, 19 / 18 instructions).  u + v, the product's remainder
// b w + qe (2^64 - q) and u + 4q - v are all taken mod 2^64 and all lie below 8q < 2^63, so the low accumulation chain of the
// remainder starts at bl wl + u instead of bl wl + 0 and ends as a' = u + v; b' = (2u + 4q) - a' with 2u + 4q < 12q < 2^64
// (one v_lshl_add_u64 with shift 1).
// Contract: a is a tied operand ("+v"), its halves are also passed as the 32-bit INPUTS al / ah, and the block relies on the
// register allocator keeping those in the two registers of a's pair.  Once the chain has written the pair the block reads the
// low half of a' through %[al] and both reads AND WRITES the high half through %[ah] (v_add_u32 %[ah], %[ah], c_lo).  Writing
// an input operand is outside what the asm constraints express: the compiler believes ah's register unchanged, which is true
// only because that register is the high half of the tied output.  Where the allocator chose otherwise the block would be
// silently wrong, not merely slow.  So the aliasing is not a tuning check but part of the block's correctness:
// tools/ct_seeded_listing.py asserts it for every block of the listing of kernels_ntt16.hip (profiles/ct_seeded/), and
// tests/test_ct_seeded_listing.py runs that on every checkout as part of the default suite (no GPU needed); it must stay
// there, and has to pass after any change to this file, to a kernel that calls bfly<false, ...>, or to the compiler.
// -DNTT16_CT_SEEDED=0 builds the unseeded block (NTT16_CT1 / NTT16_CT1H, 20 / 19), which has no such dependence.
#ifndef NTT16_CT_SEEDED
#define NTT16_CT_SEEDED 1
#endif
#define NTT16_S(x) "s"(x)
#define NTT16_V(x) "v"(x)
#include "ntt16_bfly.inc"

// forward (Cooley-Tukey): a, b in [0, 8q) -> a' = u + v, b' = u - v + 4q with u = a mod+ 4q in [0, 4q), v = b w in [0, 4q)
// inverse (Gentleman-Sande): a, b in [0, 4q) -> a' = (a + b) mod+ 4q, b' = (a - b + 4q) w, both in [0, 4q)
// SC: the twiddles are wave-uniform (SGPR operands).  H2: the block takes 2 sh as an operand (t.sh2) instead of doubling the
// high word of the multiplicand itself -- one instruction fewer; worth it where a twiddle serves several butterflies (every
// wave-uniform one: the doubling is a scalar instruction; per-lane ones of the stages with fewer twiddles than butterflies).
#ifndef NTT16_INV_H2
#define NTT16_INV_H2 1
#endif
template <bool INV, bool SC, bool H2 = SC && (!INV || NTT16_INV_H2)>
__device__ __forceinline__ void bfly(u64 &x0, u64 &y0, const Tw &t0, const ModC &m)
{
    u64 a0 = x0;  // forward, seeded: the tied operand -- a on entry, a' on exit
    const u64 b0 = y0;
    if (INV) {
        u32 aol0, aoh0;
        u64 bo0;
        if (SC && H2)
            NTT16_GS1H(NTT16_S);
        else if (SC)
            NTT16_GS1(NTT16_S);
        else if (H2)
            NTT16_GS1H(NTT16_V);
        else
            NTT16_GS1(NTT16_V);
        x0 = ((u64)aoh0 << 32) | aol0, y0 = bo0;
    } else {
        u32 bol0, boh0;
#if NTT16_CT_SEEDED
        u64 cs;  // takes one discarded carry-out (an SGPR pair, never read)
        if (SC && H2)
            NTT16_CTS1H(NTT16_S);
        else if (SC)
            NTT16_CTS1(NTT16_S);
        else if (H2)
            NTT16_CTS1H(NTT16_V);
        else
            NTT16_CTS1(NTT16_V);
        (void)cs;
        x0 = a0, y0 = ((u64)boh0 << 32) | bol0;
#else
        u64 ao0;
        if (SC && H2)
            NTT16_CT1H(NTT16_S);
        else if (SC)
            NTT16_CT1(NTT16_S);
        else if (H2)
            NTT16_CT1H(NTT16_V);
        else
            NTT16_CT1(NTT16_V);
        x0 = ao0, y0 = ((u64)boh0 << 32) | bol0;
#endif
    }
}
// two butterflies (call sites pair them; one block each: see tools/gen_ntt16_bfly.py on why they are not interleaved)
template <bool INV, bool SC, bool H2 = SC && !INV>
__device__ __forceinline__ void bfly2(u64 &x0, u64 &y0, const Tw &t0, u64 &x1, u64 &y1, const Tw &t1, const ModC &m)
{
    bfly<INV, SC, H2>(x0, y0, t0, m);
    bfly<INV, SC, H2>(x1, y1, t1, m);
}
// m-th index in [0, 16) whose bit `d` (a power of two) is clear
__device__ __forceinline__ constexpr int bfly_lo(int m, int d) { return ((m & ~(d - 1)) << 1) | (m & (d - 1)); }

// Wave-uniform tables (twiddles of passes 1 and 2, modulus constants) are read through the constant address space: a
// plain global pointer gives vector loads of a uniform address (the compiler cannot prove that the kernel's own stores leave
// the tables alone) -- 22 global_load_dwordx4 per slice queued in order behind the slice's HBM loads, four VGPRs per
// twiddle, VGPR operands in the butterfly blocks.  Through address space 4 they are s_load_dwordx4 into SGPRs.
typedef const __attribute__((address_space(4))) u64x2 *TwS;
typedef const __attribute__((address_space(4))) DevConsts *DcS;
__device__ __forceinline__ u64 uniform_addr(const void *p)  // (uniform integer divisions leave their results in VGPRs)
{
    const u64 v = (u64)p;
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// x in [0, 2m) -> [0, m) with the NEGATED modulus (2^64 - m), wave-uniform: t = x - m as one v_lshl_add_u64, then a select on
// the sign of t (v_ashrrev_i32 + two v_bfi_b32): 4 instructions.  hipcc's `x >= m ? x - m : x` is compare + subtract pair +
// two v_cndmask_b32 through VCC with its wait states, and `x + negm` in C++ becomes v_subrev_co / s_nop 1 / v_subb_co with the
// high word of the constant moved into a vector register first -- the whole step inside one statement avoids both.  (The
// temporaries are three of the butterfly blocks' fixed registers.)
__device__ __forceinline__ u64 csub_neg(u64 x, u64 negm)
{
    u32 lo, hi;
    asm("v_lshl_add_u64 v[126:127], %[x], 0, %[nm]\n\t"
        "v_ashrrev_i32 v125, 31, v127\n\t"
        "v_bfi_b32 %[lo], v125, %[xl], v126\n\t"
        "v_bfi_b32 %[hi], v125, %[xh], v127"
        : [lo] "=&v"(lo), [hi] "=&v"(hi)
        : [x] "v"(x), [xl] "v"((u32)x), [xh] "v"((u32)(x >> 32)), [nm] "s"(negm)
        : "v125", "v126", "v127");
    return ((u64)hi << 32) | lo;
}

// Global addresses are "uniform base + 32-bit lane offset in BYTES" (the global_load / global_store form with a scalar base
// register pair and one vector offset register).  Written with element offsets the scaling happens after the zero-extension, the
// compiler can no longer prove that the offset fits 32 bits, and every access pattern keeps a 64-bit per-lane offset pair alive
// across the item loop (eight registers instead of four, and 64-bit vector adds per access).
__device__ __forceinline__ const u64 *at_bytes(const u64 *ubase, u32 boff)
{
    return reinterpret_cast<const u64 *>(reinterpret_cast<const char *>(ubase) + boff);
}
__device__ __forceinline__ u64 *at_bytes(u64 *ubase, u32 boff) { return reinterpret_cast<u64 *>(reinterpret_cast<char *>(ubase) + boff); }
__device__ __forceinline__ const u64x2 *at_bytes(const u64x2 *ubase, u32 boff)
{
    return reinterpret_cast<const u64x2 *>(reinterpret_cast<const char *>(ubase) + boff);
}

// the CPT coefficients a thread holds of row r (pass 1): x[CPT r .. CPT r + CPT)
template <u32 CPT>
__device__ __forceinline__ void row_get(u64 *x, int r, const u64 *p)
{
    if (CPT == 2) {
        const u64x2 v = *reinterpret_cast<const u64x2 *>(p);
        x[2 * r] = v.x, x[2 * r + 1] = v.y;
    } else {
        x[r] = *p;
    }
}
template <u32 CPT>
__device__ __forceinline__ void row_put(const u64 *x, int r, u64 *p)
{
    if (CPT == 2) {
        u64x2 v;
        v.x = x[2 * r], v.y = x[2 * r + 1];
        *reinterpret_cast<u64x2 *>(p) = v;
    } else {
        *p = x[r];
    }
}
// Global-memory accesses of the slice itself: through pointers in the GLOBAL address space.  The item loop makes the slice base
// opaque (a scalar pair, see the kernel), and with that the compiler no longer knows which address space a derived pointer is in:
// it would emit FLAT loads and stores, which also count in lgkmcnt -- every wait for an LDS read or a scalar twiddle load behind
// one then waits for HBM.
// (Non-temporal loads / stores of the slices, per launch site, were measured in r04: the transforms get 3-6 % shorter and the
// kernels that consume their output -- which then find nothing in the memory-side cache -- longer by the same microseconds.)
typedef __attribute__((address_space(1))) u64 g_u64;
typedef __attribute__((address_space(1))) u64x2 g_u64x2;
__device__ __forceinline__ u64x2 pair_get_global(const u64 *p) { return *(const g_u64x2 *)p; }
__device__ __forceinline__ void pair_put_global(u64x2 v, u64 *p) { *(g_u64x2 *)p = v; }
template <u32 CPT>
__device__ __forceinline__ void row_put_global(const u64 *x, int r, u64 *p)
{
    if (CPT == 2) {
        u64x2 v;
        v.x = x[2 * r], v.y = x[2 * r + 1];
        pair_put_global(v, p);
    } else {
        *(g_u64 *)p = x[r];
    }
}
template <u32 CPT>
__device__ __forceinline__ void row_get_global(u64 *x, int r, const u64 *p)
{
    if (CPT == 2) {
        const u64x2 v = pair_get_global(p);
        x[2 * r] = v.x, x[2 * r + 1] = v.y;
    } else {
        x[r] = *(const g_u64 *)p;
    }
}

// DS operations of one wave execute in issue order: a hand-off inside the wave only needs the compiler kept from
// moving the reads above the writes
__device__ __forceinline__ void wave_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

struct Args {
    u64 *data;            // slices [nitems][NS] (item -> slice through the enumeration below)
    const u64x2 *twp;     // natural-order {w, w_shoup63} pairs: per modulus [fwd N][inv N]
    const u64x2 *twk;     // kernel-ordered pairs of passes 3, 4: per modulus [fwd][inv][slices per limb][TWK_PER_SLICE]
    const DevConsts *dc;
    u32 N;                // ring dimension (pairs per table)
    u32 s0;               // log2 slices per limb
    u32 nitems;           // slices to transform
    u32 mod_base, mod_count;  // limb i uses modulus mod_base + i % mod_count
    u32 flags;
    // forward: the limbs are a compact enumeration of [nb][4][skip_M] without limbs < skip_L of slots 0, 1 (skip_L = 0: off)
    u32 skip_L, skip_M;
    // inverse, standard order in: the lane-ordered EVALUATION input of operand-0 polynomials is also written to
    // copy_out[bin][4][copy_M][N], slots 0, 1, limbs < copy_L (input limbs are [nb][copy_K][2][copy_L])
    u64 *copy_out;
    u32 copy_K, copy_L, copy_M;
    // forward: items [lift_first, nitems) are BV key-switch digits: limb (bin, i, j) of data2[nb][lift_L][lift_L][N]
    // is the centred lift into q_j of residue limb i of the COEFFICIENT polynomial lift_src + bin * lift_stride, transformed;
    // the lift (and, with two folded slices per limb, the outermost stage) happens in the load phase.  lift_first >= nitems: off
    u64 *data2;
    const u64 *lift_src;
    size_t lift_stride;
    u32 lift_first, lift_L;
    // inverse, TENSOR instantiation: the input of item (row, d, limb m, slice) is not read from data but formed in the load phase
    // from the lane-ordered QP operands tsrc[row][4][mod_count][N] (a0 a1 b0 b1): d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1
    const u64 *tsrc;
    // ... tq_L != 0: d0 and d1 are wanted on their P limbs (>= tq_L) only.  Items [0, tq_first) are the (d0, d1, d2) triples of the P
    // limbs, items [tq_first, nitems) the d2 items of the Q limbs: (row, limb < tq_L, slice).  tq_L = 0: tq_first = nitems, every limb a triple
    u32 tq_L, tq_first;
};
enum : u32 {
    F_STD_IN = 1,    // inverse: EVALUATION input in standard (bit-reversed) order instead of lane order
    F_LAZY_OUT = 2,  // forward: leave [0, 8q) residues (the consumer reduces anyway)
    F_FOLDED = 4,    // inverse: the consumer applies the outermost stage and N^-1: hand over [0, 4q) residues as they are
    F_X_LANE_IN = 8, // inverse, standard order in: operand-0 polynomials come lane-ordered from copy_out's place instead (no copy)
};

// Host side: the twiddle pairs of passes 3 and 4 of one (modulus, direction) in kernel order, for every slice of a limb.
// nat: the N natural-order pairs {w, w_shoup63} (index = 2^stage + group).  out: [1 << s0][TWK_PER_SLICE] pairs.
template <u32 LOGNS>
inline void build_twk_table_t(const u64 *nat, u32 s0, std::vector<u64> &out)
{
    typedef Geo<LOGNS> G;
    out.assign((size_t)(1u << s0) * G::TWK_PER_SLICE * 2, 0);
    for (u32 blk = 0; blk < (1u << s0); blk++) {
        u64 *o = &out[(size_t)blk * G::TWK_PER_SLICE * 2];
        auto put = [&](size_t dst, size_t src) {
            o[2 * dst] = nat[2 * src];
            o[2 * dst + 1] = nat[2 * src + 1];
        };
        for (u32 w = 0; w < G::W; w++) {
            for (u32 sc = 0; sc < 4; sc++)  // pass 3: the four stages below pass 2, 16 W << sc local groups
                for (u32 jj = 0; jj < (1u << sc); jj++)
                    for (u32 la = 0; la < 16; la++) {
                        const u32 ml = (16 * G::W) << sc;
                        put(((size_t)w * 15 + ((1u << sc) - 1 + jj)) * 16 + la, ((size_t)ml << s0) + (size_t)blk * ml + (((16 * w + la) << sc) + jj));
                    }
            for (u32 l = 0; l < 64; l++) {  // pass 4: the last two stages (slots 0..3 and 4..11)
                const u32 m11 = 256 * G::W, m12 = 512 * G::W;
                for (u32 jj = 0; jj < 4; jj++)
                    put(G::W * 15 * 16 + ((size_t)w * 12 + jj) * 64 + l, ((size_t)m11 << s0) + (size_t)blk * m11 + 256 * w + 4 * l + jj);
                for (u32 jj = 0; jj < 8; jj++)
                    put(G::W * 15 * 16 + ((size_t)w * 12 + 4 + jj) * 64 + l, ((size_t)m12 << s0) + (size_t)blk * m12 + 512 * w + 8 * l + jj);
            }
        }
    }
}
inline void build_twk_table(const u64 *nat, u32 s0, std::vector<u64> &out) { build_twk_table_t<13>(nat, s0, out); }
// lane-order position p of a slice of T * 16 coefficients -> standard (bit-reversed) position
inline u32 lane_to_std_t(u32 p, u32 threads)
{
    const u32 tau = (p >> 1) % threads, j = (p >> 1) / threads;
    return 16 * tau + 2 * j + (p & 1);
}
inline u32 lane_to_std(u32 p) { return lane_to_std_t(p, T); }

// in-kernel cycle stamps are a tooling build (tools/ntt_lab.hip defines NTT16_STAMP before including this file)
#ifndef NTT16_STAMP
#define NTT16_STAMP(i)
#endif

// ---- the four register passes (x[16] in the layout the pass names) ---------------------------------------------------------
// group index of a stage with ml local groups: global table index (ml << s0) + blk * ml + i
#define NTT16_TWL(ml, i) tw[(((u32)(ml)) << a.s0) + blk * (u32)(ml) + (i)]
// LDS addresses are written as (one per-thread base) + (compile-time constant): phi is additive over multiples of 32, and a
// base the compiler has to keep per row ends up in scratch memory.  Global addresses: uniform row base + one lane offset.
#define NTT16_FENCE() __builtin_amdgcn_sched_barrier(0)
// Wave priority falls as a wave advances from one workgroup barrier to the next.  The SIMD arbiter serves the highest
// priority, then the oldest wave: with equal priorities the older of the waves a workgroup has on each SIMD runs at full speed,
// the younger on what is left, and the workgroup's barriers then wait for the younger ones (measured: 9000 of 32000 cycles per
// slice).  With the priority tied to progress the wave that is behind is served first and all arrive together.  Forward: the
// barrier sits after pass 1, so pass 2 is the start of the cycle and pass 1 of the NEXT slice its end (lowest priority; its
// loads are issued at the highest, they are a handful of instructions): 2048 slices 88.2 -> 82.5 us against "pass 1 highest",
// the run's ragged launches unchanged (profiles/r03/ntt16_lab_wave_priorities.txt).  Inverse (r04): both barriers sit between
// pass 2' and pass 1' (around the row reads), so pass 1' opens the cycle and pass 2' closes it at the lowest priority
// (profiles/r04/ntt16_lab_wave_priorities_inverse.txt).
#define NTT16_PASS_PRIO(p) __builtin_amdgcn_s_setprio(p)
#ifndef NTT16_PF
#define NTT16_PF 3, 0, 3, 2, 1   // forward: loads, pass 1, pass 2, pass 3, pass 4
#endif
#ifndef NTT16_PI
#define NTT16_PI 3, 3, 2, 0, 1   // inverse: loads, pass 4', pass 3', pass 2', pass 1'
#endif
#define NTT16_PRIO_PICK_(i, a0, a1, a2, a3, a4) ((i) == 0 ? (a0) : (i) == 1 ? (a1) : (i) == 2 ? (a2) : (i) == 3 ? (a3) : (a4))
#define NTT16_PRIO_PICK(i, ...) NTT16_PRIO_PICK_(i, __VA_ARGS__)
#define NTT16_PRIO_F(i) NTT16_PASS_PRIO(NTT16_PRIO_PICK(i, NTT16_PF))
#define NTT16_PRIO_I(i) NTT16_PASS_PRIO(NTT16_PRIO_PICK(i, NTT16_PI))

#ifndef NTT16_LIFT_XCD
#define NTT16_LIFT_XCD 1
#endif
// ---- the tensor product in the inverse transform's load phase (TENSOR instantiation) ----------------------------------------
// What tensor_kernel<true> (kernels_pie.hip) computes, for the one result polynomial d of the item, straight into x[16]: the
// result never goes to memory.  The operands arrive in [0, 8q) from the lazy forward transform; sign-mask subtractions bring
// them below 2q (the second factor of a single product: below 4q is enough), the products go through the carry-free 30-bit
// column sums (madasm.h) and one Barrett block that leaves [0, 4q) -- what the inverse butterflies take.  Bounds, q < 2^60:
//   one product   a < 2q, b < 4q:  30-bit low halves, high halves < 2^31 and < 2^32; columns < 2^60, < 2^63, < 2^63; z < 8 q^2 < 2^123
//   two products  all < 2q:        high halves < 2^31; columns < 2^61, < 2^63, < 2^63;                           z < 8 q^2 < 2^123
// The block is kernels_pie.hip's PIE_COLACC123_TO_4Q (one-word Barrett with mu = floor(2^123 / q): z >> 59 from the
// carry-normalised columns, quotient estimate at most 2 short: modarith.h) on ten of the butterfly blocks' fixed registers.
#ifndef NTT16_TENSOR_XCD
#define NTT16_TENSOR_XCD 1
#endif
// x in [0, 8q) -> [0, 2q): csub_neg by 4q, then by 2q, as one statement
__device__ __forceinline__ u64 csub2_neg(u64 x, u64 negm4, u64 negm2)
{
    u32 lo, hi;
    asm("v_lshl_add_u64 v[126:127], %[x], 0, %[n4]\n\t"
        "v_ashrrev_i32 v125, 31, v127\n\t"
        "v_bfi_b32 v122, v125, %[xl], v126\n\t"
        "v_bfi_b32 v123, v125, %[xh], v127\n\t"
        "v_lshl_add_u64 v[126:127], v[122:123], 0, %[n2]\n\t"
        "v_ashrrev_i32 v125, 31, v127\n\t"
        "v_bfi_b32 %[lo], v125, v122, v126\n\t"
        "v_bfi_b32 %[hi], v125, v123, v127"
        : [lo] "=&v"(lo), [hi] "=&v"(hi)
        : [x] "v"(x), [xl] "v"((u32)x), [xh] "v"((u32)(x >> 32)), [n4] "s"(negm4), [n2] "s"(negm2)
        : "v122", "v123", "v125", "v126", "v127");
    return ((u64)hi << 32) | lo;
}
// the folded block for q = 2^60 - d, d < COLACC_FOLD_MAX_D (stage_a_common.h: PIE_COLACC_FOLD_HEAD and its bound proof; z < 2^123
// here, the result below 2.75 2^60 < 3q), on eight of those registers; d is the low word of nq, no mu
__device__ __forceinline__ u64 colacc_fold_to_4q(u64 c0, u64 c1, u64 c2, u64 nq)
{
    u64 r;
    asm("v_lshrrev_b64 v[118:119], 30, %[c0]\n\t"
        "v_lshl_add_u64 v[118:119], v[118:119], 0, %[c1]\n\t"
        "v_lshrrev_b64 v[120:121], 30, v[118:119]\n\t"
        "v_lshl_add_u64 v[120:121], v[120:121], 0, %[c2]\n\t"
        "v_and_b32 v124, 0x3fffffff, %[c0l]\n\t"
        "v_bfe_u32 v125, v118, 2, 28\n\t"
        "v_mad_u64_u32 v[122:123], vcc, v121, %[d], 0\n\t"
        "v_lshl_or_b32 v124, v118, 30, v124\n\t"
        "v_mad_u64_u32 v[124:125], vcc, v120, %[d], v[124:125]\n\t"
        "v_and_b32 v118, 0xfffffff, v122\n\t"
        "v_alignbit_b32 v119, v123, v122, 28\n\t"
        "v_add_u32 v125, v125, v118\n\t"
        "v_mad_u64_u32 %[r], vcc, v119, %[d], v[124:125]"
        : [r] "=v"(r)
        : [c0] "v"(c0), [c1] "v"(c1), [c2] "v"(c2), [c0l] "v"((u32)c0), [d] "s"((u32)nq)
        : "vcc", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125");
    return r;
}
__device__ __forceinline__ u64 colacc123_to_4q(u64 c0, u64 c1, u64 c2, u64 mu, u64 nq)
{
    u64 r;
    asm("v_lshrrev_b64 v[118:119], 30, %[c0]\n\t"
        "v_lshl_add_u64 v[118:119], v[118:119], 0, %[c1]\n\t"
        "v_lshrrev_b64 v[120:121], 30, v[118:119]\n\t"
        "v_lshl_add_u64 v[120:121], v[120:121], 0, %[c2]\n\t"
        "v_lshlrev_b64 v[122:123], 1, v[120:121]\n\t"
        "v_bfe_u32 v126, v118, 29, 1\n\t"
        "v_and_b32 v124, 0x3fffffff, %[c0l]\n\t"
        "v_bfe_u32 v125, v118, 2, 28\n\t"
        "v_or_b32 v122, v122, v126\n\t"
        "v_lshl_or_b32 v124, v118, 30, v124\n\t"
        "v_lshl_or_b32 v125, v120, 28, v125\n\t"
        "v_mul_hi_u32 v126, v122, %[mul]\n\t"
        "v_mov_b32 v127, 0\n\t"
        "v_mad_u64_u32 v[126:127], vcc, v122, %[muh], v[126:127]\n\t"
        "v_mad_u64_u32 v[126:127], vcc, v123, %[mul], v[126:127]\n\t"
        "v_mad_u64_u32 v[118:119], s[96:97], v123, %[muh], 0\n\t"
        "v_lshrrev_b64 v[126:127], 32, v[126:127]\n\t"
        "v_addc_co_u32 v127, vcc, 0, v127, vcc\n\t"
        "v_lshl_add_u64 v[126:127], v[118:119], 0, v[126:127]\n\t"
        "v_mad_u64_u32 v[118:119], vcc, v126, %[nqh], 0\n\t"
        "v_mad_u64_u32 v[118:119], vcc, v127, %[nql], v[118:119]\n\t"
        "v_add_u32 v125, v125, v118\n\t"
        "v_mad_u64_u32 %[r], vcc, v126, %[nql], v[124:125]"
        : [r] "=v"(r)
        : [c0] "v"(c0), [c1] "v"(c1), [c2] "v"(c2), [c0l] "v"((u32)c0), [mul] "s"((u32)mu), [muh] "s"((u32)(mu >> 32)),
          [nql] "s"((u32)nq), [nqh] "s"((u32)(nq >> 32))
        : "vcc", "s96", "s97", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
    return r;
}
// x[16] <- a b (TWO: a b + c d) of the lane-ordered slices at pa, pb (pc, pd).  Four operands of 16 coefficients do not fit
// beside x[16]: the 16-byte lanes come in as a window of NTT16_TENSOR_DEPTH pairs per operand, the next one requested as a pair's
// products are done (its registers are the ones just freed).
#ifndef NTT16_TENSOR_DEPTH
#define NTT16_TENSOR_DEPTH 3
#endif
// FD (NttPlan::fold_moduli): the folded block reduces the column sums, mu is not used
template <u32 T, bool TWO, bool FD>
__device__ __forceinline__ void tensor_load(u64 (&x)[16], const u64 *pa, const u64 *pb, const u64 *pc, const u64 *pd, u32 voffb, u64 q,
                                            u64 mu)
{
    constexpr int DEPTH = NTT16_TENSOR_DEPTH;
    const u64 nq = 0 - q, nq2 = 0 - 2 * q, nq4 = 0 - 4 * q;
    u64x2 va[8], vb[8], vc[8], vd[8];
#define NTT16_TLOAD(j)                                                           \
    do {                                                                         \
        va[j] = pair_get_global(at_bytes(pa + 2 * T * (j), voffb));              \
        vb[j] = pair_get_global(at_bytes(pb + 2 * T * (j), voffb));              \
        if (TWO) {                                                               \
            vc[j] = pair_get_global(at_bytes(pc + 2 * T * (j), voffb));          \
            vd[j] = pair_get_global(at_bytes(pd + 2 * T * (j), voffb));          \
        }                                                                        \
    } while (0)
#pragma unroll
    for (int j = 0; j < DEPTH; j++) NTT16_TLOAD(j);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        NTT16_FENCE();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const u64 fa = csub2_neg(k ? va[j].y : va[j].x, nq4, nq2);
            const u64 fb = TWO ? csub2_neg(k ? vb[j].y : vb[j].x, nq4, nq2) : csub_neg(k ? vb[j].y : vb[j].x, nq4);
            const Split30 sa = split30(fa), sb = split30(fb);
            ColAcc c;
            c.c0 = mul_u(sa.lo, sb.lo);
            c.c1 = mad_u(sa.hi, sb.lo, mul_u(sa.lo, sb.hi));
            c.c2 = mul_u(sa.hi, sb.hi);
            if (TWO) {
                const u64 fc = csub2_neg(k ? vc[j].y : vc[j].x, nq4, nq2);
                const u64 fd = csub2_neg(k ? vd[j].y : vd[j].x, nq4, nq2);
                colacc_mac(c, split30(fc), split30(fd));
            }
            x[2 * j + k] = FD ? colacc_fold_to_4q(c.c0, c.c1, c.c2, nq) : colacc123_to_4q(c.c0, c.c1, c.c2, mu, nq);
        }
        NTT16_FENCE();
        if (j + DEPTH < 8) NTT16_TLOAD(j + DEPTH);
    }
#undef NTT16_TLOAD
}

// LIFT (forward only): the launch may carry key-switch digit items (Args::lift_first); a separate instantiation, so that the
// plain forward transform does not pay for the lift's registers
// TENSOR (inverse only, lane order in): every item forms its input from the QP operands (Args::tsrc); likewise its own instantiation
// FD (TENSOR only): the context's moduli take the folded reduction block (NttPlan::fold_moduli) -- ntt16_tensor_fd_kernel_t, a kernel
// of its own name: the ntt16_kernel_t keep their names and their listings.  Both are the one body of ntt16_kernel_body.inc.
template <u32 LOGNS, bool INV, bool LIFT = false, bool TENSOR = false>
__global__ void __launch_bounds__(Geo<LOGNS>::T, 4) ntt16_kernel_t(Args a)
{
    constexpr bool FD = false;
#include "ntt16_kernel_body.inc"
}
template <u32 LOGNS>
__global__ void __launch_bounds__(Geo<LOGNS>::T, 4) ntt16_tensor_fd_kernel_t(Args a)
{
    constexpr bool INV = true, LIFT = false, TENSOR = true, FD = true;
#include "ntt16_kernel_body.inc"
}
#undef NTT16_LOAD3
#undef NTT16_LOAD3H
#undef NTT16_LOAD4
#undef NTT16_FENCE
#undef NTT16_TWL

}  // namespace ntt16
}  // namespace piehip
