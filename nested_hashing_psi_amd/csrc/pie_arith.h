// pie_arith.h -- the arithmetic helpers of the base conversions of pie_convert.h (sign-mask conditional subtraction, the
// constant-operand modular products as instruction blocks, the exact high product, the CRT lift), in a header so that
// tests/arith_check compiles these definitions themselves.  Moved here word for word: the kernels compile to the same
// instructions as before (profiles/arith_blocks/).
#pragma once
#include "kernels.hpp"
#include "madasm.h"
#include "stage_a_common.h"

namespace piehip {

// Conditional subtraction with a wave-uniform modulus, without VCC: t = x - m as x + (2^64 - m) (one v_lshl_add_u64 with the
// negated modulus in scalar registers), then a select on the sign of t (v_ashrrev_i32 + two v_bfi_b32).  hipcc's lowering of
// `x >= m ? x - m : x` is compare + two moves of the modulus into vector registers + two v_cndmask + a two-instruction
// subtraction through VCC with its wait state: 8 instructions against 4, ~120 times per coefficient pair of a base conversion.
// Needs x < 2^63 and x - m > -2^63 (all residues here are below 2^62).
__device__ __forceinline__ u64 neg_u(u64 m)  // 2^64 - m, kept opaque so that x + neg_u(m) stays an addition
{
    u64 n = 0 - m;
    asm("" : "+s"(n));
    return n;
}
__device__ __forceinline__ u64 sel_neg(u64 x, u64 t, u32 &mask)  // t < 0 ? x : t;  mask = t < 0 ? ~0 : 0
{
    u32 lo, hi, k;
    asm("v_ashrrev_i32 %[k], 31, %[th]\n\t"
        "v_bfi_b32 %[lo], %[k], %[xl], %[tl]\n\t"
        "v_bfi_b32 %[hi], %[k], %[xh], %[th]"
        : [lo] "=&v"(lo), [hi] "=&v"(hi), [k] "=&v"(k)
        : [xl] "v"((u32)x), [xh] "v"((u32)(x >> 32)), [tl] "v"((u32)t), [th] "v"((u32)(t >> 32)));
    mask = k;
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 csub_u(u64 x, u64 negm)
{
    u32 k;
    return sel_neg(x, x + negm, k);
}
// the modarith.h formulas with this subtraction (same values; moduli wave-uniform: they come from ld_mod / scalar loads)
__device__ __forceinline__ u64 mul_shoup_lazy_u(u64 a, u64 w, u64 wsh, u64 q) { return a * w - mulhi(a, wsh) * q; }
__device__ __forceinline__ u64 mul_shoup_u(u64 a, u64 w, u64 wsh, u64 q, u64 negq) { return csub_u(mul_shoup_lazy_u(a, w, wsh, q), negq); }
__device__ __forceinline__ u64 fixfrac_u(u64 y, const Mod &m) { return mulhi(y << m.fshift, m.fconst) >> 3; }
__device__ __forceinline__ void divmod_shoup_u(u64 a, u64 w, u64 wsh, u64 q, u64 negq, u64 &quot, u64 &rem)
{
    const u64 qe = mulhi(a, wsh);
    const u64 r = a * w - qe * q;
    u32 k;
    rem = sel_neg(r, r + negq, k);
    quot = qe + 1 + (u64)(int64_t)(int32_t)k;  // + 1 unless r < q
}
__device__ __forceinline__ u64 reduce123_u(U128 z, const Mod &m, u64 negq, u64 neg2q)
{
    const u64 mu = (m.r1 << 59) | (m.r0 >> 5);
    const u64 zh = (z.hi << 5) | (z.lo >> 59);
    const u64 qhat = mulhi(zh, mu);
    return csub_u(csub_u(z.lo - qhat * m.q, neg2q), negq);
}

// ---- constant-operand modular products as instruction blocks (every modulus < 2^60) ---------------------------------------------
// A mixed VALU stream issues one instruction per ~4 cycles per wave on gfx950 whatever the instruction (a 2-cycle VOP1/VOP2
// that follows a 4-cycle VOP3 costs 4: profiles/r03/microbench_operands.txt), so these kernels are bound by their instruction
// COUNT.  hipcc spends 28 instructions on a Shoup product with a wave-uniform constant (an exact __umul64hi with six register
// moves, three 64-bit low products through v_mul_lo_u32 + v_add3_u32, a subtraction through VCC with its wait state); the NTT
// butterfly's formulation does it in 12 -- quotient estimate from the 63-bit constant floor(w 2^63 / q) with three multiplier
// operations (error <= 3), remainder a w + qe (2^64 - q) on two v_mad_u64_u32 chains -- plus two sign-mask subtractions for a
// canonical result.  Temporaries whose halves are needed live in fixed registers v60-v71 (low enough that scale_round stays at
// 76 VGPRs = six waves per SIMD: its 5.25 waves per SIMD are then one round; an asm operand cannot name the
// halves of a 64-bit pair); constants are SGPR operands, one per instruction (constant-bus limit of VOP3 on gfx9).
// a < 2^63, w < q < 2^60: v[64:65] <- all but the last product of a w mod q + {0..3} q, v[62:63] <- the quotient estimate
#define PIE_SHOUP63_HEAD                                        \
    "v_mad_u64_u32 v[60:61], vcc, %[al], %[sh], 0\n\t"          \
    "v_mad_u64_u32 v[64:65], vcc, %[al], %[wl], 0\n\t"          \
    "v_mad_u64_u32 v[60:61], vcc, %[ah], %[sl], v[60:61]\n\t"   \
    "v_mad_u64_u32 v[66:67], vcc, %[al], %[wh], 0\n\t"          \
    "v_lshlrev_b32 v70, 1, %[ah]\n\t"                           \
    "v_mad_u64_u32 v[66:67], vcc, %[ah], %[wl], v[66:67]\n\t"   \
    "v_lshrrev_b64 v[60:61], 31, v[60:61]\n\t"                  \
    "v_mad_u64_u32 v[62:63], vcc, v70, %[sh], v[60:61]\n\t"     \
    "v_mad_u64_u32 v[66:67], vcc, v62, %[nqh], v[66:67]\n\t"    \
    "v_mad_u64_u32 v[66:67], vcc, v63, %[nql], v[66:67]\n\t"    \
    "v_add_u32 v65, v65, v66\n\t"
#define PIE_SHOUP63_IN(a, w, wsh, nq)                                                                                        \
    [al] "v"((u32)(a)), [ah] "v"((u32)((a) >> 32)), [wl] "s"((u32)(w)), [wh] "s"((u32)((w) >> 32)), [sl] "s"((u32)((wsh) >> 1)), \
        [sh] "s"((u32)((wsh) >> 33)), [nql] "s"((u32)(nq)), [nqh] "s"((u32)((nq) >> 32))
// a w mod q + {0,1,2,3} q for a < 2^63 (wsh = floor(w 2^64 / q), nq = 2^64 - q): 12 instructions
__device__ __forceinline__ u64 shoup63_lazy(u64 a, u64 w, u64 wsh, u64 nq)
{
    u64 r;
    asm(PIE_SHOUP63_HEAD
        "v_mad_u64_u32 %[r], vcc, v62, %[nql], v[64:65]"
        : [r] "=v"(r)
        : PIE_SHOUP63_IN(a, w, wsh, nq)
        : PIE_ASM_CLOB);
    return r;
}
// ... reduced to [0, q): 20 instructions
__device__ __forceinline__ u64 shoup63(u64 a, u64 w, u64 wsh, u64 nq)
{
    u32 lo, hi;
    const u64 n2q = 2 * nq;  // 2^64 - 2q
    asm(PIE_SHOUP63_HEAD
        "v_mad_u64_u32 v[64:65], vcc, v62, %[nql], v[64:65]\n\t"
        "v_lshl_add_u64 v[68:69], v[64:65], 0, %[n2q]\n\t"
        "v_ashrrev_i32 v71, 31, v69\n\t"
        "v_bfi_b32 v64, v71, v64, v68\n\t"
        "v_bfi_b32 v65, v71, v65, v69\n\t"
        "v_lshl_add_u64 v[68:69], v[64:65], 0, %[n1q]\n\t"
        "v_ashrrev_i32 v71, 31, v69\n\t"
        "v_bfi_b32 %[lo], v71, v64, v68\n\t"
        "v_bfi_b32 %[hi], v71, v65, v69"
        : [lo] "=v"(lo), [hi] "=v"(hi)
        : PIE_SHOUP63_IN(a, w, wsh, nq), [n2q] "s"(n2q), [n1q] "s"(nq)
        : PIE_ASM_CLOB);
    return ((u64)hi << 32) | lo;
}
// exact floor(a w / q) and a w mod q for a < q: the estimate is at most 3 short, and each of the two conditional
// subtractions reports whether it subtracted (64-bit sign masks M: quotient = qe + 3 + 2 M1 + M2).  23 instructions
__device__ __forceinline__ void divmod63(u64 a, u64 w, u64 wsh, u64 nq, u64 &quot, u64 &rem)
{
    u32 lo, hi;
    u64 qt;
    const u64 n2q = 2 * nq;
    asm(PIE_SHOUP63_HEAD
        "v_mad_u64_u32 v[64:65], vcc, v62, %[nql], v[64:65]\n\t"
        "v_lshl_add_u64 v[68:69], v[64:65], 0, %[n2q]\n\t"
        "v_ashrrev_i64 v[60:61], 63, v[68:69]\n\t"
        "v_bfi_b32 v64, v60, v64, v68\n\t"
        "v_bfi_b32 v65, v60, v65, v69\n\t"
        "v_lshl_add_u64 v[62:63], v[60:61], 1, v[62:63]\n\t"
        "v_lshl_add_u64 v[68:69], v[64:65], 0, %[n1q]\n\t"
        "v_ashrrev_i64 v[60:61], 63, v[68:69]\n\t"
        "v_bfi_b32 %[lo], v60, v64, v68\n\t"
        "v_bfi_b32 %[hi], v60, v65, v69\n\t"
        "v_lshl_add_u64 v[62:63], v[60:61], 0, v[62:63]\n\t"
        "v_lshl_add_u64 %[qt], v[62:63], 0, 3"
        : [lo] "=v"(lo), [hi] "=v"(hi), [qt] "=v"(qt)
        : PIE_SHOUP63_IN(a, w, wsh, nq), [n2q] "s"(n2q), [n1q] "s"(nq)
        : PIE_ASM_CLOB);
    quot = qt;
    rem = ((u64)hi << 32) | lo;
}
// exact floor(a b / 2^64), b wave-uniform: the cross products are summed with the carry kept (VCC is read two instructions
// after it is written: the wait states a VALU read of a VALU-written VCC needs on gfx950).  8 instructions (hipcc: 11)
__device__ __forceinline__ u64 mulhi_sb(u64 a, u64 b)
{
    u64 r;
    asm("v_mul_hi_u32 v60, %[al], %[bl]\n\t"
        "v_mov_b32 v61, 0\n\t"
        "v_mad_u64_u32 v[62:63], vcc, %[al], %[bh], v[60:61]\n\t"
        "v_mad_u64_u32 v[62:63], vcc, %[ah], %[bl], v[62:63]\n\t"
        "v_mad_u64_u32 v[66:67], s[96:97], %[ah], %[bh], 0\n\t"
        "v_lshrrev_b64 v[64:65], 32, v[62:63]\n\t"
        "v_addc_co_u32 v65, vcc, 0, v65, vcc\n\t"
        "v_lshl_add_u64 %[r], v[66:67], 0, v[64:65]"
        : [r] "=v"(r)
        : [al] "v"((u32)a), [ah] "v"((u32)(a >> 32)), [bl] "s"((u32)b), [bh] "s"((u32)(b >> 32))
        : PIE_ASM_CLOB, "s96", "s97");
    return r;
}
// a small integer v (< 2^30) times a residue c, into the columns
__device__ __forceinline__ void colacc_mac_small(ColAcc &a, u32 v, u64 c)
{
    const Split30 s = split30(c);
    a.c0 = mad_u(v, s.lo, a.c0);
    a.c1 = mad_u(v, s.hi, a.c1);
}

// the instruction-block forms of the helpers above where every modulus is below 2^60 (ASM), the compiler's otherwise
template <bool ASM>
__device__ __forceinline__ u64 mshoup(u64 a, u64 w, u64 wsh, u64 q, u64 negq)
{
    return ASM ? shoup63(a, w, wsh, negq) : mul_shoup_u(a, w, wsh, q, negq);
}
template <bool ASM>
__device__ __forceinline__ void mdivmod(u64 a, u64 w, u64 wsh, u64 q, u64 negq, u64 &quot, u64 &rem)
{
    if (ASM)
        divmod63(a, w, wsh, negq, quot, rem);
    else
        divmod_shoup_u(a, w, wsh, q, negq, quot, rem);
}
template <bool ASM>
__device__ __forceinline__ u64 mfixfrac(u64 y, const Mod &m)
{
    return ASM ? (mulhi_sb(y << m.fshift, m.fconst) >> 3) : fixfrac_u(y, m);
}

// sum_i y[i] * c[i] as a 128-bit integer.  MAD: carry-free column accumulators on v_mad_u64_u32 (madasm.h; needs all
// operands < 2^60 and NS <= 8), otherwise 64x64->128 multiplies.
template <u32 NS, bool MAD>
__device__ __forceinline__ U128 dot128(const u64 *y, const u64 (&c)[NS])
{
    if (MAD) {
        ColAcc a = {0, 0, 0};
#pragma unroll
        for (u32 i = 0; i < NS; i++) colacc_mac(a, split30(y[i]), split30(c[i]));
        return colacc_value(a);
    }
    U128 acc = {0, 0};
#pragma unroll
    for (u32 i = 0; i < NS; i++) mac128(acc, y[i], c[i]);
    return acc;
}

// centred CRT lift of y_i-weighted residues from a source basis into target modulus `tm`:
//   sum_i y_i * hat[i] - v * prodmod
// K: the arithmetic kind (modarith.h); the column-accumulator kinds (MAD) reduce by the Barrett or the folded block
// LZ (MAD only): the result stays in [0, 4q) (colacc_reduce123_lazy)
template <u32 NS, ArithKind K, bool LZ = false>
__device__ __forceinline__ u64 crt_out(const u64 *y, const u64 (&hat)[NS], u64 v, u64 prodmod, const Mod &tm, u64 negq, u64 neg2q)
{
    constexpr bool MAD = colacc(K), FD = K == ArithKind::fold;
    if (MAD && NS <= 7) {
        // MAD implies 2^59 < q < 2^60 for every modulus: up to 7 products plus the small term stay below 2^123; everything
        // goes through the column accumulator (v <= NS is one more, partial, term) and one reduction block
        ColAcc a = {0, 0, 0};
#pragma unroll
        for (u32 i = 0; i < NS; i++) colacc_mac(a, split30(y[i]), split30(hat[i]));
        colacc_mac_small(a, (u32)v, tm.q - prodmod);  // - v * prodmod (mod tm)
        return LZ ? colacc_red_lazy<FD>(a, tm, negq) : colacc_red<FD, false>(a, tm, negq);
    }
    U128 acc = dot128<NS, MAD>(y, hat);
    mac128(acc, v, tm.q - prodmod);  // - v * prodmod (mod tm); v <= ns: one Barrett reduction for the whole sum
    return reduce128(acc, tm);
}
// ... named by a bool, as tests/arith_check names the two kinds it checks this lift at: the 128-bit form or the Barrett block
template <u32 NS, bool MAD, bool LZ = false>
__device__ __forceinline__ u64 crt_out(const u64 *y, const u64 (&hat)[NS], u64 v, u64 prodmod, const Mod &tm, u64 negq, u64 neg2q)
{
    return crt_out<NS, MAD ? ArithKind::barrett : ArithKind::wide, LZ>(y, hat, v, prodmod, tm, negq, neg2q);
}

}  // namespace piehip
