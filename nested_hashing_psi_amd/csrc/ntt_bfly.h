// ntt_bfly.h -- the 60-bit Shoup product, the lazy Harvey butterflies and the centred digit lift of kernels_ntt_fast.hip, in a
// header so that tests/arith_check compiles these definitions themselves.  Moved here word for word: kernels_ntt_fast.hip
// compiles to the same instructions as before (profiles/arith_blocks/).
#pragma once
#include "madasm.h"

namespace piehip {

// ---- 60-bit Shoup multiplication on the 32-bit multiplier ------------------------------------------
// v_mad_u64_u32 (32x32+64 -> 64) issues at twice the rate of v_mul_lo_u32 / v_mul_hi_u32 on gfx950, and
// hipcc narrows every 64-bit product whose high half is unused to v_mul_lo_u32; inline asm keeps
// the whole butterfly on the mad.  9 mads per modular multiplication:
//   quotient estimate  qe = floor(b ws / 2^64) - {0,1,2}   from 3 partial products (b_lo ws_lo dropped)
//   remainder          b w + qe (2^64 - q)  mod 2^64       as two accumulation chains (low word, cross terms)
// ws here is the 63-bit constant floor(w 2^63 / q) (= the usual Shoup constant >> 1) so that the sum of the
// two cross products cannot overflow 64 bits for b < 2^63; qe = 2 bh sh + (bh sl + bl sh) >> 31 under-
// estimates floor(b w / q) by at most 3.  The result lies in [0, 4q); with q < 2^60 the butterflies keep
// residues in [0, 8q) (forward) or [0, 4q) (inverse) and normalise once at the end of the transform.
// b < 2^63, w < q, ws = floor(w 2^63 / q), nq = 2^64 - q: returns b w mod q + {0,1,2,3} q
__device__ __forceinline__ u64 shoup4(u64 b, u64 w, u64 ws, u64 nq)
{
    const u32 bl = (u32)b, bh = (u32)(b >> 32), wl = (u32)w, wh = (u32)(w >> 32);
    const u32 sl = (u32)ws, sh = (u32)(ws >> 32), nql = (u32)nq, nqh = (u32)(nq >> 32);
    const u64 m1 = mul_u(bl, sh);          // < 2^63  (sh < 2^31: ws is the 63-bit Shoup constant)
    const u64 cr = mad_u(bh, sl, m1);      // both cross terms, < 2^64 for b < 2^63
    const u64 top = mul_u(bh, sh);
    const u64 qe = (top << 1) + (cr >> 31);
    u64 acc = mul_u((u32)qe, nql);
    acc = mad_u(bl, wl, acc);
    u64 c = mul_u((u32)qe, nqh);
    c = mad_u((u32)(qe >> 32), nql, c);
    c = mad_u(bl, wh, c);
    c = mad_u(bh, wl, c);
    return acc + ((u64)(u32)c << 32);
}

// Harvey butterflies on lazy residues ------------------------------------------------------------------------
// forward: inputs in [0, 8q), outputs in [0, 8q)
__device__ __forceinline__ void ct_bfly(u64 &a, u64 &b, u64 w, u64 ws, u64 nq, u64 q4)
{
    const u64 u = a >= q4 ? a - q4 : a;
    const u64 v = shoup4(b, w, ws, nq);
    a = u + v;
    b = u - v + q4;
}
// inverse: inputs in [0, 4q), outputs in [0, 4q)
__device__ __forceinline__ void gs_bfly(u64 &a, u64 &b, u64 w, u64 ws, u64 nq, u64 q4)
{
    const u64 s = a + b;
    const u64 d = a - b + q4;
    a = s >= q4 ? s - q4 : s;
    b = shoup4(d, w, ws, nq);
}

// centred lift of a residue mod q_i into q_j (same rule as digits_kernel / oracle keyswitch_acc)
__device__ __forceinline__ u64 lift_digit(u64 v, u64 qi, u64 qi_mod_qj, const Mod &mj)
{
    // v < q_i; when q_i < 2 q_j (every chain of equal-width primes) one conditional subtraction reduces it
    u64 r = (qi < 2 * mj.q) ? (v >= mj.q ? v - mj.q : v) : barrett128(0, v, mj);
    if (v > qi / 2) r = submod(r, qi_mod_qj, mj.q);
    return r;
}

}  // namespace piehip
