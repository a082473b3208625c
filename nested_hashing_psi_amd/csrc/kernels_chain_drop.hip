// kernels_chain_drop.hip -- limb drops: of a result ciphertext, of the accumulators in front of the product chain (chain limbs), and
// fused into the load phase of a product's two base conversions; and those conversions on the plain operands the unfused drop leaves
// (pie_convert.h: drop_limbs, expand_body).
#include "pie_convert.h"

namespace piehip {

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

// launch_expand_pair's plain operands (x.plain and y.plain, neither dropped)
bool launch_expand_pair_plain(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y, u32 n_outer, u64 *out,
                              hipStream_t st, Arith ar, bool fold)
{
    const dim3 grid(((fold ? N / 2 : N) + TPB - 1) / TPB, n_outer * 4), block(TPB);
    // (a level context has fewer limbs than MAX_L)
    return !x.q_ready && with_u32<1, 6>(L, [&](auto L_) {
        with_arith(ar, [&](auto K_) {
            with_bools([&](auto F_) {
                hipLaunchKernelGGL((expand_both_plain_kernel<F_(), L_(), K_()>), grid, block, 0, st, dc, N, x.p, x.row, x.poly, y.p, y.row, y.poly,
                                   out, n_outer);
            }, fold);
        });
    });
}

// launch_expand_pair's fused limb drop (y.src_L > L): X is dropped too, or lies on this level with its Q limbs in place
bool launch_expand_pair_drop(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y, u32 n_outer, u64 *out,
                             hipStream_t st, Arith ar, bool fold)
{
    const bool xdrop = x.src_L > L;
    const dim3 grid(((fold ? N / 2 : N) + TPB - 1) / TPB, n_outer * 4), block(TPB);
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

}  // namespace piehip
