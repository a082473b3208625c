// pie_convert.h -- the cores of the HPS base conversions and of the limb drop, and the body of one conversion (expand_body), for the
// product conversions of kernels_convert.hip and the chain-limb forms of kernels_chain_drop.hip.
#pragma once
#include "pie_kernel_common.h"

namespace piehip {

// ---------------------------------------------------------------------------------------------
// Base conversions (row A6).  One thread per coefficient reads its L (or 2L+1) residues at limb
// stride N and writes every output limb.  Rounding terms use the 60-bit fixed-point rule of
// modarith.h (identical to oracle/pie_oracle.c: po_expand_q_to_qp, po_scale_pq_expand, po_scale_round_tp).
// ---------------------------------------------------------------------------------------------
// The limb drop of limb_drop_kernel (kernels_chain_drop.hip) on the NP coefficient columns a thread holds, with the constants of the
// block that has all L limbs, read per dropped limb through the laundered pointer (the convention of pie_kernel_common.h).  S63 (every
// modulus below 2^60): the shoup63 instruction block; otherwise limb_drop_kernel's own product.  Only c[..][0 .. KEEP) are meaningful
// afterwards.
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

// The cases of launch_expand_pair (kernels.hpp) on a level context, in kernels_chain_drop.hip beside the kernels they launch: both
// operands plain, and the fused limb drop (y.src_L > L)
__attribute__((visibility("hidden"))) bool launch_expand_pair_plain(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y,
                                                                    u32 n_outer, u64 *out, hipStream_t st, Arith ar, bool fold);
__attribute__((visibility("hidden"))) bool launch_expand_pair_drop(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y,
                                                                   u32 n_outer, u64 *out, hipStream_t st, Arith ar, bool fold);

}  // namespace piehip
