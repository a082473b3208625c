// kernels_keyswitch.hip -- a ciphertext multiplication behind its base conversions: tensor product over QP, scale-and-round by t/P,
// BV digit decomposition, key-switch accumulation with the mask multiply, and the finish of a degree-2 result.  One thread per
// coefficient or coefficient pair, constants scalar-loaded from one DevConsts block.
#include "pie_kernel_common.h"

namespace piehip {

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

}  // namespace piehip
