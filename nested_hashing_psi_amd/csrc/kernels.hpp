// kernels.hpp -- launch wrappers of the gfx950 kernels behind the C ABI (include/piehip.h).
// Every wrapper only enqueues on `st`; none allocates or synchronises (graph-capturable).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "params.hpp"

namespace piehip {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: one bit per device ordinal and kernel instantiation,
// so that handles on several devices of one process each raise the limit where they launch.
struct PerDeviceOnce {
    std::atomic<unsigned long long> done{0};
    bool first_on_current_device()
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;
        const unsigned long long bit = 1ULL << dev;
        return (done.fetch_or(bit) & bit) == 0;
    }
};

// Which transform kernel a call takes: radix-2 stages in LDS (kernels_ntt.hip), 32 coefficients per thread (kernels_ntt_fast.hip),
// 16 coefficients per thread (ntt16_kernel.h, kernels_ntt16.hip).  DESIGN.md section 5a is the table; ntt_route() implements it.
enum class NttKernel { radix2, blocked32, blocked16 };
struct NttRoute {
    NttKernel kernel;
    u32 s0;             // log2 of the slices per limb
    u32 global_stages;  // outermost stages run in global memory around the slice kernel (a folded call has none: its neighbours apply it)
    bool extra() const { return kernel != NttKernel::radix2 && !global_stages; }  // the call honours NttExtra
};

// Device-resident NTT tables (for modulus a, tables + a*4*N holds tw | tw_sh | itw | itw_sh, N each) and what the context does with
// them: every field below max_slots is decided once, by ntt_plan_decide() in piehip_create, and only read afterwards.
struct NttPlan {
    const u64 *tables;
    const u64 *twp;       // interleaved {w, w_shoup} pairs: per modulus [fwd N pairs][inv N pairs]
    const u64 *twc = nullptr;       // 32-coefficient kernel, pass-C twiddles in kernel order: per modulus [fwd][inv], see build_twc_table
    const u64 *twc_fold = nullptr;  // ... for two folded half-size slices per limb (fold)
    const u64 *twk16 = nullptr;     // 16-coefficient kernel: kernel-ordered pairs of passes 3, 4 for the slices of its lane order
    const DevConsts *dc;  // device pointer
    u32 N, logN;
    u32 num_cus;
    u32 max_slots = 0;    // piehip_set_transform_slots: cap on the persistent transform grids (workgroups), 0 = every slot
    bool lane_order = false;     // the register-blocked kernels apply: arrays that stay inside the library keep their EVALUATION side as
                                 // the threads of lane_kernel hold it (sigma), keys and masks have lane-ordered copies
    bool fold = false;           // lane-ordered transforms run as two half-size slices per limb; the neighbouring coefficient-wise
                                 // kernels apply the outermost stage (pie_kernel_common.h "Outer-stage folding")
    NttKernel lane_kernel = NttKernel::radix2;  // the kernel that defines the lane order
    u32 lane_logn = 0;           // log2 of its slice length,
    u32 lane_T = 0;              // its threads per slice
    u32 lane_kp = 16;            // and coefficient pairs per thread (16: kernels_ntt_fast.hip, 8: ntt16_kernel.h)
    bool small_moduli = false;   // every Q and P modulus lies in (2^59, 2^60): v_mad_u64_u32 column accumulators, one-word Barrett
    bool fold_moduli = false;    // ... and is 2^60 - d with d < COLACC_FOLD_MAX_D (the default chains): the base conversions, scale-and-
                                 // round and the tensor load phase reduce their column sums by folding with d (stage_a_common.h)
    u32 fold_mod_count = 0;      // ... the moduli [0, fold_mod_count) that says it of (Q and P, not the plaintext modulus behind them): a
                                 // launch of the 16-coefficient transform on moduli inside takes the folding butterflies (ntt16_kernel.h)
    // schedule switches derived from the above (piehip_run.cpp)
    bool xq_reuse = false;         // the inverse transform of operand X drops a lane-ordered copy into the QP array, the forward skips it
    bool x_direct = false;         // stage A of a query batch may write X there in the first place (StageAXOut)
    bool fused_tensor = false;     // launch_ntt16_tensor instead of launch_tensor + inverse transform
    bool d01_eval_q = false;       // relinearising product: the Q limbs of d0, d1 stay in EVALUATION form -- not inverse-
                                   // transformed, not seen by scale-and-round; the key-switch MAC forms c_k (a (x) b)_k from the QP operands
    bool result_eval_q = false;    // a product that is NOT relinearised (the last one of a run() with piehip_set_result_relin(0)): no Q limb of
                                   // d0, d1, d2 is inverse-transformed; launch_deg2_finish forms the three own-limb terms from the QP operands
    bool digits_with_d01 = false;  // the key-switch digits join the forward launch of d0, d1 (Ntt16Digits)
    bool digit_lift_lane = false;  // launch_ntt_digits instead of launch_digits + transform: lane-ordered key switches,
    bool digit_lift_std = false;   // ... standard-order key switches (FHEHIPPIE, piehip_eval_automorph)
    // CUs the persistent transform grids may fill (two workgroup slots of 512 threads, or one of 1024, per CU)
    u32 transform_cus() const
    {
        if (!max_slots) return num_cus;
        const u32 c = (max_slots + 1) / 2;
        return c < num_cus ? (c ? c : 1u) : num_cus;
    }
};
// fills in everything from lane_order on, from N / logN and the three facts about the moduli: lazy_ok -- every modulus, t included, is
// below 2^60 (lazy residues need 8q < 2^63) --, small_moduli and fold_moduli (kept only with small_moduli)
void ntt_plan_decide(NttPlan &pl, bool lazy_ok, bool small_moduli, bool fold_moduli = false);
// q = 2^60 - d takes the folded block for d below this: the largest d its bound proof supports at z < 2^124 (2^28 at z < 2^123)
static const u64 COLACC_FOLD_MAX_D = 1ull << 27;
// The arithmetic kind (ArithKind, modarith.h) a launcher runs its kernel at: every kernel that reduces variable x variable column sums
// takes the kind as one template argument, and the launchers turn this run-time value into it (with_arith, pie_kernel_common.h).  The
// library passes its plans; tests/lazy_inputs builds an Arith from the plan or, explicitly, from its option fd=, and prints the kind
// that ran (DESIGN.md section 5a lists who holds which kind).
// mad, fold: the kind read as the two questions a caller may ask of it -- column accumulators at all? the folded block? --, fixed with
// the kind by the one constructor: tests/lazy_inputs prints the kind that ran from them.  The launchers dispatch on `kind` alone.
struct Arith {
    const ArithKind kind;
    const bool mad, fold;
    explicit Arith(bool small_moduli, bool fold_moduli = false)
        : kind(!small_moduli ? ArithKind::wide : fold_moduli ? ArithKind::fold : ArithKind::barrett), mad(colacc(kind)), fold(kind == ArithKind::fold) {}
    Arith(const NttPlan &pl) : Arith(pl.small_moduli, pl.fold_moduli) {}
};
// sigma, folded: as for launch_ntt.  Requires sigma <= pl.lane_order and folded <= pl.fold (the callers' wrappers mask them)
NttRoute ntt_route(const NttPlan &pl, bool inverse, bool sigma, bool folded);

// host side of piehip_create: kernel-ordered twiddles of one (modulus, direction) from its natural-order {w, w_shoup} pairs, and the
// map lane-order position -> standard position, for the 32-coefficient kernel (s0 = ~0u: no lane order, identity) and the 16-coefficient one
void build_twc_table(const u64 *nat_pairs, u32 logN, u32 s0, std::vector<u64> &out);
void build_twk16_table(const u64 *nat_pairs, u32 s0, u32 slice_log, std::vector<u64> &out);  // slices of 2^13 or 2^14
void ntt_sigma_inverse_map(u32 logN, u32 s0, std::vector<u32> &map);
void ntt16_sigma_inverse_map(u32 logN, u32 s0, std::vector<u32> &map);
// Optional extras of the register-blocked kernels (ciphertext multiplication), honoured where NttRoute::extra() -- elsewhere launch_ntt
// drops the copy and the compact enumeration (the copy array is not written) and keeps lazy_out, which the slice kernel of a route
// with global stages honours as well (it stores last):
//   inverse, standard order in:  limbs [nb][copy_K][2][copy_L]; the lane-ordered EVALUATION input of operand 0 of every
//                                bin is also written to the Q limbs of copy_out[nb][4][copy_M][N] (slots 0, 1)
//   forward, lane order:         lazy_out -- no final normalisation
//   forward:                     nlimbs counts a compact enumeration of [nb][4][skip_M] that omits limbs < skip_L of
//                                slots 0 and 1 (they already hold EVALUATION data)
struct NttExtra {
    u64 *copy_out = nullptr;
    u32 copy_K = 1, copy_L = 1, copy_M = 1;
    u32 skip_L = 0, skip_M = 0;
    bool lazy_out = false;  // forward, lane order: leave the residues in [0, 8q) (the consumer reduces anyway)
    bool x_lane_in = false; // 16-coefficient kernel, inverse, standard order in: the operand-0 polynomials are READ, lane-ordered, from
                            // where copy_out would have put them (stage A wrote them there: StageAXOut) and nothing is copied
};
// In-place negacyclic NTT over `nlimbs` limbs [nlimbs][N]; limb i uses modulus mod_base + i % mod_count.
// (replaces DCRTPoly::SetFormat under BatchedFHEHIPPIE.cpp:123)
// sigma: the EVALUATION side is in the plan's lane order (internal arrays only); folded: the outermost stage is NOT done here, the
// limb is transformed as two independent half-size slices.  The kernel follows from ntt_route().
void launch_ntt(const NttPlan &pl, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inverse, hipStream_t st,
                bool sigma = false, bool folded = false, const NttExtra *ex = nullptr);
// The launchers below are what launch_ntt dispatches to; the schedule calls them directly only for the fusions, and only where
// the plan's switch says so (they assert it).
void launch_ntt_fast(const NttPlan &pl, const u64 *twc, u32 s0, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inverse,
                     bool sigma, hipStream_t st, const u64 *lift_src = nullptr, u32 lift_L = 0, const NttExtra *ex = nullptr);
// dg (forward, lane order, mod_base 0, mod_count L; pl.digits_with_d01): the BV key-switch digits of nb polynomials join the launch --
// limb (bin, i, j) of dig[nb][L][L][N] = transform of the centred lift into q_j of residue limb i of the COEFFICIENT polynomial
// d2 + bin * stride2 (replaces launch_digits + a second transform launch)
struct Ntt16Digits {
    const u64 *d2;
    size_t stride2;
    u64 *dig;
    u32 nb, L;
};
void launch_ntt16(const NttPlan &pl, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inverse, bool sigma, hipStream_t st,
                  const NttExtra *ex, const Ntt16Digits *dg = nullptr);
// pl.fused_tensor: the tensor product in the load phase of the inverse transform that follows it: e[nb][4][M][N] (a0 a1 b0 b1,
// EVALUATION, lane order, [0, 8q) residues) -> d[nb][3][M][N] in COEFFICIENT format, as launch_tensor +
// launch_ntt(d, nb * 3 * M, 0, M, inverse, sigma, fold) leave it.  -DPIEHIP_FUSE_TENSOR=0 clears the switch (two launches, for A/B runs)
#ifndef PIEHIP_FUSE_TENSOR
#define PIEHIP_FUSE_TENSOR 1
#endif
// eval_q_L = L (pl.d01_eval_q, relinearising products): the Q limbs (< L) of d0 and d1 are not produced -- 3 M - 2 L limbs per row; their
// places in d[nb][3][M][N] are not written.  -DPIEHIP_D01_EVAL_Q=0 clears that switch
#ifndef PIEHIP_D01_EVAL_Q
#define PIEHIP_D01_EVAL_Q 1
#endif
// eval_q_d2 (pl.result_eval_q, with eval_q_L = L): the Q limbs of d2 are not produced either -- 3 (M - L) limbs per row.
// -DPIEHIP_RESULT_EVAL_Q=0 clears that switch
#ifndef PIEHIP_RESULT_EVAL_Q
#define PIEHIP_RESULT_EVAL_Q 1
#endif
void launch_ntt16_tensor(const NttPlan &pl, const u64 *e, u64 *d, u32 nb, u32 M, hipStream_t st, u32 eval_q_L = 0, bool eval_q_d2 = false);
// pl.digit_lift_lane / digit_lift_std: forward transform of the BV digits with the digit lift in the 32-coefficient kernel's load
// phase (no digits kernel): d2[nb][L][N] COEFFICIENT -> dig[nb][L(i)][L(j)][N] EVALUATION
void launch_ntt_digits(const NttPlan &pl, const u64 *d2, u64 *dig, u32 nb, u32 L, bool sigma, hipStream_t st);

// Stage A of 1 <= nq <= STAGE_A_MAX_QUERIES queries on one database:
// acc[b][nq][K][2][L][N] = sum_j idx_q[h][j] (.) db[h][beta][j] + minus_q    (BatchedFHEHIPPIE.cpp:101-116)
// A batch goes through stage_a_tiled_kernel in groups of two to four queries, each group reading the database once (a group of three
// on a ring that fills the chip through stage_a_resident_kernel: stage_a_resident_lpp of stage_a_common.h); a single query through
// stage_a_mad_kernel or, on the 128-bit arithmetic, stage_a_kernel.
// small_moduli: every RNS modulus is in (2^59, 2^60) (the v_mad_u64_u32 column accumulators; 128-bit accumulators otherwise)
// bstride: bin-layer count of the database array db[K][bstride][E][L][N] when only b <= bstride layers (starting at the
// layer db points to) are evaluated; 0 = b.  h0, hn: only the inner hash functions [h0, h0 + hn) (hn = 0: all from h0)
// xo (column accumulators only): the accumulators of inner hash function 0 -- operand X of the first ciphertext product --
// are not written to acc but, lane-ordered (ntt16_kernel.h), into the Q limbs of the QP operand array xo->out[row][4][M][N],
// slots 0, 1: where the tensor product reads them.  The inverse transform then takes them from there (NttExtra::x_lane_in)
// instead of writing that copy itself.
struct StageAXOut {
    u64 *out = nullptr;
    u32 M = 0, logns = 0;  // limbs per polynomial of the QP array; log2 of the transform's slice length
};
static const u32 STAGE_A_MAX_QUERIES = 8;
struct StageAQueries {
    const u64 *idx[STAGE_A_MAX_QUERIES];
    const u64 *minus[STAGE_A_MAX_QUERIES];
};
void launch_stage_a_batch(const DevConsts *dc, u32 N, u32 L, u32 K, u32 b, u32 E, const StageAQueries &qs, u32 nq, const u64 *db,
                          u64 *acc, hipStream_t st, bool small_moduli, u32 bstride = 0, u32 h0 = 0, u32 hn = 0,
                          const StageAXOut *xo = nullptr);

// Base conversions, COEFFICIENT format.  Polynomial (o, c), o < n_outer, c < 2,
// is read at in + o*in_stride_outer + c*in_stride_inner ([L][N] limbs, canonical, nothing pending) and written to
// out + ((o*out_polys + out_slot + c)*M)*N ([M][N] limbs): every limb, no folding (piehip_base_convert)
// small_moduli (here and below): NttPlan::small_moduli of the context -- selects the v_mad_u64_u32 / one-word Barrett variants
// ar (here and below): the context's arithmetic kind (Arith: callers pass the plan)
void launch_expand_q_to_qp(const DevConsts *dc, u32 N, u32 L, const u64 *in, size_t in_stride_outer,
                           size_t in_stride_inner, u32 n_outer, u64 *out, u32 out_polys, u32 out_slot, hipStream_t st,
                           Arith ar);
void launch_scale_pq_expand(const DevConsts *dc, u32 N, u32 L, const u64 *in, size_t in_stride_outer,
                            size_t in_stride_inner, u32 n_outer, u64 *out, u32 out_polys, u32 out_slot, hipStream_t st,
                            Arith ar);
// Both conversions of a ciphertext multiplication in one launch, on the context (dc, L limbs, M = 2 L + 1; small_moduli and fold: its
// plan's): X centred-lifted into slots 0, 1 of out[n_outer][4][M][N], Y scaled by P/Q into slots 2, 3.  fold: the outermost stage of
// the forward transform that follows is applied on the store side (pie_kernel_common.h, "Outer-stage folding").
// An operand: polynomial c of row o at p + o*row + c*poly, COEFFICIENT format, and how it arrives --
//   neither of the below   as the context's inverse transform left it: [L][N] limbs; with fold the outer stage is pending, [0, 4q) residues
//   plain                  [L][N] limbs, canonical, nothing pending even where the context folds (launch_chain_drop, an unfolded inverse
//                          transform): a product on a level context, L < MAX_L
//   src_L > L              chain limbs, fused: [src_L][N] limbs as the folded inverse transform of the level with src_L limbs left them
//                          (src_dc: that level's constants); dropped to L limbs in the load phase.  Folded rings with every modulus in
//                          (2^59, 2^60), and (Y's, X's, L) a combination expand_drop_built knows
//   q_ready (X only)       the Q limbs of X in `out` already hold its EVALUATION form (NttExtra, StageAXOut) and are left alone
// Built: both pending on one polynomial distance, L <= MAX_L, with fold only where X is q_ready (a folding plan has xq_reuse); both
// plain; Y dropped with X dropped from Y's level (under Y's constants) or another, or with X pending and q_ready.  false, nothing
// launched, for anything else.
struct ExpandOperand {
    const u64 *p = nullptr;
    size_t row = 0, poly = 0;
    const DevConsts *src_dc = nullptr;
    u32 src_L = 0;
    bool plain = false;
    bool q_ready = false;
};
bool launch_expand_pair(const DevConsts *dc, u32 N, u32 L, const ExpandOperand &x, const ExpandOperand &y, u32 n_outer, u64 *out,
                        hipStream_t st, Arith ar, bool fold);
// the first case by its parts: both pending on the context's own level, rows sx and sy apart, polynomials si (lazy_inputs_check)
inline bool launch_expand_both(const DevConsts *dc, u32 N, u32 L, const u64 *x, size_t sx, const u64 *y, size_t sy, size_t si, u32 n_outer,
                               u64 *out, hipStream_t st, Arith ar, bool fold = false, bool skip_q = false)
{
    ExpandOperand xo, yo;
    xo.p = x, yo.p = y;
    xo.row = sx, yo.row = sy, xo.poly = yo.poly = si;
    xo.q_ready = skip_q;
    return launch_expand_pair(dc, N, L, xo, yo, n_outer, out, st, ar, fold);
}
// is the fused form built for Y on Ly limbs and X on Lx (Lx <= Lc: X is not dropped), both to Lc?  (-DPIEHIP_CHAIN_DROP_FUSED=0: never)
bool expand_drop_built(u32 Ly, u32 Lx, u32 Lc);
// e[nb][4][M][N] (a0 a1 b0 b1, EVALUATION) -> d[nb][3][M][N]
void launch_tensor(const DevConsts *dc, u32 N, u32 M, const u64 *e, u64 *d, u32 nb, hipStream_t st, bool small_moduli);
// d[nb][3][M][N] (COEFFICIENT) -> components 0,1 to out01 + bin*stride01 + c*L*N, component 2 to out2 + bin*stride2
// fold: the outermost NTT stage of the neighbouring transforms is applied here (see pie_kernel_common.h, "Outer-stage
// folding"); fold_comp2: component 2 also feeds a forward transform directly (3-component output)
// p_only2 (pl.result_eval_q, with p_only01 and fold_comp2): component 2 likewise -- the product is not relinearised, launch_deg2_finish
// adds all three terms
// p_only01 (pl.d01_eval_q): components 0 and 1 are computed from their P limbs alone -- the Q limbs of d are not read and the own-limb
// term d_k [t P^-1]_{q_k} is left out (the key-switch MAC adds its transform: launch_relin_mac, eqp)
void launch_scale_round(const DevConsts *dc, u32 N, u32 L, const u64 *d, u32 nb, u64 *out01, size_t stride01, u64 *out2,
                        size_t stride2, hipStream_t st, Arith ar, bool fold = false, bool fold_comp2 = false, bool p_only01 = false,
                        bool p_only2 = false);
// BV digits: d2c at d2 + bin*stride2 ([L][N], COEFFICIENT) -> dig[nb][L(i)][L(j)][N] (centred lift of residue i into q_j)
void launch_digits(const DevConsts *dc, u32 N, u32 L, const u64 *d2, size_t stride2, u32 nb, u64 *dig, hipStream_t st,
                   bool fold = false);
// out[bin][c][j] = (d01[bin][c][j] + sum_i dig[bin][i][j] (.) key[i][c][j]) (.) mask[bin][j]   (mask may be null)
// out_map (may be null): coefficient n of the result is written to position out_map[n] (lane order -> standard)
// key_group > 1: ciphertext `bin` uses key + (bin % key_group) * key_stride (EvalMerge: one rotation key per position)
// mask_div > 1: ciphertext `bin` takes mask[bin / mask_div] (a query batch: mask_div queries per bin layer)
// sigma_T != 0: out_map is the lane order of a transform with sigma_T threads per slice and sigma_kp coefficient pairs per thread
// (16: kernels_ntt_fast.hip, 8: ntt16_kernel.h); stores then go through an LDS tile
// eqp (pl.d01_eval_q; null: off): the QP operands e[nb][4][eqp_M][N] (a0 a1 b0 b1, EVALUATION, ordered like d01, [0, 8q) residues) of the
// product whose d0, d1 arrive without their own-limb term: [t P^-1]_{q_j} a0 b0 is added to component 0, ... (a0 b1 + a1 b0) to component 1
void launch_relin_mac(const DevConsts *dc, u32 N, u32 L, const u64 *d01, size_t stride01, const u64 *dig, const u64 *key,
                      const u64 *mask, u64 *out, u32 nb, hipStream_t st, bool small_moduli, const u32 *out_map = nullptr, size_t key_stride = 0,
                      u32 key_group = 1, u32 sigma_T = 0, u32 sigma_kp = 16, u32 mask_div = 1, const u64 *eqp = nullptr, u32 eqp_M = 0);
// Degree-2 results (pl.result_eval_q): out[row][c][j] = (d[row][c][j] + [t P^-1]_{q_j} (a (x) b)[c][j]) (.) mask[row / mask_div][j] for the
// three components c of a product that is not relinearised.  d[nb][3][L][N] and mask are lane-ordered (sigma_T threads per slice,
// sigma_kp pairs per thread: deg2_finish_applies says whether the kernel takes that order), d in [0, 8q); eqp as for launch_relin_mac;
// out[nb][3][L][N] leaves in standard order, canonical
bool deg2_finish_applies(u32 N, u32 sigma_T, u32 sigma_kp);
void launch_deg2_finish(const DevConsts *dc, u32 N, u32 L, const u64 *d, const u64 *eqp, u32 eqp_M, const u64 *mask, u64 *out, u32 nb,
                        hipStream_t st, u32 sigma_T, u32 sigma_kp, u32 mask_div = 1);
// rotation-based PIE (FHEHIPPIE.cpp:61-77), see kernels_pie.hip
void launch_bcast_mul_plain(const DevConsts *dc, u32 N, u32 L, const u64 *x, size_t xs, u32 group, const u64 *pt, size_t ps_outer,
                            size_t ps_inner, u64 *out, u32 nct, hipStream_t st);
void launch_rot_prepare(const DevConsts *dc, u32 N, u32 L, const u64 *x, const u32 *maps, u32 map_group, bool acc, bool identity_first,
                        u64 *d01, u64 *d2, u32 nct, hipStream_t st);
void launch_sum_mul_plain(const DevConsts *dc, u32 N, u32 L, const u64 *x, u32 group, const u64 *pt, size_t pt_stride, u64 *out,
                          size_t out_stride, u32 ngroups, hipStream_t st);
// writes `value` to a word of page-locked host memory (its device address) behind everything queued on `st` so far
void launch_host_flag(u64 *flag_dev, u64 value, hipStream_t st);
// element-wise helpers on nct ciphertexts [nct][2][L][N]
void launch_ct_add(const DevConsts *dc, u32 N, u32 L, const u64 *x, const u64 *y, u64 *out, u32 nct, hipStream_t st);
// (pt_div > 1: ciphertext i takes plaintext i / pt_div; comps: components per ciphertext, 3 for a product that was not relinearised)
void launch_ct_mul_plain(const DevConsts *dc, u32 N, u32 L, const u64 *x, const u64 *pt, size_t pt_stride, u64 *out,
                         u32 nct, hipStream_t st, u32 pt_div = 1, u32 comps = 2);
// limb drop of npoly polynomials in COEFFICIENT format: in[npoly][L][N] -> out[npoly][keep][N], the limbs L - 1 .. keep dropped one
// after the other with centred rounding (include/piehip.h "Result limbs").  1 <= keep < L <= MAX_L; false (nothing launched) otherwise
bool launch_limb_drop(const DevConsts *dc, u32 N, u32 L, u32 keep, const u64 *in, u64 *out, u32 npoly, hipStream_t st);
// ---- chain limbs (include/piehip.h "Chain limbs"; kernels_chain_drop.hip) -----------------------------------------------------------
// The limb drop in front of the product chain, on npoly polynomials data[npoly][L][N] in COEFFICIENT format as the parent's inverse
// transform left them (fold: outer stage pending): IN PLACE, the first `keep` limbs of every polynomial become the dropped
// polynomial's, canonical, nothing pending; the limbs behind them are left alone.  1 <= keep < L <= MAX_L; false otherwise
// per, gstride: the polynomials lie in groups of `per` neighbours, gstride words from group to group (0: one packed array)
bool launch_chain_drop(const DevConsts *dc, u32 N, u32 L, u32 keep, u64 *data, u32 npoly, hipStream_t st, bool fold, u32 per = 0,
                       size_t gstride = 0);
// out[r][p] = in[r][map[p]] for nrows limbs
void launch_permute(u32 N, const u64 *in, const u32 *map, u64 *out, u32 nrows, hipStream_t st);
// packed encoding: slots[npt][B] -> u[npt][N] residues mod t at their EVALUATION positions
void launch_encode_scatter(const DevConsts *dc, u32 N, u32 M, const int64_t *slots, u32 B, const u32 *inv_pos, u64 *u,
                           u32 npt, hipStream_t st);
// coefficients mod t [npt][N] -> centred lift into every q_i: out[npt][L][N]
// l0 (the query-sliced database: one limb per plaintext): into the L moduli from q_l0 on
void launch_encode_lift(const DevConsts *dc, u32 N, u32 L, u32 M, const u64 *u, u64 *out, u32 npt, hipStream_t st, u32 l0 = 0);

// ---- query-sliced stage A (kernels_slice.hip; include/piehip.h "Query slices") ----------------------------------------------
// Unit u = h L + l is limb l of inner hash function h; a handle holds the units [u_lo, u_lo + un) as one-limb arrays.
//   db   [un][b][E][N]                       the database plaintexts' limbs
//   idx  [un][E][2][N], minus [un][2][N]     per query: the index ciphertexts' and the minus element's limbs
//   acc  [b][nq][un][2][N]                   = sum_j idx[u][j] (.) db[u][beta][j] + minus[u], canonical, EVALUATION format
// The arithmetic of launch_stage_a_batch (column accumulators where small_moduli, 128-bit otherwise); one launch per
// group of one to four queries whatever b.
void launch_stage_a_slice(const DevConsts *dc, u32 N, u32 L, u32 u_lo, u32 un, u32 b, u32 E, const StageAQueries &qs, u32 nq,
                          const u64 *db, u64 *acc, hipStream_t st, bool small_moduli);
// Placement: the rows of bin layers [bin_lo, bin_lo + bn) of src[b][nq][un][2][N] (units from u_lo) into the chain side's
// acc[bn][nq][K][2][L][N]; with xo, the units of inner hash function 0 go, lane-ordered, into the Q limbs of the QP operand array
// instead (where stage A of an unsliced batch puts them: StageAXOut)
void launch_place_accumulators(u32 N, u32 L, u32 K, u32 u_lo, u32 un, u32 bin_lo, u32 bn, u32 nq, const u64 *src, u64 *acc,
                               const StageAXOut *xo, hipStream_t st);
// ... of all K L units in one launch, each from the block that holds it: unit u is unit u - u_lo of base[row0 + rows][un][2][N]
// (row = bin layer x query of the chain side; row0: the block's row that is the chain side's first).  K L <= PLACE_MAX_UNITS
static const u32 PLACE_MAX_UNITS = 64;
struct PlaceSource {
    const u64 *base;
    u32 row0, u_lo, un;
};
struct PlaceSources {
    PlaceSource of[PLACE_MAX_UNITS];
};
void launch_place_units(u32 N, u32 L, u32 K, u32 rows, const PlaceSources &src, u64 *acc, const StageAXOut *xo, hipStream_t st);

// ---- offline phase: nested hashing and database gather on the device (kernels_hash.hip) -----------------------
size_t hash_sort_temp_bytes(u32 n, u32 e);
hipError_t launch_hash_build(const u64 *d_tab, const u64 *d_items, u32 n, u32 k, u32 e, u32 K, u32 b, u32 E, u64 evict_seed,
                             u64 shuffle_seed, u64 *d_tbl, u32 *d_keys, u32 *d_vals, u32 *d_start, void *d_temp, size_t temp_bytes,
                             u32 *d_fail, hipStream_t st);
void launch_shuffle_rows(u64 *d_tbl, u32 rows, u32 b, u32 E, u64 seed, hipStream_t st);
void launch_gather_slots(const u64 *d_tbl, u32 B, u32 K, u32 b, u32 E, u64 t, int64_t *d_slots, u32 *d_fail, hipStream_t st);
// R bin layers per slot vector: d_slots[K][ceil(b / R)][E][R B], zero behind the last layer (include/piehip.h "Layer tiling")
void launch_gather_slots_tiled(const u64 *d_tbl, u32 B, u32 R, u32 K, u32 b, u32 E, u64 t, int64_t *d_slots, u32 *d_fail, hipStream_t st);
void launch_mask_slots(u64 t, u32 b, u32 B, u64 seed, int64_t *d_out, hipStream_t st);

// ---- client harness (kernels_client.hip) ----------------------------------------------------------------------------
void launch_enc_message(const DevConsts *dc, u32 N, u32 L, u32 M, const u64 *coeff_t, const int32_t *e, u64 *em, u32 nct, hipStream_t st);
void launch_enc_finish(const DevConsts *dc, u32 N, u32 L, const u64 *em, const u64 *sk, const u64 *a_in, u64 *out, u32 nct,
                       hipStream_t st);
void launch_ks_finish(const DevConsts *dc, u32 N, u32 L, const u64 *e, const u64 *sk, const u64 *s_from, u64 *ks, hipStream_t st);
void launch_square(const DevConsts *dc, u32 N, u32 L, const u64 *s, u64 *s2, hipStream_t st);
void launch_dec_dot(const DevConsts *dc, u32 N, u32 L, const u64 *ct, const u64 *sk, u64 *xs, u32 nct, hipStream_t st, u32 ncomp = 2);
void launch_dec_round(const DevConsts *dc, u32 N, u32 L, u32 M, const u64 *xs, u64 *coeff_t, u32 nct, hipStream_t st);
void launch_dec_round_budget(const DevConsts *dc, u32 N, u32 L, u32 M, const u64 *xs, u64 *coeff_t, u64 *max_dist, u32 nct,
                             hipStream_t st);
void launch_decode_gather(const DevConsts *dc, u32 N, u32 M, const u64 *u, const u32 *slot_pos, u32 B, int64_t *slots, u32 nct,
                          hipStream_t st);

// Seeded ciphertexts (kernels_seed.hip): job j regenerates the uniform polynomial of its 32-byte seed, a[L][N] in EVALUATION word
// order, into dst[L][N] (e.g. the c1 half of a ciphertext inside an index matrix [K][E][2][L][N]).  jobs is a device array;
// more than SEED_MAX_JOBS_PER_LAUNCH jobs take several launches.
struct SeedJob {
    u64 *dst;
    u32 seed[8];   // the seed's 32 bytes as little-endian words
};
static const u32 SEED_MAX_JOBS_PER_LAUNCH = 65535;
void launch_expand_uniform(const DevConsts *dc, u32 N, u32 L, const SeedJob *jobs, u32 njobs, hipStream_t st);
// Limb-selective expansion: job j regenerates limb `limb` of its seed's polynomial -- row `limb` of what a SeedJob writes, bit for
// bit -- into the one row dst[N] and writes nothing behind it (the c1 rows of a query slice, idx[u_n][E][2][N] and minus[u_n][2][N]:
// the next row there is the c0 of the next ciphertext).  limb < L; the same job limit per launch.
struct SeedLimbJob {
    u64 *dst;      // one row of N words
    u32 seed[8];
    u32 limb;
};
void launch_expand_uniform_limb(const DevConsts *dc, u32 N, const SeedLimbJob *jobs, u32 njobs, hipStream_t st);

}  // namespace piehip
