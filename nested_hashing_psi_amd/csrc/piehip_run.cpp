// piehip_run.cpp -- the launch schedule of BatchedFHEHIPPIE::run() (reference BatchedFHEHIPPIE.cpp:88-129) on the handle's queues:
// the schedule pieces of a ciphertext multiplication, the queues of a run and the bin layers each takes, piehip_run_into.
#include <cassert>

#include "piehip_ctx.hpp"

using namespace piehip;

namespace piehip {

// ---- schedule pieces ----------------------------------------------------------------------------
// What a context does where -- which transform kernel, which fusions -- is decided once, in its plan.  Every
// piece works on the context its Sched carries (s.cx): the handle's own, or the level context of a run() with chain limbs below L.
void ntt(const Sched &s, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inv, bool sigma, bool fold, const NttExtra *ex)
{
    const NttPlan &pl = *s.cx->plan;
    ProfScope ps(s, inv ? PIEHIP_K_NTT_INV : PIEHIP_K_NTT_FWD, 16.0 * s.cx->N * nlimbs);
    launch_ntt(pl, data, nlimbs, mod_base, mod_count, inv, s.stream, sigma && pl.lane_order, fold && pl.fold, ex);
}

// BV key switch of the COEFFICIENT-format polynomials at w.d2c with `key`, added to the EVALUATION
// ciphertexts at w.d01, optionally multiplied by mask plaintexts: out[nb][2][L][N]
void enqueue_keyswitch(Sched &s, MulWs &w, u32 nb, RunKey key, const u64 *mask, u64 *out, KeyswitchOpts o)
{
    const ChainCtx &cx = *s.cx;
    const NttPlan &pl = *cx.plan;
    const u32 N = cx.N, L = cx.L;
    const size_t LN = cx.LN();
    const double W = 8.0 * N;
    const bool lane = o.lane && pl.lane_order;
    if (o.digits_ready) {
        // the caller's transform launch of d01 also lifted and transformed the digits
    } else if (lane ? pl.digit_lift_lane : pl.digit_lift_std) {
        ProfScope ps(s, PIEHIP_K_NTT_FWD, 16.0 * N * nb * L * L);
        launch_ntt_digits(pl, w.d2c, w.dig, nb, L, lane, s.stream);
    } else {
        {
            ProfScope ps(s, PIEHIP_K_DIGITS, W * nb * (L + (double)L * L));
            launch_digits(cx.d_dc, N, L, w.d2c, LN, nb, w.dig, s.stream, lane && pl.fold);
        }
        ntt(s, w.dig, nb * L * L, 0, L, false, lane, lane);
    }
    {
        if (o.out_is_result) s.gate();
        assert(!o.d01_eval_q || (pl.d01_eval_q && lane));
        ProfScope ps(s, PIEHIP_K_RELIN,
                     W * (nb * ((double)L * L + 2 * L + 2 * L + (mask ? L : 0) + (o.d01_eval_q ? 4 * L : 0)) + 2.0 * L * L));
        launch_relin_mac(cx.d_dc, N, L, w.d01, 2 * LN, w.dig, key.key, mask, out, nb, s.stream, pl.small_moduli,
                         lane ? cx.d_sigma_inv : nullptr, key.stride, key.group, lane ? pl.lane_T : 0, pl.lane_kp, mask ? s.mask_div : 1,
                         o.d01_eval_q ? w.eqp : nullptr, cx.M);
    }
}

// The EvalMult key of the run being enqueued, lane-ordered where the context has a lane order: the handle's key for every
// ciphertext row, or -- a batch whose queries bring their own keys (piehip_load_relin_key_q) -- key r % group of the array for row r
static RunKey run_key(const Sched &s)
{
    const ChainCtx &cx = *s.cx;
    const bool lane = cx.plan->lane_order;
    if (s.key_per_query) return {lane ? cx.evkq_sigma : cx.evkq, cx.key_words(), s.key_group};
    return {lane ? cx.evk_sigma : cx.evk};
}

// One batched EvalMult(ct,ct) (BatchedFHEHIPPIE.cpp:123): operands in COEFFICIENT format (produced by
// ntt(.., inverse, sigma = false, fold = true): with folding on, their outermost inverse stage is applied here),
// X and Y as launch_expand_pair takes them.  relin: out[nb][2][L][N] (times mask if given);
// otherwise out[nb][3][L][N] holds the EVALUATION-format tensor result -- times mask if given (a run()'s degree-2 result, include/piehip.h
// "Result relinearisation": the product is formed in w.t3; the mask is lane-ordered where plan.result_eval_q, in standard order otherwise).
void enqueue_mul(Sched &s, MulWs &w, const ExpandOperand &x, const ExpandOperand &y, u32 nb, bool relin, const u64 *mask, u64 *out,
                 bool out_is_result)
{
    const ChainCtx &cx = *s.cx;
    const u32 N = cx.N, L = cx.L, M = cx.M;
    const size_t LN = cx.LN();
    const double W = 8.0 * N;
    const NttPlan &pl = *cx.plan;
    const bool xq_ready = x.q_ready;
    {
        ProfScope ps(s, PIEHIP_K_EXPAND, W * nb * (2.0 * std::max(y.src_L, L) + 2.0 * std::max(x.src_L, L) + 4.0 * M));
        const bool ok = launch_expand_pair(cx.d_dc, N, L, x, y, nb, w.eqp, s.stream, pl, pl.fold);
        assert(ok);
        (void)ok;
    }
    // the QP operands and the tensor result never leave the library: lane order, no LDS transposes
    {
        NttExtra ex;
        ex.lazy_out = true;  // the tensor product's Barrett reduction takes any operands < 2^63
        if (xq_ready) {
            ex.skip_L = L;
            ex.skip_M = M;
        }
        ntt(s, w.eqp, nb * (xq_ready ? 4 * M - 2 * L : 4 * M), 0, M, false, true, true, &ex);
    }
    // Tensor product and inverse transform of its result.  One launch where the plan allows: each item forms its input from the four
    // operands in its load phase, the tensor result is neither written nor read back (3 M limbs per row each way).
    // A relinearising product needs d0 and d1 back in EVALUATION form, and their Q limbs enter scale-and-round only as the own-limb term
    // c_k d_k: where the plan says so those 2 L limbs per row are neither inverse-transformed here nor read by scale-and-round, and the
    // key-switch MAC adds c_k (a (x) b)_k from the QP operands.  d2 keeps every limb: the digit lift wants coefficients.
    // A product that is not relinearised and goes out as a run()'s result has no digit lift: d2 qualifies too, no Q limb is
    // inverse-transformed, and the finishing kernel adds the three own-limb terms.
    const bool eval_q = relin && pl.d01_eval_q;
    const bool deg2 = !relin && mask;
    const bool eval_q3 = deg2 && pl.result_eval_q;
    if (pl.fused_tensor) {
        ProfScope ps(s, PIEHIP_K_TENSOR_NTT_INV, W * nb * 7.0 * M);  // (the tensor product's bytes, whichever limbs are transformed)
        launch_ntt16_tensor(pl, w.eqp, w.dqp, nb, M, s.stream, (eval_q || eval_q3) ? L : 0, eval_q3);
    } else {
        {
            ProfScope ps(s, PIEHIP_K_TENSOR, W * nb * 7.0 * M);
            launch_tensor(cx.d_dc, N, M, w.eqp, w.dqp, nb, s.stream, pl.small_moduli);
        }
        ntt(s, w.dqp, nb * 3 * M, 0, M, true, true, true);
    }
    if (relin) {
        {
            ProfScope ps(s, PIEHIP_K_SCALE, W * nb * (3.0 * M + 3.0 * L));
            launch_scale_round(cx.d_dc, N, L, w.dqp, nb, w.d01, 2 * LN, w.d2c, LN, s.stream, pl, pl.fold, false, eval_q);
        }
        NttExtra ex;
        ex.lazy_out = true;  // the key-switch MAC adds d01 into its accumulator before reducing
        if (pl.digits_with_d01) {
            // one launch for both forward transforms in front of the key-switch MAC: d0, d1 and the L * L digits of d2
            ProfScope ps(s, PIEHIP_K_NTT_FWD, 16.0 * N * nb * (2.0 * L + (double)L * L));
            Ntt16Digits dg = {w.d2c, LN, w.dig, nb, L};
            launch_ntt16(pl, w.d01, nb * 2 * L, 0, L, false, true, s.stream, &ex, &dg);
        } else {
            ntt(s, w.d01, nb * 2 * L, 0, L, false, true, true, &ex);
        }
        KeyswitchOpts o;
        o.lane = true;
        o.out_is_result = out_is_result;
        o.digits_ready = pl.digits_with_d01;
        o.d01_eval_q = eval_q;
        enqueue_keyswitch(s, w, nb, run_key(s), mask, out, o);
    } else if (eval_q3) {
        {
            ProfScope ps(s, PIEHIP_K_SCALE, W * nb * (3.0 * (M - L) + 3.0 * L));
            launch_scale_round(cx.d_dc, N, L, w.dqp, nb, w.t3, 3 * LN, w.t3 + 2 * LN, 3 * LN, s.stream, pl, pl.fold, true, true, true);
        }
        NttExtra ex;
        ex.lazy_out = true;  // the finishing kernel adds the own-limb term into its accumulator before reducing
        ntt(s, w.t3, nb * 3 * L, 0, L, false, true, true, &ex);
        if (out_is_result) s.gate();
        ProfScope ps(s, PIEHIP_K_DEG2_FINISH, W * nb * 11.0 * L);
        launch_deg2_finish(cx.d_dc, N, L, w.t3, w.eqp, M, mask, out, nb, s.stream, pl.lane_T, pl.lane_kp, s.mask_div);
    } else {
        u64 *t = deg2 ? w.t3 : out;
        {
            ProfScope ps(s, PIEHIP_K_SCALE, W * nb * (3.0 * M + 3.0 * L));
            launch_scale_round(cx.d_dc, N, L, w.dqp, nb, t, 3 * LN, t + 2 * LN, 3 * LN, s.stream, pl, pl.fold, true);
        }
        ntt(s, t, nb * 3 * L, 0, L, false, false, true);
        if (deg2) {
            if (out_is_result) s.gate();
            ProfScope ps(s, PIEHIP_K_MASK, W * nb * 3 * 3.0 * L);
            launch_ct_mul_plain(cx.d_dc, N, L, t, mask, LN, out, nb, s.stream, s.mask_div, 3);
        }
    }
}

// Result limbs (include/piehip.h): rows of full-width ciphertexts to their first `keep` limbs.  Three launches on the current queue: the
// inverse transform of every limb (standard order in, where relin_mac and the K = 1 mask multiply write), the limb-drop kernel --
// which holds a coefficient's L residues in registers -- and the forward transform of the kept limbs, in place in `out`.  All limbs
// are transformed; the other schedule the definition allows (inverse-transform the dropped limbs only, forward-transform a
// correction and combine in EVALUATION format) has not been built or measured.  No outer-stage folding either: the rows arrive in
// standard order from kernels that do not fold.
// In a run that brings its results down to host memory the next queue group is released here, in front of the limb-drop kernel:
// this group then has that kernel and the forward transform of the kept limbs left, about what the key-switch MAC alone is when
// nothing is reduced, and its (smaller) download still travels under the next group's evaluation.
void enqueue_mod_reduce(Sched &s, u64 *full, u32 rows, u32 keep, u64 *out, bool out_is_result, u32 comps)
{
    const ChainCtx &cx = *s.cx;
    const u32 N = cx.N, L = cx.L;
    const double W = 8.0 * N;
    {
        ProfScope ps(s, PIEHIP_K_RESULT_NTT_INV, 2 * W * rows * comps * L);
        launch_ntt(*cx.plan, full, rows * comps * L, 0, L, true, s.stream);
    }
    if (out_is_result) s.gate();
    {
        ProfScope ps(s, PIEHIP_K_LIMB_DROP, W * rows * comps * (L + keep));
        launch_limb_drop(cx.d_dc, N, L, keep, full, out, rows * comps, s.stream);
    }
    {
        ProfScope ps(s, PIEHIP_K_RESULT_NTT_FWD, 2 * W * rows * comps * keep);
        launch_ntt(*cx.plan, out, rows * comps * keep, 0, keep, false, s.stream);
    }
}

// Queues of a run().  The default is two when the handle evaluates enough bin layers to fill the chip twice over; below that
// every launch is bound by its own latency, a second queue only interleaves two latency-bound chains on the same CUs, and one
// queue is faster (measured at the C3 ring: 2 layers 115 vs 146 us, 5 layers of the E = 40 row 217 vs 239 us, 7 layers even).
static const u32 MAX_RUN_QUEUES = 2;  // 3 is equal within noise, 4 and more collapse
u32 run_queue_count(const piehip_ctx *h)
{
    const u32 want = h->run_streams ? h->run_streams : (h->b >= 8 ? 2u : 1u);
    return std::min(want, std::min(MAX_RUN_QUEUES, h->b));
}

// The queues are created when a run first needs them: a handle that runs on one queue (a query slot, a rank's small share)
// then owns one stream, not three -- the runtime multiplexes streams onto a few hardware queues, and streams that share one
// serialise against each other.
int ensure_run_queues(piehip_ctx *h, u32 ng)
{
    while (h->side_streams.size() < ng) {
        hipStream_t s = nullptr;
        hipEvent_t e = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        h->side_streams.push_back(s);
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ev_join.push_back(e);
    }
    return PIEHIP_OK;
}

// stage A of the run being enqueued hands operand X of the first product over in lane order, inside the QP operand array
// (not where the first product runs below L: the dropped X is not what stage A computed, every accumulator goes to d_acc)
bool run_x_direct(const piehip_ctx *h) { return h->K > 1 && h->nq > 1 && h->plan.x_direct && h->chain_level(1) >= h->hp.L; }

// the last product of run()'s chain works on this context (a handle with K = 1 has no product: nothing changes)
const ChainCtx &run_chain_ctx(const piehip_ctx *h) { return h->K >= 2 ? h->level_cx(h->chain_last()) : h->cx; }
// every product that relinearises finds its key(s) on its level (the handle's own context: checked by the caller, with its own message)
bool run_chain_keys_loaded(const piehip_ctx *h)
{
    for (u32 hf = 1; hf < h->K; hf++) {
        if (hf + 1 == h->K && !h->res_relin) break;   // the last product goes out as it is
        const ChainCtx &cx = h->level_cx(h->chain_level(hf));
        if (!(cx.evk || (h->cx.evkq && cx.evkq && h->evkq_n == h->nq && h->evkq_loaded == (1u << h->nq) - 1))) return false;
    }
    return true;
}

// bin layers of queue group g of ng.  Two groups take 4/7 and 3/7 of the layers: measured 3.5 % faster than equal halves at
// b = 14 (8 + 6: the ragged transform launches of the two queues fit the workgroup slots better than 7 + 7).
u32 run_group_size(u32 b, u32 ng, u32 g)
{
    if (ng == 2) {
        const u32 first = (4 * b + 3) / 7;
        return g == 0 ? first : b - first;
    }
    return b / ng + (g < b % ng ? 1 : 0);
}

}  // namespace piehip

// =================================================================================================
extern "C" {

// Bin layers [b0, b0 + nb) of run() on the queue of s: stage A, then the product chain; results[b][nq][2][L][N].
// chain_only (piehip_run_chain: the accumulators were put there, piehip_put_accumulators): the product chain alone
static void enqueue_run_bins_full(Sched &s, u32 b0, u32 nb, u64 *results, bool chain_only);
// everything of run() behind stage A for those layers (BatchedFHEHIPPIE.cpp:117-126), on the context run_chain_ctx chooses
static void enqueue_chain_bins(Sched &s, u32 b0, u32 layers, u64 *results);
// ... and, on a handle that hands its results out on fewer limbs, their reduction: results[b][nq][2][res_limbs][N].  The chain then
// writes the handle's full-width rows, which no caller reads: what orders a run against the result buffer's readers (and releases
// the next queue group of a host-results run) moves from the chain's last kernel to the reduction: the chain is enqueued ungated.
static void enqueue_run_bins(Sched &s, u32 b0, u32 nb, u64 *results, bool chain_only)
{
    piehip_ctx *h = s.h;
    const u32 keep = h->res_limbs, nq = h->nq;
    // chain limbs: the chain hands over rows of the level context, and the reduction -- from its Lc limbs down to keep -- runs there
    const ChainCtx &cx = run_chain_ctx(h);
    if (keep >= cx.L) {
        enqueue_run_bins_full(s, b0, nb, results, chain_only);
        return;
    }
    Sched chain = s;
    chain.wait_before_results = chain.release = nullptr;
    enqueue_run_bins_full(chain, b0, nb, h->d_full, chain_only);
    const size_t r0 = (size_t)b0 * nq;
    const u32 comps = h->res_comps();
    s.cx = &cx;
    enqueue_mod_reduce(s, h->d_full + r0 * comps * cx.LN(), nb * nq, keep, results + r0 * h->res_ct_words(), true, comps);
    s.cx = &h->cx;
}
static void enqueue_run_bins_full(Sched &s, u32 b0, u32 nb, u64 *results, bool chain_only)
{
    piehip_ctx *h = s.h;
    const u32 N = h->hp.N, L = h->hp.L, M = h->hp.M, K = h->K, b = h->b, E = h->E, nq = h->nq;
    const size_t LN = h->LN();
    const double W = 8.0 * N;
    // rows of the workspace: (bin layer, query) pairs, nq per layer; the product chain sees nb * nq ciphertexts
    const size_t r0 = (size_t)b0 * nq;
    const u32 layers = nb;
    nb *= nq;
    u64 *acc = h->d_acc + r0 * K * 2 * LN;
    // Operand X of the first ciphertext product (the accumulators of inner hash function 0) is needed twice: in COEFFICIENT
    // form by the base extension, and in EVALUATION form, lane-ordered, as the Q limbs of the QP operand (plan.xq_reuse).  Until r04
    // the inverse transform wrote that second copy; now stage A writes X there in the first place and the transform reads it
    // from there (out of place, lane order in: its fast path) -- 44 MB less per step at the headline shape: the inverse launches
    // 161 -> 150 us per step of three queries, stage A + 2.5 (its X rows leave in 64-byte runs) and the base extension + 2.5.
    // Query batches only: one query's transform launches are single partial rounds that gain 1 us, and its stage A kernel, which
    // runs at the HBM rate, loses 2.5 (profiles/r04/stage_a_writes_x_lane_ordered.txt).
    const bool x_direct = run_x_direct(h);
    if (h->profiling) {  // an empty bracket: what the event pair itself costs on this stream (reported beside the kernels' times)
        ProfScope ps(s, PIEHIP_K_EVENT_PAIR, 0.0);
    }
    if (!chain_only) {   // stage A: all inner products of these bin layers in one launch (BatchedFHEHIPPIE.cpp:101-116)
        ProfScope ps(s, PIEHIP_K_STAGE_A, W * ((double)layers * K * E * L + nq * ((double)K * E * 2 * L + 2.0 * L + (double)layers * K * 2 * L)));
        StageAQueries qs = {};
        for (u32 q = 0; q < nq; q++) qs.idx[q] = h->query[q].idx, qs.minus[q] = h->query[q].minus;
        const u64 *db = h->d_db + (size_t)b0 * E * LN;
        StageAXOut xo;
        if (x_direct) xo.out = h->ws.eqp + r0 * 4 * M * N, xo.M = M, xo.logns = h->plan.lane_logn;
        launch_stage_a_batch(h->d_dc, N, L, K, layers, E, qs, nq, db, acc, s.stream, h->plan.small_moduli, b, 0, 0, x_direct ? &xo : nullptr);
    }
    enqueue_chain_bins(s, b0, layers, results);
}
// Rows [r0, r0 + nb) of the workspace.  A queue group's rows start where the widest context of the chain (`wide`: the first product's)
// lays them out, and every product packs its rows behind that base at its own level's strides.  With one level for every product
// that is the level's own view, as ever; with a schedule two queue groups may be in products of different levels at the same
// moment, and a base computed in the narrower view would land inside the other group's rows.
static MulWs ws_rows(const MulWs &ws, const ChainCtx &wide, size_t r0, u32 nb)
{
    const size_t N = wide.N, LN = wide.LN();
    MulWs w = ws;
    w.nb = nb;
    w.eqp += r0 * 4 * wide.M * N;
    w.dqp += r0 * 3 * wide.M * N;
    w.d01 += r0 * 2 * LN;
    w.d2c += r0 * LN;
    w.dig += r0 * wide.L * LN;
    if (w.t3) w.t3 += r0 * 3 * LN;
    return w;
}
// What the products of a chain disagree on, one entry per product (the products behind the schedule's last entry share one)
struct ChainStep {
    const ChainCtx *cx = nullptr;   // the level the product runs on: constants, plan and tables, the limb prefixes of keys and masks
    ExpandOperand x, y;             // how X and Y lie in memory and what their conversion does first: everything but the pointers
    bool x_drop_kernel = false;     // fallback: X is the product before, on more limbs; the drop kernel rewrites it in place first ...
    bool x_folded = false;          // ... reading through the folded outer stage its inverse transform left pending
    // the inverse transform of this product's result, where another product follows: on this product's context
    bool inv_fold = false;          // leaves the outer stage to the next conversion (or to the drop kernel)
    bool inv_copy = false;          // also writes the Q limbs of the next X, lane-ordered, into the QP array (NttExtra copy_out)
};
// The product chain of run() (BatchedFHEHIPPIE.cpp:117-126).  Stage A left its accumulators on the handle's own context `top`, in rows
// of top.L limbs, and their inverse transform runs there.  Product hf runs on the level context of chain_level(hf) limbs (chain
// limbs and chain schedule, include/piehip.h) -- top itself at L.  On their way into a product of a lower level
// the accumulators, and the product before where it has more limbs, are dropped to that level: in the load phase of the fused
// conversion where every drop of the chain is built that way, otherwise by a drop kernel that rewrites them in place, after which
// the conversions of that level take plain operands.  A product on top.L limbs runs as it does without any setting, whichever route
// the products behind it take.  results[b][nq][comps][l_last][N].
static void enqueue_chain_bins(Sched &s, u32 b0, u32 layers, u64 *results)
{
    piehip_ctx *h = s.h;
    const ChainCtx &top = h->cx, &cx = run_chain_ctx(h);   // cx: the last product's level, the lowest of the chain
    const u32 N = top.N, K = h->K, nq = h->nq;
    const ChainCtx &wide = K >= 2 ? h->level_cx(h->chain_level(1)) : top;
    const NttPlan &pl = *cx.plan;
    const size_t TLN = top.LN(), LN = cx.LN();
    const double W = 8.0 * N;
    const size_t r0 = (size_t)b0 * nq;
    const u32 nb = layers * nq;
    MulWs w = ws_rows(h->ws, wide, r0, nb);
    u64 *acc = h->d_acc + r0 * K * 2 * TLN;   // stage A's rows: the handle's strides
    u64 *prod = h->d_prod ? h->d_prod + r0 * 2 * wide.LN() : nullptr;
    const bool deg2 = h->res_comps() == 3;   // piehip_set_result_relin(0): the last product goes out as it is, three components
    u64 *out = results + r0 * h->res_comps() * LN;
    const u64 *masks = ((deg2 ? pl.result_eval_q : pl.lane_order) ? cx.masks_sigma : cx.masks) + (size_t)b0 * LN;
    s.mask_div = nq;
    // per-query EvalMult keys: row r of a group is query r % nq.  A handle without a batch has query 0 only, and that query's key, once
    // loaded (piehip_load_relin_key_q(h, 0, ..)), is the one it relinearises with: run_keys_loaded accepts it in place of the handle's
    s.key_per_query = h->cx.evkq && h->evkq_n == nq;
    s.key_group = s.key_per_query ? nq : 1;
    if (K == 1) {
        // one inner hash function: multipliedResult is the inner product itself (BatchedFHEHIPPIE.cpp:117-120), so run() is
        // stage A and the mask multiply (:126) -- no ciphertext product, no transform, no key
        // (the release of the next queue group is not recorded here but behind the whole group: run_on_queues)
        s.wait_for_readers();
        ProfScope ps(s, PIEHIP_K_MASK, W * nb * 5.0 * cx.L);
        launch_ct_mul_plain(cx.d_dc, N, cx.L, acc, cx.masks + (size_t)b0 * LN, LN, out, nb, s.stream, nq);
        return;
    }
    // What the chain at L and the chains with products on a level disagree on, decided here and nowhere below.
    auto lvl = [&](u32 hf) -> const ChainCtx & { return h->level_cx(h->chain_level(hf)); };
    auto x_limbs = [&](u32 hf) { return hf == 1 ? top.L : lvl(hf - 1).L; };   // limbs of product hf's X as it arrives
    // fused: every limb drop rides in a conversion's load phase -- folded rings whose level moduli take the column-accumulator
    // arithmetic, source and target levels the conversion is built for, on every context the chain touches.  One drop that is not
    // built that way puts the whole chain on the drop kernel (dropped)
    const bool level = cx.L < top.L;   // some product runs on fewer limbs than the accumulators have
    bool fused = level && top.plan->fold;
    for (u32 hf = 1; hf < K && hf <= h->chain_n + 1 && fused; hf++) {
        const ChainCtx &c = lvl(hf);
        if (c.L == top.L) continue;
        fused = c.plan->fold && c.plan->small_moduli && c.plan->xq_reuse &&
                expand_drop_built(top.L, x_limbs(hf), c.L);
    }
    const bool dropped = level && !fused;
    // X is needed twice by a product: in COEFFICIENT form by the base extension, and in EVALUATION form, lane-ordered, as the Q limbs of
    // the QP operand (plan.xq_reuse).  The inverse transform that makes the first also writes the second (NttExtra copy_out) -- where
    // it makes the X the product takes: a dropped X is not what the QP array could hold in EVALUATION form, and below L the drop
    // kernel's chain transforms without folding, into plain coefficients like the dropped accumulators, and copies nothing
    const u32 nsteps = std::min(K - 1, h->chain_n + 1);   // the products behind the schedule's last entry are all alike
    ChainStep steps[MAX_CHAIN_SCHED + 1];
    for (u32 i = 0; i < nsteps; i++) {
        const u32 hf = i + 1;
        ChainStep &t = steps[i];
        const ChainCtx &c = lvl(hf);
        const bool at_top = c.L == top.L, x_drop = x_limbs(hf) > c.L;
        t.cx = &c;
        t.x.poly = (size_t)x_limbs(hf) * N;   // the first X is an accumulator like every Y, a later one the product before, packed
        t.x.row = hf == 1 ? (size_t)K * 2 * TLN : 2 * t.x.poly;
        t.y.poly = TLN;
        t.y.row = (size_t)K * 2 * TLN;
        if (at_top) {
            t.x.q_ready = c.plan->xq_reuse;
        } else if (fused) {
            const ChainCtx &xf = hf > 1 ? lvl(hf - 1) : top;   // where X comes from
            t.y.src_dc = top.d_dc, t.y.src_L = top.L;
            if (x_drop) t.x.src_dc = xf.d_dc, t.x.src_L = xf.L;
            t.x.q_ready = !x_drop;
        } else {
            t.x.plain = t.y.plain = true;
            t.x_drop_kernel = x_drop && hf > 1;   // (the first product's X is an accumulator: dropped with the others)
        }
        if (hf + 1 < K) {
            const bool same = lvl(hf + 1).L == c.L;
            t.inv_fold = at_top || fused;
            t.inv_copy = same && c.plan->xq_reuse && (at_top || fused);
        }
        if (i) t.x_folded = t.x_drop_kernel && steps[i - 1].inv_fold && steps[i - 1].cx->plan->fold;
    }
    const bool copy_first = steps[0].x.q_ready;
    NttExtra ex;
    ex.copy_out = w.eqp;
    ex.copy_K = K;
    ex.copy_L = top.L;
    ex.copy_M = top.M;
    ex.x_lane_in = run_x_direct(h);
    // every accumulator enters a ct x ct product exactly once: switch them all to COEFFICIENT format, on the handle's limbs
    ntt(s, acc, nb * K * 2 * top.L, 0, top.L, true, false, true, copy_first ? &ex : nullptr);
    ex.x_lane_in = false;
    ex.copy_K = 1;  // from here on the product is the X operand of the next multiplication
    if (dropped) {
        // accumulator 0 goes to the first product's level, accumulator hf to product hf's: one launch per run of neighbours with one
        // target, over all rows (a chain with one level for every product: one launch, the rows as one packed array)
        auto target = [&](u32 a) { return lvl(a ? a : 1).L; };
        for (u32 a0 = 0, a1; a0 < K; a0 = a1) {
            for (a1 = a0 + 1; a1 < K && target(a1) == target(a0); a1++) {}
            if (target(a0) == top.L) continue;
            ProfScope ps(s, PIEHIP_K_LIMB_DROP, W * nb * (a1 - a0) * 2 * (top.L + target(a0)));
            launch_chain_drop(top.d_dc, N, top.L, target(a0), acc + (size_t)a0 * 2 * TLN, nb * (a1 - a0) * 2, s.stream, top.plan->fold,
                              (a1 - a0) * 2, (size_t)K * 2 * TLN);
        }
    }
    // product chain over the inner hash functions (BatchedFHEHIPPIE.cpp:117-124); the mask multiply (:126) is fused into the last
    // key switch
    const u64 *x = acc;
    for (u32 hf = 1; hf < K; hf++) {
        const ChainStep &t = steps[std::min(hf, nsteps) - 1];
        const ChainCtx &c = *t.cx;
        const bool last = hf + 1 == K;
        if (t.x_drop_kernel) {   // under the constants of the level that made it, at its packed strides
            const ChainCtx &from = *s.cx;
            ProfScope ps(s, PIEHIP_K_LIMB_DROP, W * nb * 2 * (from.L + c.L));
            launch_chain_drop(from.d_dc, N, from.L, c.L, prod, nb * 2, s.stream, t.x_folded);
        }
        s.cx = &c;
        ExpandOperand xo = t.x, yo = t.y;
        xo.p = x, yo.p = acc + (size_t)hf * 2 * TLN;
        enqueue_mul(s, w, xo, yo, nb, !(last && deg2), last ? masks : nullptr, last ? out : prod, last);
        if (!last) {
            ex.copy_L = c.L;
            ex.copy_M = c.M;
            ntt(s, prod, nb * 2 * c.L, 0, c.L, true, false, t.inv_fold, t.inv_copy ? &ex : nullptr);
            x = prod;
        }
    }
    s.cx = &top;
}
// the result ciphertexts of bin layers [b0, b0 + nb) (rows [bin layer][query]) to the caller's host array, on the queue of s
static hipError_t download_rows(const Sched &s, u64 *host_results, const u64 *d_results, u32 b0, u32 nb)
{
    const size_t row = (size_t)s.h->nq * s.h->res_ct_words();
    return hipMemcpyAsync(host_results + (size_t)b0 * row, d_results + (size_t)b0 * row, (size_t)nb * row * sizeof(u64),
                          hipMemcpyDeviceToHost, s.stream);
}

}  // extern C

// piehip_run_into, and piehip_run_chain_into (chain_only: piehip_slice.cpp has checked what that call needs): the queues of a run
int piehip::run_on_queues(piehip_ctx *h, void *d_results, bool chain_only, u64 *host_results)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!d_results) return fail(PIEHIP_EINVAL, "null result buffer");
    if (!chain_only && h->slice.on) return fail(PIEHIP_ESTATE, "run: a query-sliced handle holds no whole database (piehip_run_slice / piehip_run_chain)");
    if (!h->K || (!chain_only && !h->d_db)) return fail(PIEHIP_ESTATE, "run: database not loaded");
    if (!h->d_acc || !h->ws.eqp) return fail(PIEHIP_ESTATE, "run: no workspace (an earlier allocation failed: piehip_set_query_batch / load)");
    if (!run_keys_loaded(h, h->cx)) return fail(PIEHIP_ESTATE, "run: relinearisation key not loaded");
    if (h->res_comps() == 3) {
        if (h->slice.on) return fail(PIEHIP_ESTATE, "run: a query-sliced handle relinearises its results (piehip_set_result_relin)");
        if (!h->ws.t3 || h->res_cap_comps < 3)
            return fail(PIEHIP_ESTATE, "run: no rows for three-component results (an earlier allocation failed: piehip_set_result_relin)");
    }
    if (!run_chain_keys_loaded(h))
        return fail(PIEHIP_ESTATE, "run: no key on the level context (an earlier allocation failed: piehip_set_chain_limbs)");
    if (h->res_limbs < h->hp.L && !h->d_full) return fail(PIEHIP_ESTATE, "run: no rows for the result reduction (an earlier allocation failed: piehip_set_result_limbs)");
    for (u32 q = 0; q < h->nq && !chain_only; q++) {
        if (h->query[q].idx && h->query[q].minus) continue;
        if (q) return fail(PIEHIP_ESTATE, "run: a query of the batch has no index matrix or minus element");
        return fail(PIEHIP_ESTATE, "run: setIndex / setMinusCompareElement not called");
    }
    HIPCHK(hipSetDevice(h->device));
    const u32 b = h->b;
    h->recs.clear();
    h->pool_used = 0;
    // Bin layers are independent: groups of them go to separate queues.  Most launches of one group leave part of the
    // chip idle (a transform launch is 0.4 .. 2 rounds of workgroups); another group's kernels fill it.
    // Ordering against the handle's stream:
    //   * inputs changed since the last run (setIndex, keys, database): the queues wait for the handle's stream first;
    //   * always: the kernel that writes the results waits for everything the caller queued on the handle's stream
    //     before this call (it may still be reading the result buffer of an earlier run);
    //   * the handle's stream joins the queues lazily, in the next entry point that is not a run (NEED / piehip_join),
    //     so back-to-back runs of one query batch keep every queue busy across run boundaries.
    const u32 ng = run_queue_count(h);
    if (ng > 1) {
        const int qrc = ensure_run_queues(h, ng);
        if (qrc) return qrc;
    }
    if (h->use_graph && !h->profiling && !host_results && h->nq == 1) {
        // One graph launch instead of ~13 kernel launches and 2 event operations per queue group: the same two chains, forked
        // from and joined back to the handle's stream inside the graph (so consecutive runs do not overlap each other, which
        // the eager path's lazy join allows).
        if (!h->gexec || h->g_idx != h->query[0].idx || h->g_minus != h->query[0].minus || h->g_res != d_results || h->g_ng != ng) {
            drop_graph(h);
            join_pending(h);
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            hipError_t ce = hipSuccess;
            if (ng > 1) {
                ce = hipEventRecord(h->ev_fork, h->stream);
                u32 b0 = 0;
                for (u32 g = 0; g < ng && ce == hipSuccess; g++) {
                    const u32 nb = run_group_size(b, ng, g);
                    Sched s(h, h->side_streams[g]);
                    ce = hipStreamWaitEvent(s.stream, h->ev_fork, 0);
                    enqueue_run_bins(s, b0, nb, (u64 *)d_results, chain_only);
                    if (ce == hipSuccess) ce = hipEventRecord(h->ev_join[g], s.stream);
                    if (ce == hipSuccess) ce = hipStreamWaitEvent(h->stream, h->ev_join[g], 0);
                    b0 += nb;
                }
            } else {
                Sched s(h);
                enqueue_run_bins(s, 0, b, (u64 *)d_results, chain_only);
            }
            const hipError_t ee = hipStreamEndCapture(h->stream, &graph);
            if (ce != hipSuccess || ee != hipSuccess || !graph) {
                if (graph) (void)hipGraphDestroy(graph);
                return fail(PIEHIP_EHIP, std::string("run: graph capture failed: ") + hipGetErrorString(ce != hipSuccess ? ce : ee));
            }
            const hipError_t ie = hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) {
                h->gexec = nullptr;
                return fail(PIEHIP_EHIP, std::string("run: hipGraphInstantiate: ") + hipGetErrorString(ie));
            }
            h->g_idx = h->query[0].idx, h->g_minus = h->query[0].minus, h->g_res = d_results, h->g_ng = ng;
        }
        join_pending(h);
        HIPCHK(hipGraphLaunch(h->gexec, h->stream));
        mark_dirty(h);  // the workspace is in use on the handle's stream
        return PIEHIP_OK;
    }
    if (ng > 1) {
        HIPCHK(hipEventRecord(h->ev_fork, h->stream));
        u32 b0 = 0;
        for (u32 g = 0; g < ng; g++) {
            const u32 nb = run_group_size(b, ng, g);
            Sched s(h, h->side_streams[g]);
            if (h->inputs_dirty) HIPCHK(hipStreamWaitEvent(s.stream, h->ev_fork, 0));
            s.wait_before_results = h->inputs_dirty ? nullptr : h->ev_fork;
            // Results go down to host memory (piehip_run_staged / piehip_run_host*): the groups do not run side by side but one
            // behind the other -- group g + 1 starts when group g has only its result-writing kernel left, and the download of
            // group g (8 of 14 MiB at C3) travels under the evaluation of group g + 1.  Results in host memory after 0.53 ms
            // instead of 0.60 at C3, 1.30 instead of 1.50 for a batch of three; a stream of queries over several handles is
            // bound by the uploads either way (profiles/r04/online_phase_staggered_groups.txt).
            if (host_results && g > 0) HIPCHK(hipStreamWaitEvent(s.stream, h->ev_chain, 0));
            if (host_results && g + 1 < ng) {
                if (!h->ev_chain) HIPCHK(hipEventCreateWithFlags(&h->ev_chain, hipEventDisableTiming));
                s.release = h->ev_chain;
            }
            enqueue_run_bins(s, b0, nb, (u64 *)d_results, chain_only);
            if (s.release) HIPCHK(hipEventRecord(s.release, s.stream));  // a chain without a key switch (K = 1): behind all of it
            if (host_results) HIPCHK(download_rows(s, host_results, (const u64 *)d_results, b0, nb));  // this group's slice, on this group's queue
            HIPCHK(hipEventRecord(h->ev_join[g], s.stream));
            b0 += nb;
        }
        h->pending_join = true;
        h->inputs_dirty = false;
    } else {
        join_pending(h);
        Sched s(h);
        enqueue_run_bins(s, 0, b, (u64 *)d_results, chain_only);
        if (host_results) HIPCHK(download_rows(s, host_results, (const u64 *)d_results, 0, b));
        mark_dirty(h);  // the workspace is now in use on the handle's stream: the queues of a later multi-queue run wait for it
    }
    HIPCHK(hipGetLastError());
    return PIEHIP_OK;
}

extern "C" {

int piehip_run_into(piehip_handle h, void *d_results) { return run_on_queues(h, d_results, false); }

int piehip_run(piehip_handle h)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!h->d_out) return fail(PIEHIP_ESTATE, "run: database not loaded");
    return piehip_run_into(h, h->d_out);
}

int piehip_join(piehip_handle h)
{
    NEED_RO(h);
    return PIEHIP_OK;
}

int piehip_set_graph(piehip_handle h, int on)
{
    NEED_RO(h);
    if (on && h->res_limbs < h->hp.L)
        return fail(PIEHIP_ESTATE, "set_graph: the captured graph hands out full results (piehip_set_result_limbs is below L)");
    if (on && !h->res_relin)
        return fail(PIEHIP_ESTATE, "set_graph: the captured graph relinearises its results (piehip_set_result_relin is off)");
    if (on && h->chain_floor() < h->hp.L)
        return fail(PIEHIP_ESTATE, "set_graph: the captured graph runs the product chain on every limb (piehip_set_chain_limbs is below L)");
    if (on && h->slice.on) return fail(PIEHIP_ESTATE, "set_graph: a query-sliced handle runs in two halves (piehip_run_slice, piehip_run_chain): no captured graph");
    h->use_graph = on != 0;
    if (!on) drop_graph(h);
    return PIEHIP_OK;
}

int piehip_set_run_streams(piehip_handle h, uint32_t n)
{
    NEED_RO(h);
    h->run_streams = n;
    return PIEHIP_OK;
}

}  // extern C
