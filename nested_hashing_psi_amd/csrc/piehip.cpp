// piehip.cpp -- C ABI (include/piehip.h) over the gfx950 kernels: the context, keys and database of a handle and its query inputs.
// The other entry points live in piehip_run.cpp / _host.cpp / _ops.cpp / _fhepie.cpp / _client.cpp / _rccl.cpp (piehip_ctx.hpp
// lists them).
#include "piehip_ctx.hpp"

#include <random>

using namespace piehip;

static thread_local std::string g_err;
static const char *KNAMES[PIEHIP_NKERNELS] = {"stage_a_mac", "ntt_fwd", "ntt_inv",  "expand",   "tensor",    "scale_round",
                                              "digits",      "relin",   "mask_mul", "encode",   "automorph", "other",
                                              "event_pair",  "tensor_ntt_inv", "result_ntt_inv", "limb_drop", "result_ntt_fwd",
                                              "deg2_finish"};
static void free_workspace(piehip_ctx *h);

namespace piehip {

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

void join_pending(piehip_ctx *h)
{
    if (!h->pending_join) return;
    for (size_t g = 0; g < h->ev_join.size(); g++) (void)hipStreamWaitEvent(h->stream, h->ev_join[g], 0);
    h->pending_join = false;
}

void mark_dirty(piehip_ctx *h) { h->inputs_dirty = true; }

void drop_graph(piehip_ctx *h)
{
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    h->gexec = nullptr;
}

// ---- profiling helpers -------------------------------------------------------------------------
hipEvent_t prof_event(piehip_ctx *h)
{
    if (h->pool_used == h->pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->pool.push_back(e);
    }
    return h->pool[h->pool_used++];
}

int dev_alloc(u64 **p, size_t words)
{
    *p = nullptr;
    if (!words) return PIEHIP_OK;
    hipError_t e = hipMalloc((void **)p, words * sizeof(u64));
    if (e != hipSuccess) return fail(PIEHIP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return PIEHIP_OK;
}
void dev_free(u64 **p)
{
    if (*p) (void)hipFree(*p);
    *p = nullptr;
}

int ws_alloc(piehip_ctx *h, MulWs &w, u32 nb)
{
    const size_t N = h->hp.N, L = h->hp.L, M = h->hp.M;
    w.nb = nb;
    int rc;
    if ((rc = dev_alloc(&w.eqp, (size_t)nb * 4 * M * N))) return rc;
    if ((rc = dev_alloc(&w.dqp, (size_t)nb * 3 * M * N))) return rc;
    if ((rc = dev_alloc(&w.d01, (size_t)nb * 2 * L * N))) return rc;
    if ((rc = dev_alloc(&w.d2c, (size_t)nb * L * N))) return rc;
    if ((rc = dev_alloc(&w.dig, (size_t)nb * L * L * N))) return rc;
    return PIEHIP_OK;
}
void ws_free(MulWs &w)
{
    dev_free(&w.eqp);
    dev_free(&w.dqp);
    dev_free(&w.d01);
    dev_free(&w.d2c);
    dev_free(&w.dig);
    dev_free(&w.t3);
    w.nb = 0;
}

// device-side MakePackedPlaintext of npt slot vectors (already on the device) into out[npt][L][N]
int encode_on_device(piehip_ctx *h, const int64_t *d_slots, u32 npt, u32 B, u64 *d_out)
{
    const u32 N = h->hp.N, L = h->hp.L, M = h->hp.M;
    // chunk so the mod-t scratch stays small
    const u32 chunk = ENCODE_CHUNK;
    Tmp tmp(h);
    TMPGET(d_u, (size_t)(npt < chunk ? npt : chunk) * N);
    for (u32 s = 0; s < npt; s += chunk) {
        const u32 c = npt - s < chunk ? npt - s : chunk;
        ProfScope ps(h, PIEHIP_K_ENCODE, 8.0 * c * ((double)B + 2.0 * N + (double)L * N));
        launch_encode_scatter(h->d_dc, N, M, d_slots + (size_t)s * B, B, h->d_inv_pos, d_u, c, h->stream);
        launch_ntt(h->plan, d_u, c, M, 1, true, h->stream);
        launch_encode_lift(h->d_dc, N, L, M, d_u, d_out + (size_t)s * L * N, c, h->stream);
        launch_ntt(h->plan, d_out + (size_t)s * L * N, c * L, 0, L, false, h->stream);
    }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(PIEHIP_EHIP, std::string("encode: ") + hipGetErrorString(e));
    return PIEHIP_OK;
}

int query_input_buffers(piehip_ctx *h, u32 q, u64 **d_idx, u64 **d_minus)
{
    if (!h->K) return fail(PIEHIP_ESTATE, "load the database before the index matrix");
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    Query &s = h->query[q];
    int rc;
    if (!s.idx_own && (rc = dev_alloc(&s.idx_own, (size_t)h->K * h->E * 2 * h->LN()))) return rc;
    if (!s.minus_own && (rc = dev_alloc(&s.minus_own, 2 * h->LN()))) return rc;
    *d_idx = s.idx_own;
    *d_minus = s.minus_own;
    return PIEHIP_OK;
}

int ensure_full_rows(piehip_ctx *h, u32 K)
{
    if (!h->ws_cap_rows) return PIEHIP_OK;
    const u32 comps = h->res_comps(K);
    int rc;
    if (comps > h->res_cap_comps) {   // three-component rows from here on: the result rows grow, the reduction's rows with them
        dev_free(&h->d_out);
        dev_free(&h->d_full);
        h->res_cap_comps = 0;
        if ((rc = dev_alloc(&h->d_out, h->ws_cap_rows * comps * h->LN()))) return rc;
        h->res_cap_comps = comps;
    }
    if (comps == 3 && !h->ws.t3 && (rc = dev_alloc(&h->ws.t3, h->ws_cap_rows * 3 * h->LN()))) return rc;
    if (h->res_limbs >= h->hp.L || h->d_full) return PIEHIP_OK;
    return dev_alloc(&h->d_full, h->ws_cap_rows * h->res_cap_comps * h->LN());
}

void use_owned_inputs(piehip_ctx *h)
{
    for (u32 q = 0; q < h->nq; q++) h->query[q].idx = h->query[q].idx_own, h->query[q].minus = h->query[q].minus_own;
}

// device copy of a table made by piehip_create (src null: room for one); the handle owns it (piehip_destroy frees dev_tables)
template <class T, class P>
static hipError_t upload_table(piehip_ctx *h, const T *src, size_t n, P **dst)
{
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    h->dev_tables.push_back(p);
    *dst = (P *)p;
    return src ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
}

}  // namespace piehip

// What a context (N, L, t, q, p) needs on the device: its constant block, the transform tables and the plan that says what the
// context does with them, the lane-order map (and, d_inv_pos, the encoder's slot map).  piehip_create's, and a level context's
// (chain limbs).  The handle owns the tables (dev_tables).  Returns the error text, empty on success.
static std::string context_tables(piehip_ctx *h, const HostParams &hp, NttPlan &pl, DevConsts **d_dc, u32 **d_sigma_inv, u32 **d_inv_pos)
{
#define TBL_(expr)                                                                     \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e_); \
    } while (0)
    const u32 N = hp.N, M = hp.M, logN = hp.logN;
    pl.N = N;
    pl.logN = logN;
    {
        bool lazy_ok = true, small_moduli = true, fold_moduli = true;
        for (u32 a = 0; a <= M; a++) {
            if (hp.moduli[a] >> 60) lazy_ok = false;                      // lazy residues need 8q < 2^63 (t included)
            if (a < M && (hp.moduli[a] >> 59) != 1) small_moduli = false;  // the mad paths assume 2^59 < q < 2^60 (Q and P)
            if (a < M && (1ull << 60) - hp.moduli[a] >= COLACC_FOLD_MAX_D) fold_moduli = false;  // q = 2^60 - d, d below the proven bound
        }
        ntt_plan_decide(pl, lazy_ok, small_moduli, fold_moduli);
        pl.fold_mod_count = pl.fold_moduli ? M : 0;
        hipDeviceProp_t prop;
        pl.num_cus = (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) ? (u32)prop.multiProcessorCount : 256u;
    }
    TBL_(upload_table(h, &hp.dc, 1, d_dc));
    pl.dc = *d_dc;
    {
        std::vector<u64> pairs((size_t)(M + 1) * 4 * N);
        u64 *tables = nullptr;  // [(M+1)][4][N]
        TBL_(upload_table(h, (const u64 *)nullptr, pairs.size(), &tables));
        pl.tables = tables;
        for (u32 a = 0; a <= M; a++) {
            for (const std::vector<u64> *t : {&hp.tw[a], &hp.tw_sh[a], &hp.itw[a], &hp.itw_sh[a]}) {
                TBL_(hipMemcpy(tables, t->data(), sizeof(u64) * N, hipMemcpyHostToDevice));
                tables += N;
            }
            for (u32 k = 0; k < N; k++) {
                u64 *f = &pairs[((size_t)a * 2 + 0) * 2 * N + 2 * (size_t)k];
                u64 *i = &pairs[((size_t)a * 2 + 1) * 2 * N + 2 * (size_t)k];
                // the register-blocked kernels use 63-bit Shoup constants floor(w 2^63 / q) (kernels_ntt_fast.hip)
                f[0] = hp.tw[a][k];
                f[1] = hp.tw_sh[a][k] >> 1;
                i[0] = hp.itw[a][k];
                i[1] = hp.itw_sh[a][k] >> 1;
            }
        }
        TBL_(upload_table(h, pairs.data(), pairs.size(), &pl.twp));
        // the kernel-ordered twiddles of every (modulus, direction), one after the other
        auto kernel_order = [&](bool k16, u32 s0, const u64 **dst) {
            std::vector<u64> all, one;
            for (u32 a = 0; a <= M; a++)
                for (u32 dir = 0; dir < 2; dir++) {
                    const u64 *nat = &pairs[((size_t)a * 2 + dir) * 2 * N];
                    if (k16)
                        build_twk16_table(nat, s0, logN - s0, one);
                    else
                        build_twc_table(nat, logN, s0, one);
                    all.insert(all.end(), one.begin(), one.end());
                }
            return upload_table(h, all.data(), all.size(), dst);
        };
        if (pl.lane_order) TBL_(kernel_order(false, ntt_route(pl, false, false, false).s0, &pl.twc));
        if (pl.fold) TBL_(kernel_order(false, 1, &pl.twc_fold));
        if (pl.lane_kernel == NttKernel::blocked16) TBL_(kernel_order(true, logN - pl.lane_logn, &pl.twk16));
    }
    {
        std::vector<u32> inv(N, 0xFFFFFFFFu), smap;
        for (u32 s = 0; s < N; s++) inv[hp.slot_pos[s]] = s;
        if (d_inv_pos) TBL_(upload_table(h, inv.data(), inv.size(), d_inv_pos));
        if (pl.lane_kernel == NttKernel::blocked16)
            ntt16_sigma_inverse_map(logN, logN - pl.lane_logn, smap);
        else
            ntt_sigma_inverse_map(logN, pl.lane_order ? logN - pl.lane_logn : ~0u, smap);
        TBL_(upload_table(h, smap.data(), smap.size(), d_sigma_inv));
    }
#undef TBL_
    return std::string();
}

// =================================================================================================
extern "C" {

int piehip_version(void) { return 102; }   // 101: piehip_profile_read_n, piehip_set_transform_slots, piehip_upload_turn_wait, piehip_rccl_abort; 102: seeded ciphertexts (the result limbs, the query slices, the seeded query slices and the chain limbs came without a new number: tests pin 102)
const char *piehip_last_error(void) { return g_err.c_str(); }
const char *piehip_kernel_name(int k) { return (k >= 0 && k < PIEHIP_NKERNELS) ? KNAMES[k] : "?"; }

int piehip_default_moduli(uint32_t N, uint32_t L, uint64_t *q, uint64_t *p)
{
    if (!q || !p || L < 1 || L > MAX_L || N < 8 || (N & (N - 1))) return fail(PIEHIP_EINVAL, "bad N/L");
    std::vector<u64> ch(2 * L + 1);
    if (!prime_chain(N, 1ULL << 60, 2 * L + 1, ch.data())) return fail(PIEHIP_EINVAL, "prime chain exhausted");
    memcpy(q, ch.data(), sizeof(u64) * L);
    memcpy(p, ch.data() + L, sizeof(u64) * (L + 1));
    return PIEHIP_OK;
}

int piehip_create(piehip_handle *out, uint32_t N, uint32_t L, uint64_t t, const uint64_t *q, const uint64_t *p, int device,
                  void *stream)
{
    if (!out) return fail(PIEHIP_EINVAL, "null out");
    *out = nullptr;
    piehip_ctx *h = new piehip_ctx();
    std::string err = h->hp.init(N, L, t, q, p);
    if (!err.empty()) {
        delete h;
        return fail(PIEHIP_EINVAL, err);
    }
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev <= 0) {
        delete h;
        return fail(PIEHIP_EHIP, std::string("no HIP device visible (hipGetDeviceCount: ") + hipGetErrorString(de) + ", " +
                                     std::to_string(ndev) + " devices): libpiehip has no CPU fallback");
    }
    h->device = device;
    h->res_limbs = L;
    h->chain_sched[0] = L, h->chain_n = 1;
#define CHK_(expr)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);             \
            piehip_destroy(h);                                                              \
            return fail(PIEHIP_EHIP, m_);                                                   \
        }                                                                                   \
    } while (0)
    CHK_(hipSetDevice(device));
    if (stream) {
        h->stream = (hipStream_t)stream;
    } else {
        CHK_(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    CHK_(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    {
        const std::string terr = context_tables(h, h->hp, h->plan, &h->d_dc, &h->d_sigma_inv, &h->d_inv_pos);
        if (!terr.empty()) {
            piehip_destroy(h);
            return fail(PIEHIP_EHIP, terr);
        }
    }
    h->cx.d_dc = h->d_dc, h->cx.plan = &h->plan, h->cx.d_sigma_inv = h->d_sigma_inv, h->cx.N = N, h->cx.L = L, h->cx.M = h->hp.M;
#undef CHK_
    *out = h;
    return PIEHIP_OK;
}

// The lane-ordered twin of the `rows` polynomials at src, under cx's map: allocated if absent, rows [first, first + count) permuted
// into it on the handle's stream.  Nothing where the context has no lane order.
static int lane_twin(piehip_ctx *h, const ChainCtx &cx, const u64 *src, u64 **twin, size_t rows, size_t first, size_t count)
{
    if (!cx.plan->lane_order) return PIEHIP_OK;
    if (!*twin) {
        int rc = dev_alloc(twin, rows * cx.N);
        if (rc) return rc;
    }
    launch_permute(cx.N, src + first * cx.N, cx.d_sigma_inv, *twin + first * cx.N, (u32)count, h->stream);
    return PIEHIP_OK;
}
static int lane_twin(piehip_ctx *h, const ChainCtx &cx, const u64 *src, u64 **twin, size_t rows) { return lane_twin(h, cx, src, twin, rows, 0, rows); }
static void chain_data_free(ChainCtx &cx)
{
    for (u64 **p : {&cx.evk, &cx.evk_sigma, &cx.evkq, &cx.evkq_sigma, &cx.masks, &cx.masks_sigma}) dev_free(p);
}

// what a handle that borrows its database takes of its owner by reference (piehip_attach_database), and lets go of again (null)
static void share_database(piehip_ctx *h, const piehip_ctx *owner)
{
    const ChainCtx from = owner ? owner->cx : ChainCtx();
    h->cx.evk = from.evk, h->cx.evk_sigma = from.evk_sigma, h->cx.masks = from.masks, h->cx.masks_sigma = from.masks_sigma;
    h->d_db = owner ? owner->d_db : nullptr;
}
static void detach_database(piehip_ctx *h)
{
    if (!h->db_borrowed) return;
    share_database(h, nullptr);
    h->db_borrowed = false;
    if (h->db_owner && h->db_owner->db_borrowers) h->db_owner->db_borrowers--;
    h->db_owner = nullptr;
}

int piehip_destroy(piehip_handle h)
{
    if (!h) return PIEHIP_OK;
    if (h->db_borrowers) return fail(PIEHIP_ESTATE, "destroy: other handles still use this handle's database (destroy them first)");
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)piehip_rccl_destroy(h);
    for (hipEvent_t e : h->pool) (void)hipEventDestroy(e);
    detach_database(h);
    slice_free(h);
    dev_free(&h->d_db);
    chain_data_free(h->cx);   // (what was borrowed is no longer there)
    for (Query &s : h->query) {
        dev_free(&s.idx_own);
        dev_free(&s.minus_own);
    }
    free_workspace(h);
    for (void *p : h->dev_tables) (void)hipFree(p);
    for (auto &kv : h->levels) chain_data_free(kv.second->cx);
    dev_free(&h->d_hash_tbl);
    dev_free(&h->arena);
    for (auto &kv : h->rotkeys) (void)hipFree(kv.second);
    for (auto &kv : h->rotmaps) (void)hipFree(kv.second);
    dev_free(&h->fp_pt);
    dev_free(&h->fp_mask);
    dev_free(&h->fp_e0);
    dev_free(&h->fp_idx);
    dev_free(&h->fp_out);
    dev_free(&h->fp_negkeys);
    if (h->fp_negmaps) (void)hipFree(h->fp_negmaps);
    for (hipStream_t s : h->side_streams) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    drop_graph(h);
    free_host_path(h);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_chain) (void)hipEventDestroy(h->ev_chain);
    for (hipEvent_t e : h->ev_join) (void)hipEventDestroy(e);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PIEHIP_OK;
}

int piehip_get_moduli(piehip_handle h, uint64_t *out)
{
    NEED_RO(h);
    memcpy(out, h->hp.moduli.data(), sizeof(u64) * (h->hp.M + 1));
    return PIEHIP_OK;
}
int piehip_get_root(piehip_handle h, uint32_t mi, uint64_t *psi)
{
    NEED_RO(h);
    if (mi > h->hp.M) return fail(PIEHIP_EINVAL, "mod_index out of range");
    *psi = h->hp.psi[mi];
    return PIEHIP_OK;
}
int piehip_get_twiddles(piehip_handle h, uint32_t mi, uint64_t *fwd, uint64_t *inv)
{
    NEED_RO(h);
    if (mi > h->hp.M) return fail(PIEHIP_EINVAL, "mod_index out of range");
    if (fwd) memcpy(fwd, h->hp.tw[mi].data(), sizeof(u64) * h->hp.N);
    if (inv) memcpy(inv, h->hp.itw[mi].data(), sizeof(u64) * h->hp.N);
    return PIEHIP_OK;
}
int piehip_get_slot_positions(piehip_handle h, uint32_t *pos)
{
    NEED_RO(h);
    memcpy(pos, h->hp.slot_pos.data(), sizeof(u32) * h->hp.N);
    return PIEHIP_OK;
}

// Per-query key slots (piehip_load_relin_key_q) that no query loaded hold a COPY of the handle's key and of its lane-ordered
// twin, if the handle has one: they follow it.  Queued on the handle's stream; the caller waits.
static int fill_unloaded_key_slots(piehip_ctx *h)
{
    const ChainCtx &c = h->cx;
    const size_t words = c.key_words();
    for (u32 i = 0; i < h->evkq_n && c.evkq && c.evk; i++) {
        if (h->evkq_loaded >> i & 1) continue;
        HIPCHK(hipMemcpyAsync(c.evkq + i * words, c.evk, words * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
        if (h->plan.lane_order && c.evkq_sigma)
            HIPCHK(hipMemcpyAsync(c.evkq_sigma + i * words, c.evk_sigma, words * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
    }
    return PIEHIP_OK;
}

int piehip_load_relin_key(piehip_handle h, const uint64_t *evk)
{
    NEED(h);
    if (!evk) return fail(PIEHIP_EINVAL, "null evk");
    if (h->db_borrowed) return fail(PIEHIP_EINVAL, "this handle uses another handle's key and database (piehip_attach_database)");
    if (h->db_borrowers) return fail(PIEHIP_ESTATE, "the key cannot be reloaded while other handles are attached to this one");
    HIPCHK(hipSetDevice(h->device));
    ChainCtx &c = h->cx;
    const size_t words = c.key_words();
    int rc;
    if (!c.evk && (rc = dev_alloc(&c.evk, words))) return rc;
    // on the handle's stream: NEED() has ordered it behind every run still in flight (a null-stream copy would not be)
    HIPCHK(hipMemcpyAsync(c.evk, evk, words * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((rc = lane_twin(h, c, c.evk, &c.evk_sigma, c.L * 2 * c.L))) return rc;  // for the key-switch MAC
    if (h->plan.lane_order) HIPCHK(hipStreamSynchronize(h->stream));
    if ((rc = fill_unloaded_key_slots(h))) return rc;
    if (c.evkq) HIPCHK(hipStreamSynchronize(h->stream));
    return level_sync(h);
}

// lane-ordered copy of the mask plaintexts for the fused mask multiply of the last key switch (freed with the run buffers when the
// shape changes); with chain limbs, the level context's copies follow every mask load
extern "C++" int piehip::make_masks_sigma(piehip_ctx *h)
{
    int rc = lane_twin(h, h->cx, h->cx.masks, &h->cx.masks_sigma, (size_t)h->b * h->hp.L);
    if (rc) return rc;
    if (h->plan.lane_order) {
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(PIEHIP_EHIP, std::string("mask permutation: ") + hipGetErrorString(e));
    }
    return level_sync(h);
}

// run() workspace and result rows for b bin layers x nq queries of K inner hash functions
static void free_workspace(piehip_ctx *h)
{
    dev_free(&h->d_acc);
    dev_free(&h->d_prod);
    dev_free(&h->d_out);
    dev_free(&h->d_full);
    ws_free(h->ws);
    h->ws_cap_rows = h->ws_cap_K = 0;
    h->res_cap_comps = 0;
}
// Every array of the workspace is indexed by row first, so one sized for more rows serves fewer as it stands: a smaller batch
// keeps the larger allocation (a server that alternates between batch sizes would otherwise free and allocate 0.6 GiB per change,
// and what the allocator hands back after such churn is not what it handed out first: uploads into input buffers allocated later
// ran at half the link rate in some sequences of bench.py's legs).
static int alloc_workspace(piehip_ctx *h, u32 K, u32 b)
{
    const size_t LN = h->LN(), rows = (size_t)b * h->nq;
    if (h->d_acc && h->d_out && h->ws.eqp && h->ws_cap_K == K && rows <= h->ws_cap_rows && (K <= 2 || h->d_prod)) {
        h->ws.nb = (u32)rows;
        return ensure_full_rows(h, K);
    }
    free_workspace(h);
    int rc;
    if ((rc = dev_alloc(&h->d_acc, rows * K * 2 * LN))) return rc;
    const u32 comps = h->res_comps(K);
    if ((rc = dev_alloc(&h->d_out, rows * comps * LN))) return rc;
    if (K > 2 && (rc = dev_alloc(&h->d_prod, rows * 2 * LN))) return rc;
    if ((rc = ws_alloc(h, h->ws, (u32)rows))) return rc;
    h->ws_cap_rows = rows;
    h->ws_cap_K = K;
    h->res_cap_comps = comps;
    return ensure_full_rows(h, K);
}

extern "C++" int piehip::alloc_run_buffers(piehip_ctx *h, u32 K, u32 b, u32 E, bool with_db)
{
    drop_graph(h);  // the captured launches hold the addresses and shapes of the buffers below
    h->forget_rows();  // K decides the components and limbs of a result row
    if (with_db) slice_free(h);  // a whole database from here on: no longer a query-sliced handle
    if (h->db_borrowed && with_db) {  // a database of its own from here on; the key goes back too (load it again)
        detach_database(h);
        h->K = h->b = h->E = 0;
    }
    if (K < 1) return fail(PIEHIP_EINVAL, "at least one inner hash function");
    // (a query-sliced handle without a chain side keeps no bin layer: piehip_slice.cpp, with_db false)
    if ((b < 1 && with_db) || E < 1) return fail(PIEHIP_EINVAL, "Bin size needs to be at least of size one!");
    // the database and masks are shared with the attached query slots, whose streams are not ordered against this handle's:
    // rewriting them in place (same shape) would race with their runs, reallocating them would leave them dangling
    if (with_db && h->db_borrowers)
        return fail(PIEHIP_ESTATE, "a database cannot be loaded while other handles are attached to this one (destroy or re-home them first)");
    const size_t LN = h->LN();
    if (with_db && h->K == K && h->b == b && h->E == E && h->d_db && h->cx.masks && h->d_acc && h->d_out && h->ws.nb == b * h->nq) {
        // same shape as the database being replaced (or reserved): keep the 0.5 GiB of buffers (hipFree + hipMalloc cost
        // ~10 ms); the inputs of the previous database are stale
        for (Query &s : h->query) s.idx = nullptr;
        return PIEHIP_OK;
    }
    dev_free(&h->d_db);
    dev_free(&h->cx.masks);
    dev_free(&h->cx.masks_sigma);
    free_workspace(h);
    h->K = h->b = h->E = 0;
    int rc;
    if (with_db && (rc = dev_alloc(&h->d_db, (size_t)K * b * E * LN))) return rc;
    if (with_db && (rc = dev_alloc(&h->cx.masks, (size_t)b * LN))) return rc;
    if ((rc = alloc_workspace(h, K, b))) return rc;
    h->K = K;
    h->b = b;
    h->E = E;
    // inputs depend on K,E: drop stale copies
    h->stage_open = false;
    for (Query &s : h->query) {
        dev_free(&s.idx_own);
        s.idx = nullptr;
    }
    return PIEHIP_OK;
}

int piehip_load_db(piehip_handle h, uint32_t K, uint32_t b, uint32_t E, const uint64_t *pts, const uint64_t *masks)
{
    NEED(h);
    if (!pts || !masks) return fail(PIEHIP_EINVAL, "null database");
    HIPCHK(hipSetDevice(h->device));
    int rc = alloc_run_buffers(h, K, b, E);
    if (rc) return rc;
    const size_t LN = h->LN();
    HIPCHK(hipMemcpyAsync(h->d_db, pts, sizeof(u64) * (size_t)K * b * E * LN, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->cx.masks, masks, sizeof(u64) * (size_t)b * LN, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return make_masks_sigma(h);
}

// Another query slot on the same database: `h` takes `owner`'s relinearisation key, database and masks by reference (device
// pointers; nothing is copied) and gets a run() workspace of its own, so that run() calls on the two handles -- each on its
// own stream -- overlap.  One query's stage A is HBM-bound while another's transforms are ALU-bound: two handles with one
// queue each finish two queries 10 % sooner than one handle with two queues finishes them one after the other (DESIGN.md
// section 6).  The owner must outlive the borrower and must not reload its key or database while the borrower is in use.
int piehip_attach_database(piehip_handle h, piehip_handle owner)
{
    NEED(h);
    if (!owner || owner == h) return fail(PIEHIP_EINVAL, "attach_database: needs another handle");
    if (h->slice.on || owner->slice.on) return fail(PIEHIP_ESTATE, "attach_database: a query-sliced handle neither lends nor borrows a database");
    if (h->db_borrowers)  // its key and database are in use by the handles attached to it: nothing of them may be freed
        return fail(PIEHIP_ESTATE, "attach_database: other handles are attached to this handle's database (detach or destroy them first)");
    join_pending(owner);
    if (owner->db_borrowed) return fail(PIEHIP_EINVAL, "attach_database: the owner itself borrows its database");
    // (an owner that hands out unrelinearised results of a K = 2 database runs without a key: so may its slots, each by its own setting)
    if (!owner->d_db || (!owner->cx.evk && owner->K > 1 && !(owner->K == 2 && !owner->res_relin))) return fail(PIEHIP_ESTATE, "attach_database: the owner has no key or no database yet");
    if (owner->device != h->device) return fail(PIEHIP_EINVAL, "attach_database: handles on different devices");
    if (owner->hp.N != h->hp.N || owner->hp.L != h->hp.L || owner->hp.t != h->hp.t || owner->hp.moduli != h->hp.moduli)
        return fail(PIEHIP_EINVAL, "attach_database: handles with different parameters");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(owner->stream));  // uploads of the owner's key / database have landed
    if (!h->db_borrowed)
        for (u64 **p : {&h->cx.evk, &h->cx.evk_sigma, &h->d_db, &h->cx.masks, &h->cx.masks_sigma}) dev_free(p);
    detach_database(h);
    h->K = h->b = h->E = 0;
    int rc = alloc_run_buffers(h, owner->K, owner->b, owner->E, false);
    if (rc) return rc;
    share_database(h, owner);
    h->db_borrowed = true;
    h->db_owner = owner;
    owner->db_borrowers++;
    return level_sync(h);   // a slot has its own chain-limbs setting, and its own copies of the owner's key and masks for it
}

// Layer tiling: R bin layers side by side in one slot vector leave b' = ceil(b / R) tiled layers.  The encoder's input is
// [max(K b E, b)][B] words -- the database's slot vectors, then the masks' in the same scratch -- for the b and B it encodes:
// b' and R k e with a tiling
static u32 tiled_layers(u32 b, u32 R) { return (u32)(((u64)b + R - 1) / R); }
static size_t slot_scratch_words(u32 K, u32 b, u32 E, size_t B)
{
    const size_t npt = (size_t)K * b * E;
    return (npt > b ? npt : b) * B;
}
// what every loader that reads the setting refuses: more tiled slots than the ring has
static int tiling_check(const piehip_ctx *h, u32 k, u32 e)
{
    if ((size_t)h->tiling * k * e > h->hp.N) return fail(PIEHIP_EINVAL, "layer tiling: R*k*e exceeds the ring dimension");
    return PIEHIP_OK;
}

// the persistent hash-table buffer [k][e][K][b][E]: reallocated only when the size changes
extern "C++" int piehip::hash_tbl_alloc(piehip_ctx *h, size_t words)
{
    if (h->d_hash_tbl && h->hash_tbl_words == words) return PIEHIP_OK;
    dev_free(&h->d_hash_tbl);
    h->hash_tbl_words = 0;
    int rc = dev_alloc(&h->d_hash_tbl, words);
    if (rc) return rc;
    h->hash_tbl_words = words;
    return PIEHIP_OK;
}

// A table built elsewhere, tbl[k][e][K][b][E] in host memory, as far as the encoder: into the handle's table buffer, its rows shuffled
// whole (every handle given the same seed holds one and the same database), its slot vectors gathered into *d_slots
// [max(K b E, b)][k e], carved from the caller's scratch (R > 1: the tiled vectors, [max(K b' E, b')][R k e])
extern "C++" int piehip::table_to_slots(piehip_ctx *h, Tmp &tmp, const u64 *tbl, u32 k, u32 e, u32 K, u32 b, u32 E, u64 shuffle_seed, int64_t **d_slots, u32 R)
{
    const size_t B = (size_t)k * e, npt = (size_t)K * b * E, tbl_words = B * npt;
    const int rc = hash_tbl_alloc(h, tbl_words);
    if (rc) return rc;
    h->hk = k, h->he = e, h->hb = b;
    TMPGET(d_slotsw, slot_scratch_words(K, tiled_layers(b, R), E, R * B));
    TMPGET(d_failw, 1);
    *d_slots = (int64_t *)d_slotsw;
    u32 *d_fail = (u32 *)d_failw;
    HIPCHK(hipMemcpyAsync(h->d_hash_tbl, tbl, tbl_words * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(d_fail, 0, sizeof(u32), h->stream));
    launch_shuffle_rows(h->d_hash_tbl, (u32)(B * K), b, E, shuffle_seed, h->stream);
    if (R > 1) launch_gather_slots_tiled(h->d_hash_tbl, (u32)B, R, K, b, E, h->hp.t, *d_slots, d_fail, h->stream);
    else launch_gather_slots(h->d_hash_tbl, (u32)B, K, b, E, h->hp.t, *d_slots, d_fail, h->stream);
    HIPCHK(hipGetLastError());  // (as in piehip_build_db_bins)
    u32 failed = 0;
    HIPCHK(hipMemcpyAsync(&failed, d_fail, sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (failed & 2u) return fail(PIEHIP_EINVAL, "server item does not fit the plaintext modulus");
    return PIEHIP_OK;
}

// scratch words piehip_build_db_bins carves (256-byte granules), including the encoder's
static size_t build_db_scratch_words(const piehip_ctx *h, size_t n, u32 k, u32 e, u32 K, u32 b, u32 E, u32 R)
{
    auto g = [](size_t w) { return ((w ? w : 1) + 31) & ~(size_t)31; };
    const size_t B = (size_t)k * e;
    return g((size_t)(k + K) * 16 * 256) + g(n) + 2 * g(n + 1) + g((e + 2) / 2 + 1) + g(1) + g(hash_sort_temp_bytes((u32)n, e) / 8 + 1) +
           g(slot_scratch_words(K, tiled_layers(b, R), E, R * B)) + g((size_t)ENCODE_CHUNK * h->hp.N);
}

int piehip_load_db_slots(piehip_handle h, uint32_t K, uint32_t b, uint32_t E, uint32_t B, const int64_t *slots,
                         const int64_t *mask_slots)
{
    NEED(h);
    if (!slots || !mask_slots) return fail(PIEHIP_EINVAL, "null database");
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size exceeds the ring dimension");
    HIPCHK(hipSetDevice(h->device));
    int rc = alloc_run_buffers(h, K, b, E);
    if (rc) return rc;
    const size_t npt = (size_t)K * b * E;
    int64_t *d_s = nullptr;
    HIPCHK(hipMalloc((void **)&d_s, sizeof(int64_t) * (npt > b ? npt : b) * B));
    hipError_t e = hipMemcpy(d_s, slots, sizeof(int64_t) * npt * B, hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = encode_on_device(h, d_s, (u32)npt, B, h->d_db);
    if (e == hipSuccess && rc == PIEHIP_OK) e = hipMemcpy(d_s, mask_slots, sizeof(int64_t) * (size_t)b * B, hipMemcpyHostToDevice);
    if (e == hipSuccess && rc == PIEHIP_OK) rc = encode_on_device(h, d_s, b, B, h->cx.masks);
    (void)hipFree(d_s);
    if (e != hipSuccess) return fail(PIEHIP_EHIP, std::string("load_db_slots: ") + hipGetErrorString(e));
    if (rc) return rc;
    return make_masks_sigma(h);
}

// Last step of the constructor (BatchedFHEHIPPIE.cpp:45-82) for the bin layers [lo, hi) this handle keeps: MakePackedPlaintext
// of the gathered slot vectors d_slots[K][b][E][B] into the database [K][hi - lo][E], then the masks of those layers (drawn per
// layer from mask_seed, so every shard of a sharded server holds the masks the unsharded one would).  Overwrites d_slots.
// With a layer tiling R > 1, b counts tiled layers and B = R k e: tiled layer g's mask is the masks of layers g R .. g R + R - 1 one
// after the other -- the draw of b R layers on k e slots, read as [b][R k e] (the layer index runs on past the last bin layer).
static int encode_bin_layers(piehip_ctx *h, int64_t *d_slots, u32 K, u32 b, u32 E, u32 B, u32 lo, u32 hi, u64 mask_seed, u32 R = 1)
{
    const u32 nb = hi - lo;
    const size_t LN = h->LN();
    int rc;
    for (u32 hf = 0; hf < K; hf++)
        if ((rc = encode_on_device(h, d_slots + ((size_t)hf * b + lo) * E * B, nb * E, B, h->d_db + (size_t)hf * nb * E * LN))) return rc;
    launch_mask_slots(h->hp.t, b * R, B / R, mask_seed, d_slots, h->stream);
    if ((rc = encode_on_device(h, d_slots + (size_t)lo * B, nb, B, h->cx.masks))) return rc;
    return make_masks_sigma(h);
}

// TabulationHashing tables (TabulationHashing.cpp:16-36): [nfun][16][256], drawn in that order from
// std::mt19937(seed) through std::uniform_int_distribution<uint64_t> -- the library types themselves, so the
// stream is the reference's under libstdc++.
static void tabulation_tables(uint64_t seed, uint32_t nfun, std::vector<u64> &tab)
{
    tab.resize((size_t)nfun * 16 * 256);
    std::mt19937 gen(seed);
    std::uniform_int_distribution<uint64_t> dis;
    for (auto &v : tab) v = dis(gen);
}

int piehip_tabulation_hash(uint64_t hash_seed, uint32_t nfun, uint32_t hf, const uint64_t *x, size_t n, uint64_t *out)
{
    if (!x || !out || hf >= nfun) return fail(PIEHIP_EINVAL, "bad argument");
    std::vector<u64> tab;
    tabulation_tables(hash_seed, nfun, tab);
    const u64 *t = tab.data() + (size_t)hf * 16 * 256;
    for (size_t a = 0; a < n; a++) {
        u64 v = x[a], res = 0;
        for (int i = 0; i < 16; i++) {
            res ^= t[i * 256 + (v & 0xff)];
            v >>= 8;
        }
        out[a] = res;
    }
    return PIEHIP_OK;
}

// The client's table (host side, no device): CuckooHashTable(hash, e, k, startingHashId 0, stash 0, multi tables, 1 layer),
// insertAll (BatchedFHEPSIClient.cpp:97-99,109; insert / eviction walk at CuckooHashTable.cpp:72-114, 1000 retries).
int piehip_client_cuckoo_table(uint64_t hash_seed, uint32_t nfun, uint32_t k, uint32_t e, const uint64_t *items, size_t n,
                               uint64_t *table)
{
    if (!items || !table || !k || !e || k > nfun) return fail(PIEHIP_EINVAL, "bad argument");
    std::vector<u64> tab;
    tabulation_tables(hash_seed, nfun, tab);
    auto pos = [&](u64 x, u32 hf) -> size_t {
        const u64 *t = tab.data() + (size_t)hf * 16 * 256;
        u64 v = x, res = 0;
        for (int i = 0; i < 16; i++) {
            res ^= t[i * 256 + (v & 0xff)];
            v >>= 8;
        }
        return (size_t)(res % e);
    };
    std::fill(table, table + (size_t)k * e, 0);
    for (size_t a = 0; a < n; a++) {
        u64 x = items[a];
        bool dup = false;
        for (u32 hf = 0; hf < k; hf++) dup = dup || table[(size_t)hf * e + pos(x, hf)] == x;  // lookUp
        if (dup) continue;
        bool placed = false;
        for (int retry = 0; retry < 1000 && !placed; retry++) {  // numberOfRetries
            for (u32 hf = 0; hf < k; hf++) {
                u64 &slot = table[(size_t)hf * e + pos(x, hf)];
                if (slot == 0) {
                    slot = x;
                    placed = true;
                    break;
                }
                std::swap(x, slot);  // one layer: evict the occupant and carry it to the next table
            }
        }
        if (!placed) return fail(PIEHIP_EHASH, "(Blocked) Cuckoo hashing error");
    }
    return PIEHIP_OK;
}

int piehip_reserve(piehip_handle h, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E, uint32_t bin_lo, uint32_t bin_hi)
{
    NEED(h);
    if (k < 1 || e < 1 || bin_lo >= bin_hi || bin_hi > tiled_layers(b, h->tiling) || !n || n > 0x7FFFFFFFu) return fail(PIEHIP_EINVAL, "bad shape");
    if (K < 2) return fail(PIEHIP_EINVAL, "Cuckoo Table needs more than one hash function!");  // CuckooHashTable.cpp:39-42
    if (h->tiling > 1 && tiling_check(h, k, e)) return PIEHIP_EINVAL;
    HIPCHK(hipSetDevice(h->device));
    int rc = alloc_run_buffers(h, K, bin_hi - bin_lo, E);
    if (rc) return rc;
    if ((rc = hash_tbl_alloc(h, (size_t)k * e * K * b * E))) return rc;
    const size_t need = build_db_scratch_words(h, n, k, e, K, b, E, h->tiling);
    if (h->arena_words < need) {
        if (h->arena_used) return fail(PIEHIP_ESTATE, "scratch in use");
        dev_free(&h->arena);
        h->arena_words = 0;
        if ((rc = dev_alloc(&h->arena, need))) return rc;
        h->arena_words = need;
    }
    // the input buffers of query 0 too (setIndex / setMinusCompareElement from host memory)
    u64 *di = nullptr, *dm = nullptr;
    return query_input_buffers(h, 0, &di, &dm);
}

// The offline phase as far as the encoder (BatchedFHEHIPPIE.cpp:45-66): the server set hashed into the handle's table buffer
// [k][e][K][b][E] on the device, its rows shuffled, its slot vectors gathered into *d_slots [max(K b E, b)][k e], carved from the
// caller's scratch (piehip_build_db_bins, piehip_build_db_sliced); R > 1: the tiled vectors, [max(K b' E, b')][R k e]
extern "C++" int piehip::items_to_slots(piehip_ctx *h, Tmp &tmp, const u64 *items, size_t n, u32 k, u32 e, u32 K, u32 b, u32 E, u64 hash_seed,
                                        u64 evict_seed, u64 shuffle_seed, int64_t **d_slots_out, u32 R)
{
    const size_t B = (size_t)k * e;
    const size_t tbl_words = B * K * b * E;
    int rc;
    if ((rc = hash_tbl_alloc(h, tbl_words))) return rc;
    h->hk = k;
    h->he = e;
    h->hb = b;
    std::vector<u64> tab;
    tabulation_tables(hash_seed, k + K, tab);
    TMPGET(d_tab, tab.size());
    TMPGET(d_items, n);
    TMPGET(d_keys, n + 1);      // 2 n u32
    TMPGET(d_vals, n + 1);      // 2 n u32
    TMPGET(d_start, (e + 2) / 2 + 1);
    TMPGET(d_failw, 1);
    const size_t temp_bytes = hash_sort_temp_bytes((u32)n, e);
    TMPGET(d_temp, temp_bytes / 8 + 1);
    TMPGET(d_slotsw, slot_scratch_words(K, tiled_layers(b, R), E, R * B));
    int64_t *d_slots = (int64_t *)d_slotsw;
    u32 *d_fail = (u32 *)d_failw;
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_items, items, n * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_hash_tbl, 0, tbl_words * sizeof(u64), h->stream));
    HIPCHK(hipMemsetAsync(d_fail, 0, sizeof(u32), h->stream));
    {
        ProfScope ps(h, PIEHIP_K_OTHER, 8.0 * (double)n * k * 4);
        HIPCHK(launch_hash_build(d_tab, d_items, (u32)n, k, e, K, b, E, evict_seed, shuffle_seed, h->d_hash_tbl, (u32 *)d_keys,
                                 (u32 *)d_vals, (u32 *)d_start, d_temp, temp_bytes, d_fail, h->stream));
        if (R > 1) launch_gather_slots_tiled(h->d_hash_tbl, (u32)B, R, K, b, E, h->hp.t, d_slots, d_fail, h->stream);
        else launch_gather_slots(h->d_hash_tbl, (u32)B, K, b, E, h->hp.t, d_slots, d_fail, h->stream);
        HIPCHK(hipGetLastError());  // a launch that failed would leave d_slots uninitialised for the encoder
    }
    u32 failed = 0;
    HIPCHK(hipMemcpyAsync(&failed, d_fail, sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (failed & 1u) return fail(PIEHIP_EHASH, "(Blocked) Cuckoo hashing error");
    if (failed & 2u) return fail(PIEHIP_EINVAL, "server item does not fit the plaintext modulus");
    *d_slots_out = d_slots;
    return PIEHIP_OK;
}

int piehip_build_db_bins(piehip_handle h, const uint64_t *items, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                         uint64_t hash_seed, uint64_t evict_seed, uint64_t shuffle_seed, uint64_t mask_seed, uint32_t bin_lo,
                         uint32_t bin_hi)
{
    NEED(h);
    if (!items || !n || n > 0x7FFFFFFFu) return fail(PIEHIP_EINVAL, "empty or oversized server set");
    if (k < 1 || e < 1) return fail(PIEHIP_EINVAL, "need at least one outer hash function and position");
    if (K < 2) return fail(PIEHIP_EINVAL, "Cuckoo Table needs more than one hash function!");  // CuckooHashTable.cpp:39-42
    const u32 R = h->tiling;  // bin_lo, bin_hi count tiled layers
    if (bin_lo >= bin_hi || bin_hi > tiled_layers(b, R)) return fail(PIEHIP_EINVAL, "bin-layer slice must be non-empty and within [0, b)");
    const size_t B = (size_t)k * e;
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size k*e exceeds the ring dimension");
    if (tiling_check(h, k, e)) return PIEHIP_EINVAL;
    HIPCHK(hipSetDevice(h->device));
    int rc = alloc_run_buffers(h, K, bin_hi - bin_lo, E);
    if (rc) return rc;
    Tmp tmp(h);
    int64_t *d_slots = nullptr;
    if ((rc = items_to_slots(h, tmp, items, n, k, e, K, b, E, hash_seed, evict_seed, shuffle_seed, &d_slots, R))) return rc;
    return encode_bin_layers(h, d_slots, K, tiled_layers(b, R), E, R * (u32)B, bin_lo, bin_hi, mask_seed, R);
}

int piehip_build_db(piehip_handle h, const uint64_t *items, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                    uint64_t hash_seed, uint64_t evict_seed, uint64_t shuffle_seed, uint64_t mask_seed)
{
    return piehip_build_db_bins(h, items, n, k, e, K, b, E, hash_seed, evict_seed, shuffle_seed, mask_seed, 0, h ? tiled_layers(b, h->tiling) : b);
}

int piehip_load_db_table_bins(piehip_handle h, const uint64_t *tbl, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                              uint64_t shuffle_seed, uint64_t mask_seed, uint32_t bin_lo, uint32_t bin_hi)
{
    NEED(h);
    if (!tbl || k < 1 || e < 1) return fail(PIEHIP_EINVAL, "bad hash table");
    if (K < 2) return fail(PIEHIP_EINVAL, "Cuckoo Table needs more than one hash function!");  // CuckooHashTable.cpp:39-42
    const u32 R = h->tiling;  // bin_lo, bin_hi count tiled layers
    if (bin_lo >= bin_hi || bin_hi > tiled_layers(b, R)) return fail(PIEHIP_EINVAL, "bin-layer slice must be non-empty and within [0, b)");
    const size_t B = (size_t)k * e;
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size k*e exceeds the ring dimension");
    if (tiling_check(h, k, e)) return PIEHIP_EINVAL;
    HIPCHK(hipSetDevice(h->device));
    int rc = alloc_run_buffers(h, K, bin_hi - bin_lo, E);
    if (rc) return rc;
    Tmp tmp(h);
    int64_t *d_slots = nullptr;
    if ((rc = table_to_slots(h, tmp, tbl, k, e, K, b, E, shuffle_seed, &d_slots, R))) return rc;
    return encode_bin_layers(h, d_slots, K, tiled_layers(b, R), E, R * (u32)B, bin_lo, bin_hi, mask_seed, R);
}

int piehip_load_db_table(piehip_handle h, const uint64_t *tbl, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                         uint64_t shuffle_seed, uint64_t mask_seed)
{
    return piehip_load_db_table_bins(h, tbl, k, e, K, b, E, shuffle_seed, mask_seed, 0, h ? tiled_layers(b, h->tiling) : b);
}

int piehip_get_hash_table(piehip_handle h, uint64_t *tbl)
{
    NEED(h);
    if (!tbl) return fail(PIEHIP_EINVAL, "null out");
    if (!h->d_hash_tbl) return fail(PIEHIP_ESTATE, "no table: call piehip_build_db first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(tbl, h->d_hash_tbl, sizeof(u64) * (size_t)h->hk * h->he * h->K * h->hb * h->E, hipMemcpyDeviceToHost));
    return PIEHIP_OK;
}

// ---- layer tiling (include/piehip.h "Layer tiling") -------------------------------------------------------------------------
int piehip_set_layer_tiling(piehip_handle h, uint32_t R)
{
    NEED_RO(h);
    if (R < 1) return fail(PIEHIP_EINVAL, "layer tiling: at least one bin layer per slot vector");
    h->tiling = R;
    return PIEHIP_OK;
}
int piehip_get_layer_tiling(piehip_handle h, uint32_t *R)
{
    NEED_RO(h);
    if (!R) return fail(PIEHIP_EINVAL, "null out");
    *R = h->tiling;
    return PIEHIP_OK;
}
int piehip_layer_tiling(uint32_t N, uint32_t k, uint32_t e, uint32_t b, uint32_t *R, uint32_t *b_tiled)
{
    if (!R || !b_tiled || !k || !e || !b) return fail(PIEHIP_EINVAL, "layer_tiling: null out or empty shape");
    const uint64_t rmax = (uint64_t)N / ((uint64_t)k * e);
    if (!rmax) return fail(PIEHIP_EINVAL, "batch size k*e exceeds the ring dimension");
    const uint32_t most = rmax < b ? (uint32_t)rmax : b;
    *b_tiled = (b + most - 1) / most;
    *R = (b + *b_tiled - 1) / *b_tiled;
    return PIEHIP_OK;
}

// ---- query inputs ---------------------------------------------------------------------------------------------------------
// Query q of the batch (piehip_set_query_batch; a handle without a batch has query 0 only, which the plain names set).
static int batch_query_check(piehip_ctx *h, u32 q)
{
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    return PIEHIP_OK;
}
// a host array to the owned device copy of one input of a query, which the next run() then reads
static int upload_input(piehip_ctx *h, const uint64_t *src, size_t words, u64 **own, const u64 **in)
{
    HIPCHK(hipSetDevice(h->device));
    int rc;
    if (!*own && (rc = dev_alloc(own, words))) return rc;
    HIPCHK(hipMemcpyAsync(*own, src, words * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *in = *own;
    return PIEHIP_OK;
}
int piehip_set_index_q(piehip_handle h, uint32_t q, const uint64_t *idx)
{
    NEED(h);
    if (!idx) return fail(PIEHIP_EINVAL, "null index matrix");
    if (!h->K) return fail(PIEHIP_ESTATE, "load the database before the index matrix");
    int rc = batch_query_check(h, q);
    if (rc) return rc;
    return upload_input(h, idx, (size_t)h->K * h->E * 2 * h->LN(), &h->query[q].idx_own, &h->query[q].idx);
}
int piehip_set_minus_q(piehip_handle h, uint32_t q, const uint64_t *minus)
{
    NEED(h);
    if (!minus) return fail(PIEHIP_EINVAL, "null minus element");
    int rc = batch_query_check(h, q);
    if (rc) return rc;
    return upload_input(h, minus, 2 * h->LN(), &h->query[q].minus_own, &h->query[q].minus);
}
int piehip_set_index_device_q(piehip_handle h, uint32_t q, const void *d_idx)
{
    NEED(h);
    if (!d_idx) return fail(PIEHIP_EINVAL, "null index matrix");
    int rc = batch_query_check(h, q);
    if (rc) return rc;
    h->query[q].idx = (const u64 *)d_idx;
    return PIEHIP_OK;
}
int piehip_set_minus_device_q(piehip_handle h, uint32_t q, const void *d_minus)
{
    NEED(h);
    if (!d_minus) return fail(PIEHIP_EINVAL, "null minus element");
    int rc = batch_query_check(h, q);
    if (rc) return rc;
    h->query[q].minus = (const u64 *)d_minus;
    return PIEHIP_OK;
}
int piehip_set_index(piehip_handle h, const uint64_t *idx) { return piehip_set_index_q(h, 0, idx); }
int piehip_set_minus(piehip_handle h, const uint64_t *minus) { return piehip_set_minus_q(h, 0, minus); }
int piehip_set_index_device(piehip_handle h, const void *d_idx) { return piehip_set_index_device_q(h, 0, d_idx); }
int piehip_set_minus_device(piehip_handle h, const void *d_minus) { return piehip_set_minus_device_q(h, 0, d_minus); }

// ---- query batches --------------------------------------------------------------------------------------------------------
// run() over nq queries at once (each with its own index matrix and minus element) against the handle's database.  Stage A
// reads every database plaintext once for the batch instead of once per query, and every later launch works on nq times as
// many ciphertexts.  Rows of the workspace and of the results: [bin layer][query].
int piehip_set_query_batch(piehip_handle h, uint32_t nq)
{
    NEED(h);
    if (nq < 1 || nq > STAGE_A_MAX_QUERIES) return fail(PIEHIP_EINVAL, "set_query_batch: between 1 and 8 queries per run()");
    if (nq == h->nq) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    h->forget_rows();
    h->stage_open = false;
    // caller-owned device pointers of queries outside the new batch are forgotten (they may be freed by now); a later, larger
    // batch must set them again.  Per-query keys are sized by the batch: load them again after a change.
    for (u32 q = nq; q < STAGE_A_MAX_QUERIES; q++) h->query[q].idx = h->query[q].minus = nullptr;
    dev_free(&h->cx.evkq);
    dev_free(&h->cx.evkq_sigma);
    h->evkq_n = h->evkq_loaded = 0;
    h->nq = nq;
    if (!h->K) return PIEHIP_OK;  // the database's arrival sizes the workspace
    const int rc = alloc_workspace(h, h->K, h->b);
    return rc ? rc : slice_batch_changed(h);
}
int piehip_get_query_batch(piehip_handle h, uint32_t *nq)
{
    NEED_RO(h);
    if (!nq) return fail(PIEHIP_EINVAL, "null out");
    *nq = h->nq;
    return PIEHIP_OK;
}

// The queries of a batch come from different clients (BatchedFHEPSIServer.cpp:94-95: one client per connection), and every client
// has its own EvalMult key (.cpp:45-49): query q's key switch takes key q.  The key-switch kernel already selects its key per
// ciphertext row (FHEHIPPIE's EvalMerge: one rotation key per position); rows of a batch are [bin layer][query], so row r
// takes key r % nq.
int piehip_load_relin_key_q(piehip_handle h, uint32_t q, const uint64_t *evk)
{
    NEED(h);
    if (!evk) return fail(PIEHIP_EINVAL, "null evk");
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    HIPCHK(hipSetDevice(h->device));
    ChainCtx &c = h->cx;
    const size_t words = c.key_words(), rows = c.L * 2 * c.L;   // of one key
    int rc;
    if (!c.evkq || h->evkq_n != h->nq) {
        // a captured run() names the key array it was captured with: the handle's key where there was no per-query array yet
        // (a handle without a batch reads query 0's own key from here on), the array freed below otherwise
        HIPCHK(hipStreamSynchronize(h->stream));
        drop_graph(h);
        dev_free(&c.evkq);
        dev_free(&c.evkq_sigma);
        h->evkq_n = h->evkq_loaded = 0;
        if ((rc = dev_alloc(&c.evkq, words * h->nq))) return rc;
        if (h->plan.lane_order && (rc = dev_alloc(&c.evkq_sigma, words * h->nq))) return rc;
        h->evkq_n = h->nq;
        // queries without a key of their own use the handle's (piehip_load_relin_key), if it has one
        if ((rc = fill_unloaded_key_slots(h))) return rc;
    }
    HIPCHK(hipMemcpyAsync(c.evkq + q * words, evk, words * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    if ((rc = lane_twin(h, c, c.evkq, &c.evkq_sigma, h->nq * rows, q * rows, rows))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->evkq_loaded |= 1u << q;
    return level_sync(h);
}

// Seeded EvalMult keys: the L first components come from the host, the L second ones are expanded from their seeds on the device;
// the assembled key then loads as an unseeded one (offline phase: the key crosses the link twice, half of it each way).
static int assemble_seeded_key(piehip_ctx *h, const uint64_t *evk0, const uint8_t *seeds, std::vector<u64> &key)
{
    const u32 L = h->hp.L;
    const size_t LN = h->LN();
    key.resize((size_t)L * 2 * LN);
    u64 *d = nullptr;
    int rc = dev_alloc(&d, (size_t)L * LN);
    if (rc) return rc;
    std::vector<SeedJob> jobs(L);
    for (u32 i = 0; i < L; i++) jobs[i] = seed_job(d + (size_t)i * LN, seeds + (size_t)i * 32);
    rc = expand_seeded_sync(h, jobs);
    for (u32 i = 0; i < L && !rc; i++) {
        memcpy(&key[(size_t)i * 2 * LN], evk0 + (size_t)i * LN, LN * sizeof(u64));
        if (hipMemcpy(&key[((size_t)i * 2 + 1) * LN], d + (size_t)i * LN, LN * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(PIEHIP_EHIP, "load_relin_key_seeded: copy-out failed");
    }
    dev_free(&d);
    return rc;
}

int piehip_load_relin_key_seeded(piehip_handle h, const uint64_t *evk0, const uint8_t *seeds)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!evk0 || !seeds) return fail(PIEHIP_EINVAL, "null evk0 or seeds");
    if (h->db_borrowed) return fail(PIEHIP_EINVAL, "this handle uses another handle's key and database (piehip_attach_database)");
    if (h->db_borrowers) return fail(PIEHIP_ESTATE, "the key cannot be reloaded while other handles are attached to this one");
    NEED(h);
    std::vector<u64> key;
    int rc = assemble_seeded_key(h, evk0, seeds, key);
    return rc ? rc : piehip_load_relin_key(h, key.data());
}

int piehip_load_relin_key_seeded_q(piehip_handle h, uint32_t q, const uint64_t *evk0, const uint8_t *seeds)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!evk0 || !seeds) return fail(PIEHIP_EINVAL, "null evk0 or seeds");
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    NEED(h);
    std::vector<u64> key;
    int rc = assemble_seeded_key(h, evk0, seeds, key);
    return rc ? rc : piehip_load_relin_key_q(h, q, key.data());
}

int piehip_set_transform_slots(piehip_handle h, uint32_t n)
{
    NEED_RO(h);
    h->plan.max_slots = n;
    for (auto &kv : h->levels) kv.second->plan.max_slots = n;
    drop_graph(h);   // a captured run() has the old grids baked in
    return PIEHIP_OK;
}

int piehip_get_transform_slots(piehip_handle h, uint32_t *n, uint32_t *device_slots)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (n) *n = h->plan.max_slots;
    if (device_slots) *device_slots = 2 * h->plan.num_cus;
    return PIEHIP_OK;
}

int piehip_sync(piehip_handle h)
{
    NEED_RO(h);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PIEHIP_OK;
}

// Result limbs (include/piehip.h): the setting of a handle.  The full-width rows the reduction reads are allocated here, outside the
// timed path, and stay with the workspace: going back and forth between settings allocates nothing.
int piehip_set_result_limbs(piehip_handle h, uint32_t keep)
{
    NEED(h);
    if (keep < 1 || keep > h->hp.L) return fail(PIEHIP_EINVAL, "set_result_limbs: keep must be between 1 and L");
    if (keep < h->hp.L && h->use_graph)
        return fail(PIEHIP_ESTATE, "set_result_limbs: a handle that replays a captured graph (piehip_set_graph) hands out full results");
    HIPCHK(hipSetDevice(h->device));
    h->forget_rows();
    const u32 before = h->res_limbs;
    h->res_limbs = keep;
    const int rc = ensure_full_rows(h, h->K);
    if (rc) h->res_limbs = before;
    return rc;
}
int piehip_get_result_limbs(piehip_handle h, uint32_t *keep)
{
    NEED_RO(h);
    if (!keep) return fail(PIEHIP_EINVAL, "null out");
    *keep = h->res_limbs;
    return PIEHIP_OK;
}

// Result relinearisation (include/piehip.h): the setting of a handle.  Like the result limbs' rows, the larger result rows and the
// last product's scratch are allocated here, outside the timed path, and stay with the workspace.
int piehip_set_result_relin(piehip_handle h, int on)
{
    NEED(h);
    if (!on && h->use_graph)
        return fail(PIEHIP_ESTATE, "set_result_relin: a handle that replays a captured graph (piehip_set_graph) relinearises its results");
    if (!on && h->slice.on) return fail(PIEHIP_ESTATE, "set_result_relin: a query-sliced handle relinearises its results");
    HIPCHK(hipSetDevice(h->device));
    h->forget_rows();
    const bool before = h->res_relin;
    h->res_relin = on != 0;
    const int rc = ensure_full_rows(h, h->K);
    if (rc) h->res_relin = before;
    return rc;
}
int piehip_get_reduction(piehip_handle h, uint32_t *kind)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!kind) return fail(PIEHIP_EINVAL, "null out");
    *kind = h->plan.fold_moduli ? 2u : h->plan.small_moduli ? 1u : 0u;
    return PIEHIP_OK;
}
int piehip_get_level_reduction(piehip_handle h, uint32_t Lc, uint32_t *kind)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!kind) return fail(PIEHIP_EINVAL, "null out");
    if (Lc < 1 || Lc > h->hp.L) return fail(PIEHIP_EINVAL, "get_level_reduction: Lc must be between 1 and L");
    if (Lc < h->hp.L && !h->levels.count(Lc)) return fail(PIEHIP_ESTATE, "get_level_reduction: no chain schedule has named this level yet");
    const NttPlan &pl = Lc == h->hp.L ? h->plan : h->levels.at(Lc)->plan;
    *kind = pl.fold_moduli ? 2u : pl.small_moduli ? 1u : 0u;
    return PIEHIP_OK;
}
int piehip_get_result_relin(piehip_handle h, int *on)
{
    NEED_RO(h);
    if (!on) return fail(PIEHIP_EINVAL, "null out");
    *on = h->res_relin ? 1 : 0;
    return PIEHIP_OK;
}
int piehip_get_result_components(piehip_handle h, uint32_t *ncomp)
{
    NEED_RO(h);
    if (!ncomp) return fail(PIEHIP_EINVAL, "null out");
    *ncomp = h->res_comps();
    return PIEHIP_OK;
}

// Chain limbs (include/piehip.h): a level context's copies of the keys and masks in the handle's context -- the limb prefix
// evk[i][c][j], i, j < Lc, of every EvalMult key and the first Lc limbs of the masks, each with its lane-ordered twin where the
// level's plan has a lane order (its own map: a prefix of a mixed chain may take other routes than the parent).  Copied on the
// handle's stream whenever the key or the database is set and when the setting changes: 8 and 7 MiB at C3 and as much again for
// the twins.  The other choice -- reading the parent's arrays in place through their strides -- would have put two more strides
// into the key-switch MAC, whose instantiations must stay what they are.
// With a schedule: the keys for every level below L on which a product of the chain runs, the masks for the last product's level
// alone (a level that a later product leaves behind multiplies no mask).
extern "C++" int piehip::level_sync(piehip_ctx *h)
{
    if (h->chain_floor() >= h->hp.L) return PIEHIP_OK;
    const ChainCtx &top = h->cx;
    const u32 products = h->K >= 2 ? h->K - 1 : 1, last = h->chain_last();
    bool any = false;
    for (u32 hf = 1; hf <= std::min(products, h->chain_n); hf++) {
        const u32 Lc = h->chain_level(hf);
        if (Lc >= h->hp.L || (hf > 1 && Lc == h->chain_level(hf - 1))) continue;
        LevelCtx *lv = h->levels.at(Lc).get();
        ChainCtx &c = lv->cx;
        const size_t row = c.LN() * sizeof(u64);
        // n blocks of `rows` rows of L N words, SW words apart at src -> blocks of as many rows of Lc N words, and their twin.  A copy
        // that is not made (nothing at src, no memory) is not kept: the level then has none, as the handle has none
        auto copy = [&](const u64 *src, size_t SW, u32 n, size_t rows, u64 **dst, u64 **twin, size_t *cap) -> int {
            const size_t bw = rows * c.LN();
            const bool grow = *cap < n * bw;
            if (!src || !n || grow) {
                dev_free(dst);
                dev_free(twin);
                *cap = 0;
            }
            if (!src || !n) return PIEHIP_OK;
            int rc = grow ? dev_alloc(dst, n * bw) : PIEHIP_OK;
            hipError_t e = hipSuccess;
            for (u32 i = 0; i < n && !rc && e == hipSuccess; i++)
                e = hipMemcpy2DAsync(*dst + i * bw, row, src + i * SW, top.LN() * sizeof(u64), row, rows, hipMemcpyDeviceToDevice, h->stream);
            if (e != hipSuccess) rc = fail(PIEHIP_EHIP, std::string("level_sync: ") + hipGetErrorString(e));
            if (!rc) rc = lane_twin(h, c, *dst, twin, n * rows * c.L);
            if (rc) {
                dev_free(dst);
                dev_free(twin);
            }
            if (rc || grow) *cap = rc ? 0 : n * bw;
            return rc;
        };
        int rc;
        if ((rc = copy(top.evk, 0, 1, 2 * c.L, &c.evk, &c.evk_sigma, &lv->evk_cap))) return rc;
        if ((rc = copy(top.evkq, top.key_words(), h->evkq_n, 2 * c.L, &c.evkq, &c.evkq_sigma, &lv->evkq_cap))) return rc;
        if (Lc == last && (rc = copy(top.masks, top.LN(), h->b ? 1 : 0, h->b, &c.masks, &c.masks_sigma, &lv->masks_cap))) return rc;
        any = true;
    }
    if (any) HIPCHK(hipStreamSynchronize(h->stream));
    return PIEHIP_OK;
}

// The setting of a handle.  A level context is built when the setting first names its limb count and kept: going back and forth
// allocates nothing (the copies of keys and masks are made again, on the handle's stream).
int piehip_set_chain_schedule(piehip_handle h, const uint32_t *Lc, uint32_t n)
{
    NEED(h);
    const u32 L = h->hp.L;
    if (!Lc) return fail(PIEHIP_EINVAL, "set_chain_schedule: null schedule");
    if (n < 1 || n > MAX_CHAIN_SCHED) return fail(PIEHIP_EINVAL, "set_chain_schedule: between 1 and 7 entries");
    for (u32 i = 0; i < n; i++) {
        if (Lc[i] < 1 || Lc[i] > L) return fail(PIEHIP_EINVAL, "set_chain_limbs: Lc must be between 1 and L");
        if (i && Lc[i] > Lc[i - 1]) return fail(PIEHIP_EINVAL, "set_chain_schedule: the limb counts must not increase along the chain");
    }
    const bool below = Lc[n - 1] < L;
    if (below && h->use_graph)
        return fail(PIEHIP_ESTATE, "set_chain_limbs: a handle that replays a captured graph (piehip_set_graph) runs the product chain on every limb");
    if (below && h->slice.on) return fail(PIEHIP_ESTATE, "set_chain_limbs: a query-sliced handle runs the product chain on every limb");
    HIPCHK(hipSetDevice(h->device));
    for (u32 i = 0; i < n; i++) {
        if (Lc[i] == L || h->levels.count(Lc[i])) continue;
        std::unique_ptr<LevelCtx> lv(new LevelCtx());
        std::string err = lv->hp.init(h->hp.N, Lc[i], h->hp.t, h->hp.moduli.data(), h->hp.moduli.data() + L);
        if (!err.empty()) return fail(PIEHIP_EINVAL, "set_chain_limbs: " + err);
        err = context_tables(h, lv->hp, lv->plan, &lv->d_dc, &lv->d_sigma_inv, nullptr);
        if (!err.empty()) return fail(PIEHIP_EHIP, "set_chain_limbs: " + err);   // (what was uploaded stays in dev_tables and goes with the handle)
        lv->plan.max_slots = h->plan.max_slots;
        lv->cx.d_dc = lv->d_dc, lv->cx.plan = &lv->plan, lv->cx.d_sigma_inv = lv->d_sigma_inv;
        lv->cx.N = h->hp.N, lv->cx.L = Lc[i], lv->cx.M = lv->hp.M;
        h->levels.emplace(Lc[i], std::move(lv));
    }
    h->forget_rows();
    u32 before[MAX_CHAIN_SCHED];
    const u32 n_before = h->chain_n;
    std::copy(h->chain_sched, h->chain_sched + MAX_CHAIN_SCHED, before);
    std::copy(Lc, Lc + n, h->chain_sched);
    h->chain_n = n;
    const int rc = level_sync(h);
    if (rc) std::copy(before, before + MAX_CHAIN_SCHED, h->chain_sched), h->chain_n = n_before;
    return rc;
}
int piehip_get_chain_schedule(piehip_handle h, uint32_t *Lc, uint32_t cap, uint32_t *n)
{
    NEED_RO(h);
    if (!n || (!Lc && cap)) return fail(PIEHIP_EINVAL, "null out");
    if (cap < h->chain_n) return fail(PIEHIP_EINVAL, "get_chain_schedule: room for fewer entries than the schedule has");
    std::copy(h->chain_sched, h->chain_sched + h->chain_n, Lc);
    *n = h->chain_n;
    return PIEHIP_OK;
}
int piehip_set_chain_limbs(piehip_handle h, uint32_t Lc) { return piehip_set_chain_schedule(h, &Lc, 1); }
int piehip_get_chain_limbs(piehip_handle h, uint32_t *Lc)
{
    NEED_RO(h);
    if (!Lc) return fail(PIEHIP_EINVAL, "null out");
    *Lc = h->chain_last();
    return PIEHIP_OK;
}

int piehip_get_results(piehip_handle h, uint64_t *out)
{
    NEED(h);
    if (!out) return fail(PIEHIP_EINVAL, "null out");
    if (!h->d_out) return fail(PIEHIP_ESTATE, "no results");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out, h->d_out, sizeof(u64) * (size_t)h->b * h->nq * h->res_ct_words(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PIEHIP_OK;
}
int piehip_results_device(piehip_handle h, void **d_out)
{
    NEED_RO(h);
    if (!h->d_out) return fail(PIEHIP_ESTATE, "no results");
    *d_out = h->d_out;
    return PIEHIP_OK;
}

int piehip_copy_results_device(piehip_handle h, void *d_dst)
{
    NEED(h);
    if (!d_dst) return fail(PIEHIP_EINVAL, "null destination");
    if (!h->d_out) return fail(PIEHIP_ESTATE, "no results");
    HIPCHK(hipMemcpyAsync(d_dst, h->d_out, sizeof(u64) * (size_t)h->b * h->nq * h->res_ct_words(), hipMemcpyDeviceToDevice, h->stream));
    return PIEHIP_OK;
}

}  // extern C
