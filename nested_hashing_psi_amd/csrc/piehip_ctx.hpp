// piehip_ctx.hpp -- what the translation units behind include/piehip.h share: the context behind a piehip_handle, error / ordering
// macros, device scratch, event-bracketed launches, the schedule pieces of a ciphertext multiplication and the Sched each is enqueued with.
//   piehip.cpp         context, keys, database (offline phase), query inputs
//   piehip_run.cpp     the schedule pieces of a ciphertext multiplication, run() and its queues
//   piehip_host.cpp    the host-memory path of a query: page-locked staging, piecewise uploads, run_staged / run_host
//   piehip_ops.cpp     the OpenFHE primitives one by one (parity tests), NTT timing, per-kernel profiling
//   piehip_fhepie.cpp  the rotation-based sibling operator (FHEHIPPIE)
//   piehip_client.cpp  client-side harness (key generation, encryption, decryption)
//   piehip_rccl.cpp    the collectives of a sharded server over RCCL: the query's broadcast, and the final gather and the scatter and
//                      exchange of query slices, whose transfers only exchange_plan.h knows (who sends what to whom, in which order; free of HIP)
//   piehip_slice.cpp   query-sliced stage A: a handle's (inner hash function, limb) units, the accumulators' way to the chain side
//                      (slice_geometry.h: the copies that bring its inputs up, free of HIP)
#pragma once
#include "../../include/piehip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "params.hpp"
#include "exchange_plan.h"
#include "slice_geometry.h"

namespace piehip {
int fail(int code, const std::string &msg);  // sets piehip_last_error() of this thread, returns code
}
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return piehip::fail(PIEHIP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)
struct piehip_ctx;
namespace piehip {
void join_pending(piehip_ctx *h);
void mark_dirty(piehip_ctx *h);
}
// every entry point except piehip_run first orders the handle's stream behind the bin-layer queues of earlier runs
#define NEED_RO(h)                                                       \
    do {                                                                 \
        if (!(h)) return piehip::fail(PIEHIP_EINVAL, "null handle");     \
        piehip::join_pending(h);                                         \
    } while (0)
// ... and, unless it only reads (NEED_RO), may queue work on the handle's stream that the next run has to wait for
#define NEED(h)                                                 \
    do {                                                        \
        NEED_RO(h);                                             \
        piehip::mark_dirty(h);                                  \
    } while (0)

namespace piehip {

struct ProfRec {
    hipEvent_t a, b;
    int k;
    double bytes;
};

// scratch of one batched EvalMult(ct,ct) over nb ciphertext pairs
struct MulWs {
    u32 nb = 0;
    u64 *eqp = nullptr;  // [nb][4][M][N]
    u64 *dqp = nullptr;  // [nb][3][M][N]
    u64 *d01 = nullptr;  // [nb][2][L][N]
    u64 *d2c = nullptr;  // [nb][L][N]
    u64 *dig = nullptr;  // [nb][L][L][N]
    u64 *t3 = nullptr;   // [nb][3][L][N]: a run()'s last product on its way to a degree-2 result (allocated with piehip_set_result_relin(0))
};

// one query of the batch (piehip_set_query_batch; a handle without a batch has query 0 only): its device inputs, and its way
// in from host memory (piehip_host_buffers_q, piehip_stage_*_q)
struct Query {
    const u64 *idx = nullptr, *minus = nullptr;    // what the next run() reads: [K][E][2][L][N], [2][L][N]; the caller's device
                                                   // arrays (piehip_set_*_device_q) or the owned ones below
    u64 *idx_own = nullptr, *minus_own = nullptr;  // owned copies: the host setters and the staged uploads write them
    u64 *pin_idx = nullptr, *pin_minus = nullptr;  // page-locked staging [K][E][2][L][N], [2][L][N]
    std::vector<bool> rows;                        // pieces on their way since the staging sequence began
    std::vector<bool> cts;                         // ... ciphertext by ciphertext (piehip_stage_index_ct_q), [K][E]
    bool minus_staged = false;
    // seeded pieces (piehip_stage_*_seeded_q): c0 is on its way, c1 is expanded from the seed at piehip_run_staged.
    // Index p < K E: index ciphertext p = row E + j; index K E: the minus element.  Staging a piece unseeded clears its entry.
    std::vector<bool> seeded;                      // [K E + 1]
    std::vector<u32> seeds;                        // [K E + 1][8]: the 32-byte seeds as little-endian words
};

// one input piece of one query on a query-sliced handle (SliceState::in below)
struct SliceInput {
    const u64 *cur = nullptr;   // what the next piehip_run_slice reads: the caller's device array (piehip_set_*_slice_device_q) or `own`
    u64 *own = nullptr;         // the owned device copy [u_n][cts][2][N]: the host setters write it
    // set seeded (piehip_set_*_slice_seeded*_q): the c0 rows are in `own`, the c1 rows are expanded from the seeds by the next
    // piehip_run_slice, which clears the mark.  Every other setter of the piece clears it too: nothing is expanded over it.
    bool seeded = false;
};
inline u32 piece_cts(int p, u32 E) { return p == SLICE_INDEX ? E : 1; }   // ciphertexts per unit
// where the seed of ciphertext j of unit u sits in the query's seed table [K E + 1][8]
inline size_t piece_seed_at(int p, u32 u, u32 j, u32 L, u32 K, u32 E) { return p == SLICE_INDEX ? (size_t)(u / L) * E + j : (size_t)K * E; }

// Query slices (piehip_slice.cpp; include/piehip.h "Query slices").  Unit u = h L + l is limb l of inner hash function h.  The handle
// holds the units [u_lo, u_hi) of the database for ALL b_total bin layers and computes those limbs of every accumulator (the slice
// side); it runs the product chain of the bin layers [bin_lo, bin_hi) (the chain side: piehip_ctx::b = bin_hi - bin_lo, masks and
// workspace as on any handle, no database) on the accumulators piehip_put_accumulators(_from) places there.
struct SliceState {
    bool on = false;
    u32 u_lo = 0, u_hi = 0;
    u32 bin_lo = 0, bin_hi = 0, b_total = 0;
    u64 *db = nullptr;    // [u_n][b_total][E][N]: one limb per unit
    u64 *acc = nullptr;   // [b_total][nq][u_n][2][N]: what piehip_run_slice writes
    u32 acc_nq = 0;       // the batch size acc was allocated for
    // slice inputs: in[q][p] is piece p (SLICE_INDEX [u_n][E][2][N], SLICE_MINUS [u_n][2][N]) of query q of the batch.  Every consumer
    // loops over the pieces; piece_cts and piece_seed_at above are all that tells them apart.
    SliceInput in[STAGE_A_MAX_QUERIES][SLICE_PIECES];
    std::vector<u32> seeds[STAGE_A_MAX_QUERIES];   // [K E + 1][8]: the query's seed tables as little-endian words, the minus seed last
    // the job table of that one expansion launch: written in page-locked memory, copied up on the handle's stream.  ev_jobs is recorded
    // behind the copy and waited for before the table is written again (piehip_slice.cpp, queue_slice_expansion)
    SeedLimbJob *pin_jobs = nullptr, *d_jobs = nullptr;   // [jobs_cap] each
    size_t jobs_cap = 0;
    hipEvent_t ev_jobs = nullptr;
    bool jobs_copied = false;          // ev_jobs has been recorded
    std::vector<bool> put;             // [K L]: units placed since the last piehip_run_chain or batch-size change
    hipEvent_t ev_ready = nullptr;     // recorded on this handle's stream for a reader of acc on another stream (piehip_put_accumulators_from),
    hipEvent_t ev_read = nullptr;      // ... and on this handle's stream behind its own placement launch, for the source to wait on
    // across the ranks of a sharded server (piehip_rccl.cpp; exchange_plan.h)
    u64 *pin_idx[STAGE_A_MAX_QUERIES] = {}, *pin_minus[STAGE_A_MAX_QUERIES] = {};   // piehip_slice_host_buffers_q: the whole query, page-locked
    u64 *scatter_stage = nullptr;      // the root's staging area [nq][idx[K L][E][2][N], minus[K L][2][N]], allocated at the first scatter of a shape
    size_t scatter_words = 0;
    u64 *xchg_stage = nullptr;         // the received blocks of the exchange, bin_n nq 2N K L words, allocated at the first exchange of a shape
    size_t xchg_words = 0;
    u32 u_n() const { return u_hi - u_lo; }
};

// Everything a product chain and its schedule pieces (ntt, enqueue_mul, enqueue_keyswitch, enqueue_mod_reduce) read beside the
// workspace, for one prime chain: constants, plan and lane-order map, and the keys and masks on that chain's limbs.  There is one
// for the handle's L limbs (piehip_ctx::cx) and one per level context (below); a Sched carries one, as it carries a queue, and
// run()'s chain is the same schedule on either.
struct ChainCtx {
    const DevConsts *d_dc = nullptr;
    const NttPlan *plan = nullptr;
    const u32 *d_sigma_inv = nullptr;   // lane-order position -> standard position
    u32 N = 0, L = 0, M = 0;
    // EvalMult key [L][2][L][N]; per-query keys (piehip_load_relin_key_q), piehip_ctx::evkq_n of them one after the other, entries nobody
    // loaded holding the handle's key; masks [b][L][N].  *_sigma: the lane-ordered twin, where the plan has a lane order (piehip.cpp,
    // lane_twin).  A handle that borrows its database (piehip_attach_database) has its owner's evk* and masks* here.
    u64 *evk = nullptr, *evk_sigma = nullptr, *evkq = nullptr, *evkq_sigma = nullptr, *masks = nullptr, *masks_sigma = nullptr;
    size_t LN() const { return (size_t)L * N; }
    size_t key_words() const { return (size_t)L * 2 * LN(); }
};

// Chain limbs (include/piehip.h): everything piehip_create derives from (N, Lc, t, q[:Lc], p[:Lc + 1]) -- constant block, transform
// tables, plan with its routes and fusions -- behind a ChainCtx whose keys and masks are the limb prefixes of the handle's, copied
// when the key or the database is set (piehip.cpp, level_sync).  Built when the setting first takes the value Lc and kept with the
// handle; its device tables are freed with the handle's (dev_tables).
static const u32 MAX_CHAIN_SCHED = 7;   // entries of a chain schedule (include/piehip.h)
struct LevelCtx {
    HostParams hp;
    DevConsts *d_dc = nullptr;
    NttPlan plan;
    u32 *d_sigma_inv = nullptr;
    ChainCtx cx;
    size_t evk_cap = 0, evkq_cap = 0, masks_cap = 0;   // words cx.evk / cx.evkq / cx.masks (and each twin) were allocated for
};

}  // namespace piehip
using piehip::u32;
using piehip::u64;

struct piehip_ctx {
    piehip::HostParams hp;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<hipStream_t> side_streams;        // extra queues of run(): one group of bin layers each (see piehip_run)
    std::vector<hipEvent_t> ev_join;
    hipEvent_t ev_fork = nullptr;
    // runs that bring their results down to host memory: queue group g + 1 starts when group g has reached the kernel that writes
    // its results, so that the download of group g runs under the evaluation of group g + 1 (piehip_run_into)
    hipEvent_t ev_chain = nullptr;                // (the event; Sched::release says which group records it)
    u32 run_streams = 0;                          // piehip_set_run_streams: 0 = all queues
    bool inputs_dirty = true;                     // inputs / keys / database changed on the handle's stream since the last run()
    bool pending_join = false;                    // run() left work on the bin-layer queues that the handle's stream has not waited for
    // piehip_set_graph: run() as one captured hipGraph per (inputs, result buffer, queue count), replayed on the handle's stream
    bool use_graph = false;
    hipGraphExec_t gexec = nullptr;
    const void *g_idx = nullptr, *g_minus = nullptr, *g_res = nullptr;
    u32 g_ng = 0;
    // the host-memory path (piehip_host.cpp): query[q] has every query's page-locked staging and which pieces have been staged;
    // all transfers travel on the handle's own queues (no copy stream: see piehip_host.cpp)
    bool stage_open = false;                      // piehip_stage_*: the uploads of the next run()'s queries have begun
    u64 *pin_up_flag = nullptr;                   // page-locked word: sequence number of the last query of this handle whose uploads have
    u64 up_seq = 0;                               // left host memory (written by a one-thread kernel behind them); the next number
    u64 up_turn_wait_ns = 0;                      // how long the last staging sequence waited for its turn on the device's link
    u64 up_turn_wait_total_ns = 0, up_turn_waits = 0;   // ... and all of them so far (piehip_upload_turn_wait)
    // piehip_set_host_path_timing: three events per query on the handle's stream -- first staged piece, uploads handed over, results down
    bool hp_timing = false;
    hipEvent_t hp_ev[3] = {nullptr, nullptr, nullptr};
    int hp_ev_state = 0;                          // 0 nothing recorded, 1 first piece, 2 handed over, 3 complete sequence recorded
    // the one expansion launch of a staging sequence with seeded pieces: its job table goes up from a page-locked table with two
    // halves (sequence s writes half s & 1 once sequence s - 2's copy has left it: piehip_host.cpp) into d_seed_jobs
    piehip::SeedJob *pin_seed_jobs = nullptr;     // [2][seed_jobs_cap]
    piehip::SeedJob *d_seed_jobs = nullptr;       // [seed_jobs_cap]
    size_t seed_jobs_cap = 0;
    u64 *pin_res = nullptr;                       // [b][nq][2][L][N]
    size_t pin_idx_words = 0, pin_res_words = 0;
    piehip::DevConsts *d_dc = nullptr;
    // tables of piehip_create, freed through dev_tables: the transform tables live in `plan`, which also says what the context can
    // do with them (lane order, folding, fusions: DESIGN.md section 5a)
    std::vector<void *> dev_tables;
    u32 *d_inv_pos = nullptr;    // EVALUATION position -> slot
    u32 *d_sigma_inv = nullptr;  // lane-order position -> standard position (identity without a lane order)
    u64 *d_hash_tbl = nullptr;   // [k][e][K][b][E] of the last piehip_build_db
    size_t hash_tbl_words = 0;
    // scratch of the offline phase (hashing, packing, encoding), kept between calls: piehip_reserve sizes it up front so that
    // the timed offline phase allocates nothing (hipMalloc / hipFree cost milliseconds and synchronise the device)
    u64 *arena = nullptr;
    size_t arena_words = 0, arena_used = 0;
    u32 hk = 0, he = 0, hb = 0;  // table dimensions ([k][e][K][hb][E]; hb = all bin layers, of which this handle keeps b)
    // piehip_set_layer_tiling: the next build / table load / reserve packs `tiling` bin layers side by side into one slot vector and
    // keeps ceil(hb / tiling) tiled layers (1 = as ever).  Only those calls read it: the database they leave is an ordinary one
    u32 tiling = 1;
    piehip::NttPlan plan;
    piehip::ChainCtx cx;         // the handle's own context: d_dc, plan, d_sigma_inv above, and the handle's keys and masks
    // piehip_set_chain_schedule (piehip_set_chain_limbs: a schedule of one entry): product hf of run()'s chain, 1-based, works on the
    // level context of the first chain_level(hf) limbs -- the handle's own context at L.  Every level the handle has been set to stays
    // in `levels`
    u32 chain_sched[piehip::MAX_CHAIN_SCHED] = {};   // non-increasing, every entry in [1, L]
    u32 chain_n = 0;
    std::map<u32, std::unique_ptr<piehip::LevelCtx>> levels;
    // keys / database / inputs
    bool db_borrowed = false;  // piehip_attach_database: cx.evk*, d_db, cx.masks* belong to another handle (never freed or written here)
    piehip_ctx *db_owner = nullptr;  // ... that handle
    u32 db_borrowers = 0;            // handles that borrow from this one: its buffers may not move while > 0
    u32 K = 0, b = 0, E = 0;
    u64 *d_db = nullptr;
    // query batch (piehip_set_query_batch): run() evaluates queries 0 .. nq - 1 against the database at once.  Workspace and
    // results hold nq rows per bin layer: [b][nq][..].
    piehip::Query query[piehip::STAGE_A_MAX_QUERIES];
    u32 nq = 1;
    // piehip_load_relin_key_q: the queries of a batch come from different clients, each with its own EvalMult key (cx.evkq)
    u32 evkq_n = 0, evkq_loaded = 0;    // keys the array holds; bit q: query q loaded its own
    // run() workspace
    u64 *d_acc = nullptr;   // [b][K][2][L][N]
    u64 *d_prod = nullptr;  // [b][2][L][N]  (K > 2 only)
    u64 *d_out = nullptr;   // [b][2][L][N]  ([b][3][L][N] once the handle has handed out three-component rows: res_cap_comps)
    // piehip_set_result_limbs: run() hands its results out on the first res_limbs limbs of Q (L = as they are).  With fewer, the
    // product chain writes full rows into d_full and the reduction writes [b][nq][2][res_limbs][N] into the result buffer
    u32 res_limbs = 0;
    u64 *d_full = nullptr;  // [b][nq][2][L][N], allocated with the first setting below L and kept with the workspace
    // piehip_set_result_relin: off, the last product of a run() with K >= 2 is not relinearised and a result row has three components.
    // d_out and d_full then hold res_cap_comps = 3 components per row (allocated with the setting, kept with the workspace), and the
    // workspace has ws.t3
    bool res_relin = true;
    u32 res_cap_comps = 0;
    piehip::MulWs ws;
    size_t ws_cap_rows = 0;   // rows (bin layer x query) the workspace arrays were allocated for; ws.nb = rows in use
    u32 ws_cap_K = 0;
    // sharded server (piehip_rccl.cpp): this handle's rank in an RCCL communicator (ncclComm_t; owned if piehip_rccl_init made it)
    void *comm = nullptr;
    bool comm_owned = false;
    int comm_ranks = 0, comm_rank = 0;
    u64 *d_gather = nullptr, *pin_gather = nullptr;   // the root's gathered result list [b_total][nq][ncomp][rl][N]: HBM, page-locked host
    size_t gather_words = 0;
    // piehip_rccl_agree_rows: the row shape (components, limbs, queries) every rank of the communicator had when they last compared;
    // forgotten (forget_rows) by every call that can change this handle's.  The gather moves rows of another shape than the default
    // [2][L][N] only while the handle's shape is the agreed one
    bool rows_agreed = false;
    u32 rows_ncomp = 0, rows_limbs = 0, rows_nq = 0;
    piehip::SliceState slice;
    // rotation-based PIE (FHEHIPPIE): rotation keys by index, EVALUATION index maps, packed sub-tables
    std::map<int32_t, u64 *> rotkeys;   // [L][2][L][N] each
    std::map<int32_t, u32 *> rotmaps;   // [N] each
    u32 fp_npie = 0, fp_K = 0, fp_b = 0, fp_E = 0;
    u64 *fp_pt = nullptr;     // [npie][K][b][L][N]
    u64 *fp_mask = nullptr;   // [npie][K][L][N]
    u64 *fp_e0 = nullptr;     // [L][N]: plaintext with slot 0 = 1 (EvalMerge's mask)
    u64 *fp_idx = nullptr;    // [npie][K][2][L][N]
    u64 *fp_out = nullptr;    // [npie][K][2][L][N]
    u64 *fp_negkeys = nullptr;  // [b][L][2][L][N]: key of rotation -r at position r (position 0 unused)
    u32 *fp_negmaps = nullptr;  // [b][N]
    // profiling
    bool profiling = false;
    std::vector<piehip::ProfRec> recs;
    std::vector<hipEvent_t> pool;
    size_t pool_used = 0;

    size_t LN() const { return (size_t)hp.L * hp.N; }
    u32 res_comps(u32 K_) const { return (!res_relin && K_ >= 2) ? 3u : 2u; }   // components of a result row for K_ inner hash functions
    u32 res_comps() const { return res_comps(K); }
    u32 chain_level(u32 hf) const { return chain_sched[std::min(hf, chain_n) - 1]; }   // limbs of product hf = 1, 2, ..
    // ... of the last product that runs (K - 1; a handle without products answers as one with a single product would), which are
    // the mask multiply's and the result rows'; and the lowest entry: below L, the handle refuses what a chain on fewer limbs refuses
    u32 chain_last() const { return chain_level(K >= 2 ? K - 1 : 1); }
    u32 chain_floor() const { return chain_sched[chain_n - 1]; }
    const piehip::ChainCtx &level_cx(u32 limbs) const { return limbs >= hp.L ? cx : levels.at(limbs)->cx; }
    // limbs of a result row: the minimum of the two settings (chain limbs change nothing where there is no product: K = 1)
    u32 out_limbs() const { return K >= 2 ? std::min(res_limbs, chain_last()) : res_limbs; }
    size_t res_ct_words() const { return res_comps() * (size_t)out_limbs() * hp.N; }   // one result ciphertext as it leaves the handle
    void forget_rows() { rows_agreed = false; }
};

namespace piehip {

// the key switch of a run() on context cx (the handle's own or one of its levels) has a key for every query: the context's copy of the
// handle's key, or of one key per query of the batch -- read only while the handle's per-query array is the current batch's
// (piehip_set_query_batch frees that one and leaves a level's copy behind)
inline bool run_keys_loaded(const piehip_ctx *h, const ChainCtx &cx)
{
    if (h->K == 2 && !h->res_relin) return true;   // the only product is not relinearised
    return h->K <= 1 || cx.evk || (h->cx.evkq && cx.evkq && h->evkq_n == h->nq && h->evkq_loaded == (1u << h->nq) - 1);
}

// Where and how a schedule piece is enqueued.  A handle alone converts to "its stream, no gate, one mask and one key for every
// row": what every entry point outside run() enqueues with.  run_on_queues makes one per queue group.
struct Sched {
    piehip_ctx *h;
    hipStream_t stream;
    hipEvent_t wait_before_results = nullptr;  // the result buffer may still be read by work queued on the handle's stream before
                                               // this run: the kernel that writes the results waits for this (null: no need)
    hipEvent_t release = nullptr;  // host-results runs: recorded, and cleared, when this group has only its result-writing kernel
                                   // left; the next queue group starts behind it (null: nobody waits)
    u32 mask_div = 1;   // a batch: ciphertext row r of the product chain takes mask r / mask_div
    u32 key_group = 1;  // ... and, with per-query EvalMult keys, key r % key_group of cx->evkq
    bool key_per_query = false;  // the keys are cx->evkq's (a batch of one included: key_group 1 of that array)
    const ChainCtx *cx; // the context the pieces work on: the handle's own unless run() hands them its level context (chain limbs)
    Sched(piehip_ctx *h_) : h(h_), stream(h_->stream), cx(&h_->cx) {}
    Sched(piehip_ctx *h_, hipStream_t s) : h(h_), stream(s), cx(&h_->cx) {}
    void wait_for_readers() const { if (wait_before_results) (void)hipStreamWaitEvent(stream, wait_before_results, 0); }
    void gate()  // in front of the kernel that writes a run's results
    {
        wait_for_readers();
        if (release) (void)hipEventRecord(release, stream);
        release = nullptr;
    }
};

hipEvent_t prof_event(piehip_ctx *h);
// brackets the launches queued in its scope with HIP events on the caller's stream (a handle: its own) when profiling is on
struct ProfScope {
    piehip_ctx *h;
    hipStream_t stream;
    ProfRec r;
    bool on;
    ProfScope(const Sched &s, int k, double bytes) : h(s.h), stream(s.stream), on(s.h->profiling)
    {
        if (!on) return;
        r.k = k;
        r.bytes = bytes;
        r.a = prof_event(h);
        r.b = prof_event(h);
        if (!r.a || !r.b) {
            on = false;
            return;
        }
        (void)hipEventRecord(r.a, stream);
    }
    ~ProfScope()
    {
        if (!on) return;
        (void)hipEventRecord(r.b, stream);
        h->recs.push_back(r);
    }
};

void drop_graph(piehip_ctx *h);
int dev_alloc(u64 **p, size_t words);
void dev_free(u64 **p);

struct Tmp {  // RAII device scratch: carved from the handle's arena while it has room, hipMalloc otherwise
    piehip_ctx *h = nullptr;
    size_t mark = 0;
    std::vector<u64 *> ptrs;
    Tmp() {}
    explicit Tmp(piehip_ctx *h_) : h(h_), mark(h_->arena_used) {}
    ~Tmp()
    {
        for (u64 *p : ptrs) (void)hipFree(p);
        if (h) h->arena_used = mark;
    }
    u64 *get(size_t words)
    {
        if (!words) words = 1;
        const size_t w32 = (words + 31) & ~(size_t)31;  // 256-byte granules
        if (h && h->arena && h->arena_used + w32 <= h->arena_words) {
            u64 *p = h->arena + h->arena_used;
            h->arena_used += w32;
            return p;
        }
        u64 *p = nullptr;
        if (hipMalloc((void **)&p, words * sizeof(u64)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
};
#define TMPGET(var, words)                                          \
    piehip::u64 *var = tmp.get(words);                              \
    if (!var) return piehip::fail(PIEHIP_ENOMEM, "hipMalloc failed (scratch)")

int ws_alloc(piehip_ctx *h, MulWs &w, u32 nb);
void ws_free(MulWs &w);

// ---- schedule pieces (piehip_run.cpp) --------------------------------------------------------------
// Each launches on s.stream; a piece told that it writes a run's results (out_is_result) passes s.gate() in front of that kernel
// sigma: lane order on the EVALUATION side; fold: outer stage applied by the neighbouring kernels.  Callers say what they would
// like; ntt() and enqueue_keyswitch() are where a context without lane order / folding (h->plan) turns that into standard order
void ntt(const Sched &s, u64 *data, u32 nlimbs, u32 mod_base, u32 mod_count, bool inv, bool sigma = false, bool fold = false,
         const NttExtra *ex = nullptr);
// a key-switching key [L][2][L][N]; group > 1: ciphertext row r takes key r % group of an array of keys `stride` words apart
struct RunKey {
    const u64 *key;
    size_t stride;
    u32 group;
    RunKey(const u64 *key_, size_t stride_ = 0, u32 group_ = 1) : key(key_), stride(stride_), group(group_) {}
};
struct KeyswitchOpts {
    bool lane = false;           // w.d01, the digits, key and mask are lane-ordered (and folded) where the context has a lane order
    bool out_is_result = false;  // out (always in standard order) is a run()'s result buffer
    bool digits_ready = false;
    bool d01_eval_q = false;     // (enqueue_mul only, plan.d01_eval_q) w.d01 lacks the own-limb term; the MAC adds it from w.eqp
};
void enqueue_keyswitch(Sched &s, MulWs &w, u32 nb, RunKey key, const u64 *mask, u64 *out, KeyswitchOpts o = {});
// x, y: the operands as launch_expand_pair takes them (kernels.hpp), rows of [2] polynomials each
void enqueue_mul(Sched &s, MulWs &w, const ExpandOperand &x, const ExpandOperand &y, u32 nb, bool relin, const u64 *mask, u64 *out,
                 bool out_is_result = false);
int encode_on_device(piehip_ctx *h, const int64_t *d_slots, u32 npt, u32 B, u64 *d_out);
static const u32 ENCODE_CHUNK = 256;  // plaintexts per batch of the device encoder (bounds its mod-t scratch)
// piehip.cpp: run() workspace (and, with_db, database and masks) of a handle for b bin layers; the lane-ordered copy of its masks; the
// persistent hash-table buffer; a host table [k][e][K][b][E] uploaded into it, shuffled and gathered into slot vectors in the
// caller's scratch (piehip_load_db_table_bins, piehip_load_db_table_sliced).  R > 1 (layer tiling): the slot vectors are the tiled
// ones, [max(K b' E, b')][R k e] with b' = ceil(b / R)
int alloc_run_buffers(piehip_ctx *h, u32 K, u32 b, u32 E, bool with_db = true);
int make_masks_sigma(piehip_ctx *h);
int hash_tbl_alloc(piehip_ctx *h, size_t words);
// (hidden: the library's dynamic symbols stay the ones they were)
__attribute__((visibility("hidden"))) int table_to_slots(piehip_ctx *h, Tmp &tmp, const u64 *tbl, u32 k, u32 e, u32 K, u32 b, u32 E,
                                                          u64 shuffle_seed, int64_t **d_slots, u32 R = 1);
__attribute__((visibility("hidden"))) int items_to_slots(piehip_ctx *h, Tmp &tmp, const u64 *items, size_t n, u32 k, u32 e, u32 K, u32 b, u32 E,
                                                          u64 hash_seed, u64 evict_seed, u64 shuffle_seed, int64_t **d_slots, u32 R = 1);
// piehip_run.cpp: the queues of piehip_run_into / piehip_run_chain_into (host_results, piehip_run_staged: every queue group also
// downloads its slice of the results there); whether stage A hands operand X over in lane order
int run_on_queues(piehip_ctx *h, void *d_results, bool chain_only, u64 *host_results = nullptr);
bool run_x_direct(const piehip_ctx *h);
// the context the LAST product of run()'s chain works on -- the handle's own, or a level's: the mask multiply's, the result rows' and
// the result reduction's
const ChainCtx &run_chain_ctx(const piehip_ctx *h);
bool run_chain_keys_loaded(const piehip_ctx *h);   // every level on which a product of the chain relinearises has its key(s)
// piehip_slice.cpp
void slice_free(piehip_ctx *h);          // back to an unsliced handle: the slice side's buffers and state
int slice_batch_changed(piehip_ctx *h);  // piehip_set_query_batch on a sliced handle: acc for the new batch, nothing put
// result limbs (piehip_run.cpp): `rows` ciphertexts full[rows][2][L][N] (EVALUATION, standard order; overwritten) reduced to their
// first `keep` limbs, out[rows][2][keep][N].  out_is_result: out is a run()'s result buffer
// comps: polynomials per row (3: degree-2 results)
void enqueue_mod_reduce(Sched &s, u64 *full, u32 rows, u32 keep, u64 *out, bool out_is_result = false, u32 comps = 2);
// piehip.cpp: what the handle's result settings need beside the workspace's rows, for a database of K inner hash functions: d_full when
// it reduces its results; three-component d_out / d_full and ws.t3 when it hands out degree-2 results
int ensure_full_rows(piehip_ctx *h, u32 K);
// piehip.cpp: with a chain schedule below L, bring the level contexts' copies of keys and masks up to the handle's (on its stream)
int level_sync(piehip_ctx *h);
// device input buffers of query q of the batch (owned copies: the host setters and the staged uploads write them)
int query_input_buffers(piehip_ctx *h, u32 q, u64 **d_idx, u64 **d_minus);
void use_owned_inputs(piehip_ctx *h);   // the next run() evaluates the owned copies of every query of the batch
void free_host_path(piehip_ctx *h);   // piehip_host.cpp: page-locked staging
// piehip_host.cpp: expand the seeded polynomials of `jobs` on the handle's stream and wait for them (client, keys, tests; the
// staged path queues its expansion without waiting)
int expand_seeded_sync(piehip_ctx *h, const std::vector<SeedJob> &jobs);
SeedJob seed_job(u64 *dst, const uint8_t *seed);
bool stage_has_seeded(const piehip_ctx *h);
// queues of a run() and the bin layers each takes
u32 run_queue_count(const piehip_ctx *h);
int ensure_run_queues(piehip_ctx *h, u32 ng);
u32 run_group_size(u32 b, u32 ng, u32 g);

}  // namespace piehip
