// piehip_slice.cpp -- query slices (include/piehip.h "Query slices"): stage A of BatchedFHEHIPPIE::run() sharded by
// what the QUERY is made of.  Unit u = h L + l is limb l of inner hash function h.  A handle holds a contiguous unit range of the packed
// database for all bin layers and computes those limbs of every accumulator (reference BatchedFHEHIPPIE.cpp:96-116: the slice side);
// the accumulators then travel to the handles that own the bin layers, which run the product chain as ever (.cpp:117-126: the chain
// side, piehip_run.cpp).  A handle needs 1 / (K L) of the query per unit it holds, and no handle needs the whole query.
#include "piehip_ctx.hpp"

using namespace piehip;

namespace piehip {

void slice_free(piehip_ctx *h)
{
    SliceState &s = h->slice;
    if (!s.on && !s.db && !s.acc && !s.ev_ready) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    dev_free(&s.db);
    dev_free(&s.acc);
    for (auto &query : s.in)
        for (SliceInput &in : query) dev_free(&in.own);
    if (s.ev_ready) (void)hipEventDestroy(s.ev_ready);
    if (s.ev_read) (void)hipEventDestroy(s.ev_read);
    if (s.ev_jobs) (void)hipEventDestroy(s.ev_jobs);
    if (s.pin_jobs) (void)hipHostFree(s.pin_jobs);
    if (s.d_jobs) (void)hipFree(s.d_jobs);
    for (u64 *p : s.pin_idx)
        if (p) (void)hipHostFree(p);
    for (u64 *p : s.pin_minus)
        if (p) (void)hipHostFree(p);
    dev_free(&s.scatter_stage);
    dev_free(&s.xchg_stage);
    s = SliceState();
}

static int slice_alloc_acc(piehip_ctx *h)
{
    SliceState &s = h->slice;
    dev_free(&s.acc);
    s.acc_nq = 0;
    const int rc = dev_alloc(&s.acc, (size_t)s.b_total * h->nq * s.u_n() * 2 * h->hp.N);
    if (rc) return rc;
    s.acc_nq = h->nq;
    return PIEHIP_OK;
}

int slice_batch_changed(piehip_ctx *h)
{
    SliceState &s = h->slice;
    if (!s.on) return PIEHIP_OK;
    // caller-owned slice inputs of queries outside the new batch are forgotten, as piehip_set_query_batch forgets the whole ones
    for (u32 q = h->nq; q < STAGE_A_MAX_QUERIES; q++)
        for (SliceInput &in : s.in[q]) in.cur = nullptr, in.seeded = false;
    std::fill(s.put.begin(), s.put.end(), false);
    return slice_alloc_acc(h);
}

}  // namespace piehip

// the handle becomes a query-sliced one of this shape: chain-side workspace for its bin layers (none for an empty range), room for
// its units of the database and of the accumulators.  The masks and the database's contents are the callers' business.
static int slice_setup(piehip_ctx *h, u32 K, u32 b, u32 E, u32 u_lo, u32 u_hi, u32 bin_lo, u32 bin_hi)
{
    const u32 L = h->hp.L;
    if (K < 1 || b < 1 || E < 1) return fail(PIEHIP_EINVAL, "query slice: K, b and E are at least one");
    if (u_lo > u_hi || u_hi > K * L) return fail(PIEHIP_EINVAL, "query slice: the unit range must lie within [0, K L] with u_lo <= u_hi");
    if (bin_lo > bin_hi || bin_hi > b) return fail(PIEHIP_EINVAL, "query slice: the bin-layer range must lie within [0, b] with bin_lo <= bin_hi");
    if ((size_t)(bin_hi - bin_lo) * STAGE_A_MAX_QUERIES * 2 > 65535) return fail(PIEHIP_EINVAL, "query slice: too many bin layers for one placement launch");
    if (h->db_borrowed || h->db_borrowers)
        return fail(PIEHIP_ESTATE, "query slice: the handle lends or borrows a database (piehip_attach_database)");
    if (h->use_graph) return fail(PIEHIP_ESTATE, "query slice: the handle replays a captured graph (piehip_set_graph)");
    if (!h->res_relin) return fail(PIEHIP_ESTATE, "query slice: the handle hands out unrelinearised results (piehip_set_result_relin)");
    if (h->chain_floor() < h->hp.L) return fail(PIEHIP_ESTATE, "query slice: the handle runs its product chain on fewer limbs (piehip_set_chain_limbs)");
    HIPCHK(hipSetDevice(h->device));
    slice_free(h);
    int rc = alloc_run_buffers(h, K, bin_hi - bin_lo, E, false);
    if (rc) return rc;
    if (bin_hi > bin_lo && (rc = dev_alloc(&h->cx.masks, (size_t)(bin_hi - bin_lo) * h->LN()))) return rc;
    SliceState &s = h->slice;
    s.u_lo = u_lo, s.u_hi = u_hi, s.bin_lo = bin_lo, s.bin_hi = bin_hi, s.b_total = b;
    s.put.assign((size_t)K * L, false);
    if ((rc = dev_alloc(&s.db, (size_t)s.u_n() * b * E * h->hp.N))) return rc;
    if ((rc = slice_alloc_acc(h))) return rc;
    HIPCHK(hipEventCreateWithFlags(&s.ev_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.ev_read, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.ev_jobs, hipEventDisableTiming));
    s.on = true;
    return PIEHIP_OK;
}

// MakePackedPlaintext (BatchedFHEHIPPIE.cpp:68) of the gathered slot vectors d_slots[K][b][E][B] for the handle's units only: the
// encoder's own steps (encode_on_device), the mod-t part once per inner hash function and chunk, lift and forward transform for
// the limbs the handle holds of it -- one-limb plaintexts slice.db[u][b][E][N]
static int encode_units(piehip_ctx *h, const int64_t *d_slots, u32 b, u32 E, u32 B)
{
    const u32 N = h->hp.N, L = h->hp.L, M = h->hp.M;
    const SliceState &s = h->slice;
    const u32 npt = b * E, chunk = ENCODE_CHUNK;
    Tmp tmp(h);
    TMPGET(d_u, (size_t)(npt < chunk ? npt : chunk) * N);
    for (u32 u0 = s.u_lo; u0 < s.u_hi;) {
        const u32 hf = u0 / L, u1 = std::min(s.u_hi, (hf + 1) * L);   // the handle's limbs [u0, u1) of inner hash function hf
        for (u32 p = 0; p < npt; p += chunk) {
            const u32 c = npt - p < chunk ? npt - p : chunk;
            ProfScope ps(h, PIEHIP_K_ENCODE, 8.0 * c * ((double)B + 2.0 * N + (double)(u1 - u0) * N));
            launch_encode_scatter(h->d_dc, N, M, d_slots + ((size_t)hf * npt + p) * B, B, h->d_inv_pos, d_u, c, h->stream);
            launch_ntt(h->plan, d_u, c, M, 1, true, h->stream);
            for (u32 u = u0; u < u1; u++) {
                u64 *out = s.db + ((size_t)(u - s.u_lo) * npt + p) * N;
                launch_encode_lift(h->d_dc, N, 1, M, d_u, out, c, h->stream, u % L);
                launch_ntt(h->plan, out, c, u % L, 1, false, h->stream);
            }
        }
        u0 = u1;
    }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(PIEHIP_EHIP, std::string("sliced encode: ") + hipGetErrorString(e));
    return PIEHIP_OK;
}

static int need_sliced(const piehip_ctx *h, const char *who = "")
{
    if (h->slice.on) return PIEHIP_OK;
    return fail(PIEHIP_ESTATE, std::string(who) + "not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
}

static int slice_query_check(piehip_ctx *h, u32 q, const void *p, const char *what)
{
    if (!p) return fail(PIEHIP_EINVAL, std::string("null ") + what);
    if (need_sliced(h)) return PIEHIP_ESTATE;
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    return PIEHIP_OK;
}

// query q's seed tables as the expansion reads them: n seeds from `seeds` to position `at` of [K E + 1][8]
static void keep_seeds(piehip_ctx *h, u32 q, size_t at, const uint8_t *seeds, size_t n)
{
    std::vector<u32> &t = h->slice.seeds[q];
    t.resize(((size_t)h->K * h->E + 1) * 8);
    memcpy(&t[at * 8], seeds, n * 32);   // little-endian host: the bytes are the words
}

// Every host setter of a slice input: piece p of query q from `src` in host memory, already cut or the whole query (slice_geometry.h),
// into the owned device copy, which the next piehip_run_slice then reads.  seeded: src holds the c0 rows only and `seeds` the query's
// seeds of the piece ([K][E][32], [32]); the c1 rows are expanded at piehip_run_slice (queue_slice_expansion).  All refusals come in
// front of the device.  SLICE_WHOLE is one strided copy per unit, not one per ciphertext.
static int set_piece(piehip_ctx *h, u32 q, SlicePiece p, SliceLayout layout, bool seeded, const u64 *src, const uint8_t *seeds, const char *what)
{
    NEED(h);
    if (seeded && !seeds) return fail(PIEHIP_EINVAL, std::string("null seeds of ") + what);
    int rc = slice_query_check(h, q, src, what);
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, E = h->E;
    SliceInput &in = s.in[q][p];
    if (!in.own && (rc = dev_alloc(&in.own, (size_t)s.u_n() * piece_cts(p, E) * 2 * N))) return rc;
    for (u32 c = 0, n = layout == SLICE_WHOLE ? s.u_n() : 1; c < n; c++) {
        const SliceCopy g = slice_copy(p, layout, seeded, N, h->hp.L, E, s.u_lo, s.u_hi, c);
        HIPCHK(hipMemcpy2DAsync(in.own + g.dst_off, g.dst_pitch * sizeof(u64), src + g.src_off, g.src_pitch * sizeof(u64), N * sizeof(u64), g.rows,
                                hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (seeded) keep_seeds(h, q, piece_seed_at(p, 0, 0, h->hp.L, h->K, E), seeds, p == SLICE_INDEX ? (size_t)h->K * E : 1);
    in.cur = in.own, in.seeded = seeded;
    return PIEHIP_OK;
}

// ... and the two that take the caller's device array
static int set_piece_device(piehip_ctx *h, u32 q, SlicePiece p, const void *d_src, const char *what)
{
    NEED(h);
    const int rc = slice_query_check(h, q, d_src, what);
    if (rc) return rc;
    h->slice.in[q][p].cur = (const u64 *)d_src, h->slice.in[q][p].seeded = false;
    return PIEHIP_OK;
}

// One expansion launch for every piece of the batch that was set seeded since the last piehip_run_slice, on the handle's stream in
// front of stage A: the c1 row of limb u % L behind each c0 row of the handle's units.
// The job table.  The page-locked table is read by ONE copy, queued here; ev_jobs is recorded behind that copy, and the next call
// that has jobs waits for ev_jobs before it writes the table -- so the table is never rewritten while an earlier run's copy of it
// can still be in flight.  The device table is written by that copy alone, on the handle's stream, behind the earlier run's
// expansion launch that read it (stream order).  Both tables hold every piece of the batch and are reallocated (a new batch size)
// only once the stream has drained.
static int queue_slice_expansion(piehip_ctx *h)
{
    SliceState &s = h->slice;
    const u32 N = h->hp.N, L = h->hp.L, E = h->E, un = s.u_n();
    size_t n = 0;
    for (u32 q = 0; q < h->nq; q++)
        for (int p = 0; p < SLICE_PIECES; p++) n += s.in[q][p].seeded ? (size_t)un * piece_cts(p, E) : 0;
    if (!n) return PIEHIP_OK;
    if (n > s.jobs_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (s.pin_jobs) (void)hipHostFree(s.pin_jobs);
        if (s.d_jobs) (void)hipFree(s.d_jobs);
        s.pin_jobs = s.d_jobs = nullptr;
        s.jobs_cap = 0, s.jobs_copied = false;
        const size_t cap = (size_t)h->nq * un * (E + 1);   // every piece of the batch
        HIPCHK(hipHostMalloc((void **)&s.pin_jobs, cap * sizeof(SeedLimbJob), hipHostMallocPortable));
        HIPCHK(hipMalloc((void **)&s.d_jobs, cap * sizeof(SeedLimbJob)));
        s.jobs_cap = cap;
    }
    if (s.jobs_copied) HIPCHK(hipEventSynchronize(s.ev_jobs));
    size_t at = 0;
    for (u32 q = 0; q < h->nq; q++) {
        const u32 *seeds = s.seeds[q].data();
        for (int p = 0; p < SLICE_PIECES; p++)   // the index piece's units and ciphertexts, then the minus piece's units
            for (u32 u = s.u_lo; u < s.u_hi && s.in[q][p].seeded; u++)
                for (u32 j = 0, cts = piece_cts(p, E); j < cts; j++) {
                    SeedLimbJob &job = s.pin_jobs[at++];
                    job.dst = s.in[q][p].own + (((size_t)(u - s.u_lo) * cts + j) * 2 + 1) * N;
                    memcpy(job.seed, seeds + piece_seed_at(p, u, j, L, h->K, E) * 8, 32);
                    job.limb = u % L;
                }
    }
    HIPCHK(hipMemcpyAsync(s.d_jobs, s.pin_jobs, n * sizeof(SeedLimbJob), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(s.ev_jobs, h->stream));
    s.jobs_copied = true;
    launch_expand_uniform_limb(h->d_dc, N, s.d_jobs, (u32)n, h->stream);
    HIPCHK(hipGetLastError());
    for (u32 q = 0; q < h->nq; q++)
        for (SliceInput &in : s.in[q]) in.seeded = false;
    return PIEHIP_OK;
}

// the rows of the handle's bin layers of src[b_total][nq][un][2][N] (units from u_lo) into the chain side, on the handle's stream
static int place_units(piehip_ctx *h, u32 u_lo, u32 u_hi, const u64 *d_src)
{
    SliceState &s = h->slice;
    for (u32 u = u_lo; u < u_hi; u++)
        if (s.put[u]) return fail(PIEHIP_ESTATE, "put_accumulators: a unit of this range has been put since the last piehip_run_chain");
    if (s.bin_hi > s.bin_lo && u_hi > u_lo) {
        if (!h->d_acc || !h->ws.eqp) return fail(PIEHIP_ESTATE, "put_accumulators: no workspace (an earlier allocation failed)");
        HIPCHK(hipSetDevice(h->device));
        StageAXOut xo;
        const bool x_direct = run_x_direct(h);
        if (x_direct) xo.out = h->ws.eqp, xo.M = h->hp.M, xo.logns = h->plan.lane_logn;
        ProfScope ps(h, PIEHIP_K_OTHER, 16.0 * h->hp.N * (double)(s.bin_hi - s.bin_lo) * h->nq * (u_hi - u_lo) * 2);
        launch_place_accumulators(h->hp.N, h->hp.L, h->K, u_lo, u_hi - u_lo, s.bin_lo, s.bin_hi - s.bin_lo, h->nq, d_src, h->d_acc,
                                  x_direct ? &xo : nullptr, h->stream);
        HIPCHK(hipGetLastError());
    }
    for (u32 u = u_lo; u < u_hi; u++) s.put[u] = true;
    return PIEHIP_OK;
}

// =================================================================================================
extern "C" {

int piehip_query_slice(uint32_t K, uint32_t L, int nranks, int rank, uint32_t *u_lo, uint32_t *u_hi)
{
    if (!u_lo || !u_hi || nranks < 1 || rank < 0 || rank >= nranks) return fail(PIEHIP_EINVAL, "query_slice: bad rank or null out");
    plan_range(K * L, nranks, rank, u_lo, u_hi);
    return PIEHIP_OK;
}

int piehip_load_db_table_sliced(piehip_handle h, const uint64_t *tbl, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                                uint64_t shuffle_seed, uint64_t mask_seed, uint32_t u_lo, uint32_t u_hi, uint32_t bin_lo, uint32_t bin_hi)
{
    NEED(h);
    if (!tbl || k < 1 || e < 1) return fail(PIEHIP_EINVAL, "bad hash table");
    if (K < 2) return fail(PIEHIP_EINVAL, "Cuckoo Table needs more than one hash function!");  // CuckooHashTable.cpp:39-42
    const size_t B = (size_t)k * e;
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size k*e exceeds the ring dimension");
    if (h->tiling > 1) return fail(PIEHIP_ESTATE, "query slice: not with a layer tiling (piehip_set_layer_tiling above 1)");
    int rc = slice_setup(h, K, b, E, u_lo, u_hi, bin_lo, bin_hi);
    if (rc) return rc;
    Tmp tmp(h);
    int64_t *d_slots = nullptr;
    if ((rc = table_to_slots(h, tmp, tbl, k, e, K, b, E, shuffle_seed, &d_slots))) return rc;
    if ((rc = encode_units(h, d_slots, b, E, (u32)B))) return rc;
    if (bin_hi == bin_lo) return PIEHIP_OK;
    // the masks of the chain side's layers: drawn per layer from mask_seed, the ones the unsharded call draws (encode_bin_layers)
    launch_mask_slots(h->hp.t, b, (u32)B, mask_seed, d_slots, h->stream);
    if ((rc = encode_on_device(h, d_slots + (size_t)bin_lo * B, bin_hi - bin_lo, (u32)B, h->cx.masks))) return rc;
    return make_masks_sigma(h);
}

int piehip_build_db_sliced(piehip_handle h, const uint64_t *items, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                           uint64_t hash_seed, uint64_t evict_seed, uint64_t shuffle_seed, uint64_t mask_seed, uint32_t u_lo, uint32_t u_hi,
                           uint32_t bin_lo, uint32_t bin_hi)
{
    NEED(h);
    if (!items || !n || n > 0x7FFFFFFFu) return fail(PIEHIP_EINVAL, "empty or oversized server set");
    if (k < 1 || e < 1) return fail(PIEHIP_EINVAL, "need at least one outer hash function and position");
    if (K < 2) return fail(PIEHIP_EINVAL, "Cuckoo Table needs more than one hash function!");  // CuckooHashTable.cpp:39-42
    const size_t B = (size_t)k * e;
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size k*e exceeds the ring dimension");
    if (h->tiling > 1) return fail(PIEHIP_ESTATE, "query slice: not with a layer tiling (piehip_set_layer_tiling above 1)");
    int rc = slice_setup(h, K, b, E, u_lo, u_hi, bin_lo, bin_hi);
    if (rc) return rc;
    // the table is hashed, shuffled and gathered where it stays: in HBM (piehip_build_db_bins' steps), then encoded as
    // piehip_load_db_table_sliced encodes the one it was handed
    Tmp tmp(h);
    int64_t *d_slots = nullptr;
    if ((rc = items_to_slots(h, tmp, items, n, k, e, K, b, E, hash_seed, evict_seed, shuffle_seed, &d_slots))) return rc;
    if ((rc = encode_units(h, d_slots, b, E, (u32)B))) return rc;
    if (bin_hi == bin_lo) return PIEHIP_OK;
    launch_mask_slots(h->hp.t, b, (u32)B, mask_seed, d_slots, h->stream);
    if ((rc = encode_on_device(h, d_slots + (size_t)bin_lo * B, bin_hi - bin_lo, (u32)B, h->cx.masks))) return rc;
    return make_masks_sigma(h);
}

int piehip_slice_host_buffers_q(piehip_handle h, uint32_t q, uint64_t **idx, uint64_t **minus)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (need_sliced(h, "slice_host_buffers: ")) return PIEHIP_ESTATE;
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    SliceState &s = h->slice;
    HIPCHK(hipSetDevice(h->device));
    const size_t ct = 2 * h->LN();
    if (idx && !s.pin_idx[q]) HIPCHK(hipHostMalloc((void **)&s.pin_idx[q], (size_t)h->K * h->E * ct * sizeof(u64), hipHostMallocPortable));
    if (minus && !s.pin_minus[q]) HIPCHK(hipHostMalloc((void **)&s.pin_minus[q], ct * sizeof(u64), hipHostMallocPortable));
    if (idx) *idx = s.pin_idx[q];
    if (minus) *minus = s.pin_minus[q];
    return PIEHIP_OK;
}

int piehip_load_db_sliced(piehip_handle h, uint32_t K, uint32_t b, uint32_t E, uint32_t u_lo, uint32_t u_hi, const uint64_t *pts_slice,
                          uint32_t bin_lo, uint32_t bin_hi, const uint64_t *masks)
{
    NEED(h);
    if ((!pts_slice && u_hi > u_lo) || (!masks && bin_hi > bin_lo)) return fail(PIEHIP_EINVAL, "null database");
    int rc = slice_setup(h, K, b, E, u_lo, u_hi, bin_lo, bin_hi);
    if (rc) return rc;
    const SliceState &s = h->slice;
    if (s.u_n())
        HIPCHK(hipMemcpyAsync(s.db, pts_slice, sizeof(u64) * (size_t)s.u_n() * b * E * h->hp.N, hipMemcpyHostToDevice, h->stream));
    if (bin_hi > bin_lo)
        HIPCHK(hipMemcpyAsync(h->cx.masks, masks, sizeof(u64) * (size_t)(bin_hi - bin_lo) * h->LN(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return bin_hi > bin_lo ? make_masks_sigma(h) : PIEHIP_OK;
}

int piehip_get_query_slice(piehip_handle h, uint32_t *u_lo, uint32_t *u_hi, uint32_t *bin_lo, uint32_t *bin_hi)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (need_sliced(h)) return PIEHIP_ESTATE;
    if (u_lo) *u_lo = h->slice.u_lo;
    if (u_hi) *u_hi = h->slice.u_hi;
    if (bin_lo) *bin_lo = h->slice.bin_lo;
    if (bin_hi) *bin_hi = h->slice.bin_hi;
    return PIEHIP_OK;
}

// ---- slice inputs: set_piece, set_piece_device ------------------------------------------------------------------------------------
int piehip_set_index_slice_q(piehip_handle h, uint32_t q, const uint64_t *idx_slice)
{
    return set_piece(h, q, SLICE_INDEX, SLICE_CUT, false, idx_slice, nullptr, "index slice");
}
int piehip_set_minus_slice_q(piehip_handle h, uint32_t q, const uint64_t *minus_slice)
{
    return set_piece(h, q, SLICE_MINUS, SLICE_CUT, false, minus_slice, nullptr, "minus slice");
}
int piehip_set_index_slice_from_q(piehip_handle h, uint32_t q, const uint64_t *idx)
{
    return set_piece(h, q, SLICE_INDEX, SLICE_WHOLE, false, idx, nullptr, "index matrix");
}
int piehip_set_minus_slice_from_q(piehip_handle h, uint32_t q, const uint64_t *minus)
{
    return set_piece(h, q, SLICE_MINUS, SLICE_WHOLE, false, minus, nullptr, "minus element");
}
int piehip_set_index_slice_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0_slice, const uint8_t *seeds)
{
    return set_piece(h, q, SLICE_INDEX, SLICE_CUT, true, c0_slice, seeds, "seeded index slice");
}
int piehip_set_minus_slice_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0_slice, const uint8_t *seed)
{
    return set_piece(h, q, SLICE_MINUS, SLICE_CUT, true, c0_slice, seed, "seeded minus slice");
}
int piehip_set_index_slice_seeded_from_q(piehip_handle h, uint32_t q, const uint64_t *c0idx, const uint8_t *seeds)
{
    return set_piece(h, q, SLICE_INDEX, SLICE_WHOLE, true, c0idx, seeds, "seeded index matrix");
}
int piehip_set_minus_slice_seeded_from_q(piehip_handle h, uint32_t q, const uint64_t *c0minus, const uint8_t *seed)
{
    return set_piece(h, q, SLICE_MINUS, SLICE_WHOLE, true, c0minus, seed, "seeded minus element");
}
int piehip_set_index_slice_device_q(piehip_handle h, uint32_t q, const void *d_idx_slice)
{
    return set_piece_device(h, q, SLICE_INDEX, d_idx_slice, "index slice");
}
int piehip_set_minus_slice_device_q(piehip_handle h, uint32_t q, const void *d_minus_slice)
{
    return set_piece_device(h, q, SLICE_MINUS, d_minus_slice, "minus slice");
}

// ---- the slice side -------------------------------------------------------------------------------------------------------
int piehip_run_slice(piehip_handle h)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    SliceState &s = h->slice;
    if (need_sliced(h, "run_slice: ")) return PIEHIP_ESTATE;
    if (!s.u_n()) return PIEHIP_OK;   // a handle without units: nothing to compute
    if (!s.db || !s.acc || s.acc_nq != h->nq) return fail(PIEHIP_ESTATE, "run_slice: no slice buffers (an earlier allocation failed)");
    StageAQueries qs = {};
    for (u32 q = 0; q < h->nq; q++) {
        for (const SliceInput &in : s.in[q])
            if (!in.cur) return fail(PIEHIP_ESTATE, "run_slice: a query of the batch has no index slice or minus slice");
        qs.idx[q] = s.in[q][SLICE_INDEX].cur, qs.minus[q] = s.in[q][SLICE_MINUS].cur;
    }
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N;
    const int rc = queue_slice_expansion(h);   // the c1 rows of the pieces set seeded since the last run
    if (rc) return rc;
    {
        ProfScope ps(h, PIEHIP_K_STAGE_A, 8.0 * N * s.u_n() * ((double)s.b_total * h->E + h->nq * (2.0 * h->E + 2.0 + 2.0 * s.b_total)));
        launch_stage_a_slice(h->d_dc, N, h->hp.L, s.u_lo, s.u_n(), s.b_total, h->E, qs, h->nq, s.db, s.acc, h->stream, h->plan.small_moduli);
    }
    HIPCHK(hipGetLastError());
    return PIEHIP_OK;
}

int piehip_slice_accumulators_device(piehip_handle h, void **d_acc_slice)
{
    if (!h || !d_acc_slice) return fail(PIEHIP_EINVAL, "null handle or out");
    if (need_sliced(h)) return PIEHIP_ESTATE;
    *d_acc_slice = h->slice.acc;
    return PIEHIP_OK;
}

int piehip_get_slice_accumulators(piehip_handle h, uint64_t *out)
{
    if (!h || !out) return fail(PIEHIP_EINVAL, "null handle or out");
    const SliceState &s = h->slice;
    if (need_sliced(h)) return PIEHIP_ESTATE;
    HIPCHK(hipSetDevice(h->device));
    const size_t words = (size_t)s.b_total * h->nq * s.u_n() * 2 * h->hp.N;
    if (words) HIPCHK(hipMemcpyAsync(out, s.acc, words * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PIEHIP_OK;
}

// ---- the way to the chain side ----------------------------------------------------------------------------------------------
int piehip_put_accumulators(piehip_handle h, uint32_t u_lo, uint32_t u_hi, const void *d_src)
{
    NEED(h);
    if (!h->slice.on) return fail(PIEHIP_ESTATE, "put_accumulators: not a query-sliced handle");
    if (u_lo > u_hi || u_hi > h->K * h->hp.L) return fail(PIEHIP_EINVAL, "put_accumulators: the unit range must lie within [0, K L] with u_lo <= u_hi");
    if (!d_src && u_hi > u_lo) return fail(PIEHIP_EINVAL, "put_accumulators: null source");
    return place_units(h, u_lo, u_hi, (const u64 *)d_src);
}

int piehip_put_accumulators_from(piehip_handle h, piehip_handle src)
{
    NEED(h);
    if (!src) return fail(PIEHIP_EINVAL, "put_accumulators_from: null source handle");
    SliceState &s = h->slice, &f = src->slice;
    if (!s.on || !f.on) return fail(PIEHIP_ESTATE, "put_accumulators_from: both handles must be query-sliced");
    if (src->hp.N != h->hp.N || src->hp.L != h->hp.L || src->hp.moduli != h->hp.moduli || src->K != h->K || f.b_total != s.b_total ||
        src->nq != h->nq)
        return fail(PIEHIP_EINVAL, "put_accumulators_from: the handles differ in parameters, database shape or batch size");
    if (!f.u_n()) return PIEHIP_OK;
    if (!f.acc || f.acc_nq != src->nq) return fail(PIEHIP_ESTATE, "put_accumulators_from: the source has no accumulator buffer");
    const bool work = s.bin_hi > s.bin_lo, cross = work && src->stream != h->stream;
    if (cross) {   // the source's stage A (piehip_run_slice, on its stream) before this handle's placement
        HIPCHK(hipSetDevice(src->device));
        HIPCHK(hipEventRecord(f.ev_ready, src->stream));
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamWaitEvent(h->stream, f.ev_ready, 0));
    }
    const int rc = place_units(h, f.u_lo, f.u_hi, f.acc);
    if (rc) return rc;
    if (cross) {   // ... and the placement before whatever the source queues next (its next piehip_run_slice overwrites the buffer)
        HIPCHK(hipEventRecord(s.ev_read, h->stream));
        HIPCHK(hipSetDevice(src->device));
        HIPCHK(hipStreamWaitEvent(src->stream, s.ev_read, 0));
        HIPCHK(hipSetDevice(h->device));
    }
    return PIEHIP_OK;
}

// ---- the chain side -------------------------------------------------------------------------------------------------------
int piehip_run_chain_into(piehip_handle h, void *d_results)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    SliceState &s = h->slice;
    if (need_sliced(h, "run_chain: ")) return PIEHIP_ESTATE;
    for (size_t u = 0; u < s.put.size(); u++)
        if (!s.put[u]) return fail(PIEHIP_ESTATE, "run_chain: not every unit of the accumulators has been put (piehip_put_accumulators) since the last run_chain");
    if (s.bin_hi > s.bin_lo) {
        const int rc = run_on_queues(h, d_results, true);
        if (rc) return rc;
    }
    std::fill(s.put.begin(), s.put.end(), false);
    return PIEHIP_OK;
}

int piehip_run_chain(piehip_handle h)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (h->slice.on && h->slice.bin_hi == h->slice.bin_lo) return piehip_run_chain_into(h, nullptr);
    if (h->slice.on && !h->d_out) return fail(PIEHIP_ESTATE, "run_chain: no result buffer (an earlier allocation failed)");
    return piehip_run_chain_into(h, h->d_out);
}

}  // extern C
