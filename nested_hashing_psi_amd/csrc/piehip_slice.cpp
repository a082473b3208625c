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
    for (u32 q = 0; q < STAGE_A_MAX_QUERIES; q++) dev_free(&s.idx_own[q]), dev_free(&s.minus_own[q]);
    if (s.ev_ready) (void)hipEventDestroy(s.ev_ready);
    if (s.ev_read) (void)hipEventDestroy(s.ev_read);
    if (s.ev_jobs) (void)hipEventDestroy(s.ev_jobs);
    if (s.pin_jobs) (void)hipHostFree(s.pin_jobs);
    if (s.d_jobs) (void)hipFree(s.d_jobs);
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
    for (u32 q = h->nq; q < STAGE_A_MAX_QUERIES; q++) s.idx[q] = s.minus[q] = nullptr, s.idx_seeded[q] = s.minus_seeded[q] = false;
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
    HIPCHK(hipSetDevice(h->device));
    slice_free(h);
    int rc = alloc_run_buffers(h, K, bin_hi - bin_lo, E, false);
    if (rc) return rc;
    if (bin_hi > bin_lo && (rc = dev_alloc(&h->d_masks, (size_t)(bin_hi - bin_lo) * h->LN()))) return rc;
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

static int slice_query_check(piehip_ctx *h, u32 q, const void *p, const char *what)
{
    if (!p) return fail(PIEHIP_EINVAL, std::string("null ") + what);
    if (!h->slice.on) return fail(PIEHIP_ESTATE, "not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
    if (q >= h->nq) return fail(PIEHIP_EINVAL, "query index outside the batch (piehip_set_query_batch)");
    return PIEHIP_OK;
}

// `rows` rows of N words each, `pitch` words apart in host memory, to the owned device copy of a slice input at word offset dst_off,
// dpitch words apart there (0: one behind the other; 2 N: the c0 rows of ciphertexts that follow each other)
static int upload_rows(piehip_ctx *h, u64 **own, size_t own_words, size_t dst_off, const u64 *src, size_t pitch, u32 rows, size_t dpitch = 0)
{
    int rc;
    if (!*own && (rc = dev_alloc(own, own_words))) return rc;
    const size_t w = (size_t)h->hp.N * sizeof(u64);
    HIPCHK(hipMemcpy2DAsync(*own + dst_off, dpitch ? dpitch * sizeof(u64) : w, src, pitch * sizeof(u64), w, rows, hipMemcpyHostToDevice, h->stream));
    return PIEHIP_OK;
}

// the refusals of a seeded setter, all in front of the device: null input, unsliced handle, query outside the batch
static int slice_seeded_check(piehip_ctx *h, u32 q, const void *c0, const void *seeds, const char *what)
{
    if (!seeds) return fail(PIEHIP_EINVAL, std::string("null seeds of ") + what);
    return slice_query_check(h, q, c0, what);
}

// query q's seed tables as the expansion reads them: n seeds from `seeds` to position `at` of [K E + 1][8]
static void keep_seeds(piehip_ctx *h, u32 q, size_t at, const uint8_t *seeds, size_t n)
{
    std::vector<u32> &t = h->slice.seeds[q];
    t.resize(((size_t)h->K * h->E + 1) * 8);
    memcpy(&t[at * 8], seeds, n * 32);   // little-endian host: the bytes are the words
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
    for (u32 q = 0; q < h->nq; q++) n += (size_t)un * ((s.idx_seeded[q] ? E : 0) + (s.minus_seeded[q] ? 1 : 0));
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
        for (u32 u = s.u_lo; u < s.u_hi && s.idx_seeded[q]; u++)
            for (u32 j = 0; j < E; j++) {
                SeedLimbJob &job = s.pin_jobs[at++];
                job.dst = s.idx_own[q] + (((size_t)(u - s.u_lo) * E + j) * 2 + 1) * N;
                memcpy(job.seed, seeds + ((size_t)(u / L) * E + j) * 8, 32);
                job.limb = u % L;
            }
        for (u32 u = s.u_lo; u < s.u_hi && s.minus_seeded[q]; u++) {
            SeedLimbJob &job = s.pin_jobs[at++];
            job.dst = s.minus_own[q] + ((size_t)(u - s.u_lo) * 2 + 1) * N;
            memcpy(job.seed, seeds + (size_t)h->K * E * 8, 32);
            job.limb = u % L;
        }
    }
    HIPCHK(hipMemcpyAsync(s.d_jobs, s.pin_jobs, n * sizeof(SeedLimbJob), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(s.ev_jobs, h->stream));
    s.jobs_copied = true;
    launch_expand_uniform_limb(h->d_dc, N, s.d_jobs, (u32)n, h->stream);
    HIPCHK(hipGetLastError());
    for (u32 q = 0; q < h->nq; q++) s.idx_seeded[q] = s.minus_seeded[q] = false;
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
    const uint64_t units = (uint64_t)K * L;
    *u_lo = (uint32_t)(units * (uint64_t)rank / (uint64_t)nranks);
    *u_hi = (uint32_t)(units * ((uint64_t)rank + 1) / (uint64_t)nranks);
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
    int rc = slice_setup(h, K, b, E, u_lo, u_hi, bin_lo, bin_hi);
    if (rc) return rc;
    const size_t tbl_words = B * K * b * E;
    if ((rc = hash_tbl_alloc(h, tbl_words))) return rc;
    h->hk = k, h->he = e, h->hb = b;
    Tmp tmp(h);
    const size_t npt = (size_t)K * b * E;
    TMPGET(d_slotsw, (npt > b ? npt : b) * B);
    TMPGET(d_failw, 1);
    int64_t *d_slots = (int64_t *)d_slotsw;
    u32 *d_fail = (u32 *)d_failw;
    // the table is shuffled and gathered whole, as piehip_load_db_table does: every handle given the same seeds holds units of one
    // and the same database
    HIPCHK(hipMemcpyAsync(h->d_hash_tbl, tbl, tbl_words * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(d_fail, 0, sizeof(u32), h->stream));
    launch_shuffle_rows(h->d_hash_tbl, (u32)(B * K), b, E, shuffle_seed, h->stream);
    launch_gather_slots(h->d_hash_tbl, (u32)B, K, b, E, h->hp.t, d_slots, d_fail, h->stream);
    HIPCHK(hipGetLastError());
    u32 failed = 0;
    HIPCHK(hipMemcpyAsync(&failed, d_fail, sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (failed & 2u) return fail(PIEHIP_EINVAL, "server item does not fit the plaintext modulus");
    if ((rc = encode_units(h, d_slots, b, E, (u32)B))) return rc;
    if (bin_hi == bin_lo) return PIEHIP_OK;
    // the masks of the chain side's layers: drawn per layer from mask_seed, the ones the unsharded call draws (encode_bin_layers)
    launch_mask_slots(h->hp.t, b, (u32)B, mask_seed, d_slots, h->stream);
    if ((rc = encode_on_device(h, d_slots + (size_t)bin_lo * B, bin_hi - bin_lo, (u32)B, h->d_masks))) return rc;
    return make_masks_sigma(h);
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
        HIPCHK(hipMemcpyAsync(h->d_masks, masks, sizeof(u64) * (size_t)(bin_hi - bin_lo) * h->LN(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return bin_hi > bin_lo ? make_masks_sigma(h) : PIEHIP_OK;
}

int piehip_get_query_slice(piehip_handle h, uint32_t *u_lo, uint32_t *u_hi, uint32_t *bin_lo, uint32_t *bin_hi)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!h->slice.on) return fail(PIEHIP_ESTATE, "not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
    if (u_lo) *u_lo = h->slice.u_lo;
    if (u_hi) *u_hi = h->slice.u_hi;
    if (bin_lo) *bin_lo = h->slice.bin_lo;
    if (bin_hi) *bin_hi = h->slice.bin_hi;
    return PIEHIP_OK;
}

// ---- slice inputs ---------------------------------------------------------------------------------------------------------
int piehip_set_index_slice_q(piehip_handle h, uint32_t q, const uint64_t *idx_slice)
{
    NEED(h);
    int rc = slice_query_check(h, q, idx_slice, "index slice");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t words = (size_t)s.u_n() * h->E * 2 * h->hp.N;
    if ((rc = upload_rows(h, &s.idx_own[q], words, 0, idx_slice, h->hp.N, s.u_n() * h->E * 2))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    s.idx[q] = s.idx_own[q], s.idx_seeded[q] = false;
    return PIEHIP_OK;
}
int piehip_set_minus_slice_q(piehip_handle h, uint32_t q, const uint64_t *minus_slice)
{
    NEED(h);
    int rc = slice_query_check(h, q, minus_slice, "minus slice");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = upload_rows(h, &s.minus_own[q], (size_t)s.u_n() * 2 * h->hp.N, 0, minus_slice, h->hp.N, s.u_n() * 2))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    s.minus[q] = s.minus_own[q], s.minus_seeded[q] = false;
    return PIEHIP_OK;
}
int piehip_set_index_slice_from_q(piehip_handle h, uint32_t q, const uint64_t *idx)
{
    NEED(h);
    int rc = slice_query_check(h, q, idx, "index matrix");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L, E = h->E;
    const size_t words = (size_t)s.u_n() * E * 2 * N;
    // one strided copy per unit: limb l of the E ciphertexts of inner hash function hf, 2 E rows of N words that lie L N apart
    for (u32 u = s.u_lo; u < s.u_hi; u++) {
        const u64 *src = idx + ((size_t)(u / L) * E * 2 * L + u % L) * N;
        if ((rc = upload_rows(h, &s.idx_own[q], words, (size_t)(u - s.u_lo) * E * 2 * N, src, (size_t)L * N, E * 2))) return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    s.idx[q] = s.idx_own[q], s.idx_seeded[q] = false;
    return PIEHIP_OK;
}
int piehip_set_minus_slice_from_q(piehip_handle h, uint32_t q, const uint64_t *minus)
{
    NEED(h);
    int rc = slice_query_check(h, q, minus, "minus element");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L;
    for (u32 u = s.u_lo; u < s.u_hi; u++)
        if ((rc = upload_rows(h, &s.minus_own[q], (size_t)s.u_n() * 2 * N, (size_t)(u - s.u_lo) * 2 * N, minus + (size_t)(u % L) * N, (size_t)L * N, 2)))
            return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    s.minus[q] = s.minus_own[q], s.minus_seeded[q] = false;
    return PIEHIP_OK;
}
// ---- seeded slice inputs: the c0 rows go up, the c1 rows are expanded at piehip_run_slice (queue_slice_expansion) -----------------
int piehip_set_index_slice_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0_slice, const uint8_t *seeds)
{
    NEED(h);
    int rc = slice_seeded_check(h, q, c0_slice, seeds, "seeded index slice");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N;
    // c0_slice[u_n][E][N] into the c0 rows of idx_own[u_n][E][2][N]: one copy, rows 2 N apart on the device
    if ((rc = upload_rows(h, &s.idx_own[q], (size_t)s.u_n() * h->E * 2 * N, 0, c0_slice, N, s.u_n() * h->E, 2 * (size_t)N))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    keep_seeds(h, q, 0, seeds, (size_t)h->K * h->E);
    s.idx[q] = s.idx_own[q], s.idx_seeded[q] = true;
    return PIEHIP_OK;
}
int piehip_set_minus_slice_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0_slice, const uint8_t *seed)
{
    NEED(h);
    int rc = slice_seeded_check(h, q, c0_slice, seed, "seeded minus slice");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N;
    if ((rc = upload_rows(h, &s.minus_own[q], (size_t)s.u_n() * 2 * N, 0, c0_slice, N, s.u_n(), 2 * (size_t)N))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    keep_seeds(h, q, (size_t)h->K * h->E, seed, 1);
    s.minus[q] = s.minus_own[q], s.minus_seeded[q] = true;
    return PIEHIP_OK;
}
int piehip_set_index_slice_seeded_from_q(piehip_handle h, uint32_t q, const uint64_t *c0idx, const uint8_t *seeds)
{
    NEED(h);
    int rc = slice_seeded_check(h, q, c0idx, seeds, "seeded index matrix");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L, E = h->E;
    const size_t words = (size_t)s.u_n() * E * 2 * N;
    // one strided copy per unit (not one per ciphertext: DESIGN.md section 4b): limb l of the c0 halves of the E ciphertexts of inner
    // hash function hf, E rows of N words that lie L N apart in c0idx[K][E][L][N] and 2 N apart in the slice
    for (u32 u = s.u_lo; u < s.u_hi; u++) {
        const u64 *src = c0idx + ((size_t)(u / L) * E * L + u % L) * N;
        if ((rc = upload_rows(h, &s.idx_own[q], words, (size_t)(u - s.u_lo) * E * 2 * N, src, (size_t)L * N, E, 2 * (size_t)N))) return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    keep_seeds(h, q, 0, seeds, (size_t)h->K * E);
    s.idx[q] = s.idx_own[q], s.idx_seeded[q] = true;
    return PIEHIP_OK;
}
int piehip_set_minus_slice_seeded_from_q(piehip_handle h, uint32_t q, const uint64_t *c0minus, const uint8_t *seed)
{
    NEED(h);
    int rc = slice_seeded_check(h, q, c0minus, seed, "seeded minus element");
    if (rc) return rc;
    SliceState &s = h->slice;
    if (!s.u_n()) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L;
    for (u32 u = s.u_lo; u < s.u_hi; u++)   // the unit's limb of c0minus[L][N]: one row
        if ((rc = upload_rows(h, &s.minus_own[q], (size_t)s.u_n() * 2 * N, (size_t)(u - s.u_lo) * 2 * N, c0minus + (size_t)(u % L) * N, N, 1))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    keep_seeds(h, q, (size_t)h->K * h->E, seed, 1);
    s.minus[q] = s.minus_own[q], s.minus_seeded[q] = true;
    return PIEHIP_OK;
}
int piehip_set_index_slice_device_q(piehip_handle h, uint32_t q, const void *d_idx_slice)
{
    NEED(h);
    int rc = slice_query_check(h, q, d_idx_slice, "index slice");
    if (rc) return rc;
    h->slice.idx[q] = (const u64 *)d_idx_slice, h->slice.idx_seeded[q] = false;
    return PIEHIP_OK;
}
int piehip_set_minus_slice_device_q(piehip_handle h, uint32_t q, const void *d_minus_slice)
{
    NEED(h);
    int rc = slice_query_check(h, q, d_minus_slice, "minus slice");
    if (rc) return rc;
    h->slice.minus[q] = (const u64 *)d_minus_slice, h->slice.minus_seeded[q] = false;
    return PIEHIP_OK;
}

// ---- the slice side -------------------------------------------------------------------------------------------------------
int piehip_run_slice(piehip_handle h)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    SliceState &s = h->slice;
    if (!s.on) return fail(PIEHIP_ESTATE, "run_slice: not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
    if (!s.u_n()) return PIEHIP_OK;   // a handle without units: nothing to compute
    if (!s.db || !s.acc || s.acc_nq != h->nq) return fail(PIEHIP_ESTATE, "run_slice: no slice buffers (an earlier allocation failed)");
    StageAQueries qs = {};
    for (u32 q = 0; q < h->nq; q++) {
        if (!s.idx[q] || !s.minus[q]) return fail(PIEHIP_ESTATE, "run_slice: a query of the batch has no index slice or minus slice");
        qs.idx[q] = s.idx[q], qs.minus[q] = s.minus[q];
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
    if (!h->slice.on) return fail(PIEHIP_ESTATE, "not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
    *d_acc_slice = h->slice.acc;
    return PIEHIP_OK;
}

int piehip_get_slice_accumulators(piehip_handle h, uint64_t *out)
{
    if (!h || !out) return fail(PIEHIP_EINVAL, "null handle or out");
    const SliceState &s = h->slice;
    if (!s.on) return fail(PIEHIP_ESTATE, "not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
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
    if (!s.on) return fail(PIEHIP_ESTATE, "run_chain: not a query-sliced handle (piehip_load_db_sliced / piehip_load_db_table_sliced)");
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
