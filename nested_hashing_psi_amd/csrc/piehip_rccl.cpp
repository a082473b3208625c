// piehip_rccl.cpp -- the collectives of a sharded server (one process per GPU) behind the C ABI, over RCCL / xGMI:
//   the final gather of the result ciphertexts to the rank that answers the client (the path's only exchange: bin layers are
//   independent, reference BatchedFHEHIPPIE.cpp:91; sendResult at BatchedFHEPSIServer.cpp:143-152), and the per-query
//   distribution of the inputs from the rank that holds the client's socket (.cpp:94-95,114-141).
// A C++ server (host/ShardedBatchedFHEPSIServer.hpp) needs nothing but this library and RCCL; torch.distributed is only the
// Python harness's way to the same collectives (shard.py).  exchange_plan.h alone knows the ranks' ranges and the transfers of the gather,
// the scatter and the exchange, and their order; this file posts a plan (post_transfers).
//
// RCCL is bound at run time (dlopen), not at link time: a one-GPU deployment never loads the 0.5 GB library, and a process that
// already holds a copy (PyTorch bundles its own librccl.so) gets THAT copy, so a communicator made elsewhere in the process can
// be attached (piehip_rccl_attach).
#include "piehip_ctx.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <chrono>
#include <mutex>
#include <thread>

using namespace piehip;

namespace {

struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    // optional (a library without them still gathers; piehip_rccl_wait then only has its time-out, piehip_rccl_agree is refused)
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    std::string error;
};

std::mutex g_rccl_mutex;
Rccl g_rccl;

// the process's RCCL: the copy that is already mapped if there is one, else the ROCm installation's
const Rccl *rccl()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    Rccl &r = g_rccl;
    if (r.lib || !r.error.empty()) return r.lib ? &r : nullptr;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names)
        if ((r.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL))) break;
    for (size_t i = 0; !r.lib && i < sizeof(names) / sizeof(names[0]); i++) r.lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!r.lib) {
        r.error = std::string("RCCL is not available: ") + dlerror();
        return nullptr;
    }
#define BIND(field, sym)                                                      \
    do {                                                                      \
        *(void **)(&r.field) = dlsym(r.lib, sym);                             \
        if (!r.field) {                                                       \
            r.error = std::string("RCCL lacks ") + sym;                       \
            r.lib = nullptr;                                                  \
            return nullptr;                                                   \
        }                                                                     \
    } while (0)
    BIND(GetUniqueId, "ncclGetUniqueId");
    BIND(CommInitRank, "ncclCommInitRank");
    BIND(CommDestroy, "ncclCommDestroy");
    BIND(GroupStart, "ncclGroupStart");
    BIND(GroupEnd, "ncclGroupEnd");
    BIND(Send, "ncclSend");
    BIND(Recv, "ncclRecv");
    BIND(Broadcast, "ncclBroadcast");
    BIND(GetErrorString, "ncclGetErrorString");
#undef BIND
    *(void **)(&r.CommAbort) = dlsym(r.lib, "ncclCommAbort");
    *(void **)(&r.CommGetAsyncError) = dlsym(r.lib, "ncclCommGetAsyncError");
    *(void **)(&r.AllReduce) = dlsym(r.lib, "ncclAllReduce");
    return &r;
}

int no_rccl()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    return fail(PIEHIP_EHIP, g_rccl.error.empty() ? "RCCL is not available" : g_rccl.error);
}

#define NCCLCHK(R, expr)                                                                                          \
    do {                                                                                                          \
        ncclResult_t r_ = (expr);                                                                                 \
        if (r_ != ncclSuccess) return fail(PIEHIP_EHIP, std::string(#expr) + ": " + (R)->GetErrorString(r_));     \
    } while (0)

#define NEED_RCCL(R)         \
    const Rccl *R = rccl(); \
    if (!R) return no_rccl()

// the one group bracket: what `body` posts is one group call; GroupEnd runs whatever body returns, the first failure names the call
template <typename Body>
int in_group(const Rccl *R, const char *who, Body body)
{
    NCCLCHK(R, R->GroupStart());
    const ncclResult_t gr = body();
    const ncclResult_t ge = R->GroupEnd();
    if (gr != ncclSuccess || ge != ncclSuccess) return fail(PIEHIP_EHIP, std::string(who) + ": " + R->GetErrorString(gr != ncclSuccess ? gr : ge));
    return PIEHIP_OK;
}

// one group call of a plan's transfers in its posting order; base(t): the device address transfer t's offset counts from
template <typename Base>
int post_transfers(piehip_ctx *h, const Rccl *R, const std::vector<PlanTransfer> &plan, Base base, const char *who)
{
    if (plan.empty()) return PIEHIP_OK;
    const ncclComm_t comm = (ncclComm_t)h->comm;
    return in_group(R, who, [&] {
        ncclResult_t gr = ncclSuccess;
        for (size_t i = 0; i < plan.size() && gr == ncclSuccess; i++) {
            const PlanTransfer &t = plan[i];
            u64 *p = base(t) + t.off;
            gr = t.send ? R->Send(p, t.words, ncclUint64, t.peer, comm, h->stream) : R->Recv(p, t.words, ncclUint64, t.peer, comm, h->stream);
        }
        return gr;
    });
}

// a device buffer of a call, kept while its size stays: the stream drains before it is replaced
int keep_buffer(piehip_ctx *h, u64 **buf, size_t *have, size_t words)
{
    if (*have == words) return PIEHIP_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    dev_free(buf);
    *have = 0;
    const int rc = dev_alloc(buf, words);
    if (rc) return rc;
    *have = words;
    return PIEHIP_OK;
}

void set_comm(piehip_ctx *h, void *comm, bool owned, int nranks, int rank)
{
    h->comm = comm;
    h->comm_owned = owned;
    h->comm_ranks = nranks;
    h->comm_rank = rank;
    h->forget_rows();   // what was agreed was agreed with the ranks of another communicator
}
void forget_comm(piehip_ctx *h) { set_comm(h, nullptr, false, 0, 0); }

}  // namespace

extern "C" {

int piehip_rccl_unique_id(void *id)
{
    if (!id) return fail(PIEHIP_EINVAL, "null id");
    NEED_RCCL(R);
    ncclUniqueId u;
    NCCLCHK(R, R->GetUniqueId(&u));
    static_assert(sizeof(u) == PIEHIP_RCCL_ID_BYTES, "ncclUniqueId size");
    memcpy(id, &u, sizeof(u));
    return PIEHIP_OK;
}

int piehip_rccl_init(piehip_handle h, const void *id, int nranks, int rank)
{
    NEED_RO(h);
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(PIEHIP_EINVAL, "rccl_init: bad rank or id");
    if (h->comm) return fail(PIEHIP_ESTATE, "rccl_init: the handle already has a communicator");
    NEED_RCCL(R);
    HIPCHK(hipSetDevice(h->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t c = nullptr;
    NCCLCHK(R, R->CommInitRank(&c, nranks, u, rank));
    set_comm(h, c, true, nranks, rank);
    return PIEHIP_OK;
}

int piehip_rccl_attach(piehip_handle h, void *comm, int nranks, int rank)
{
    NEED_RO(h);
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(PIEHIP_EINVAL, "rccl_attach: bad communicator or rank");
    if (h->comm) return fail(PIEHIP_ESTATE, "rccl_attach: the handle already has a communicator");
    if (!rccl()) return no_rccl();
    set_comm(h, comm, false, nranks, rank);
    return PIEHIP_OK;
}

int piehip_rccl_destroy(piehip_handle h)
{
    NEED_RO(h);
    if (!h->comm) return PIEHIP_OK;
    const Rccl *R = rccl();
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));  // collectives queued on the handle's stream have drained
    if (h->comm_owned && R) (void)R->CommDestroy((ncclComm_t)h->comm);
    dev_free(&h->d_gather);
    if (h->pin_gather) (void)hipHostFree(h->pin_gather);
    h->pin_gather = nullptr;
    h->gather_words = 0;
    forget_comm(h);
    return PIEHIP_OK;
}

// Giving up.  A collective is queued in the handle's stream and completes when every rank has queued its side; a rank that
// never does (it died, it failed a precondition and returned before queueing anything, it is a programming error away from the
// others) leaves its peers' streams blocked for ever -- the reference aborts the whole process on any error
// (BatchedFHEHIPPIE.cpp:15,20), a hung group of server processes is worse.  So nobody waits without a bound:
//   piehip_rccl_wait    piehip_sync with a time-out: polls the handle's stream and the communicator's asynchronous error state;
//                       when the time is up (or RCCL reports a failed peer) it ABORTS the communicator -- which releases the
//                       blocked stream -- and returns PIEHIP_EHIP.  The communicator is gone afterwards.
//   piehip_rccl_abort   the same on purpose: a rank that cannot take part any more (an exception on its way out) tears its
//                       side down so that its peers' waits end at once instead of at their time-out.
//   piehip_rccl_agree   one word from every rank, everybody learns whether ALL said yes (an all-reduce + wait): the ranks of a
//                       server call it at the end of a phase (database built? key loaded?) so that a failure on one of them
//                       ends the session everywhere before anybody enters a collective the failed rank will not join.
static int abort_comm(piehip_ctx *h, const Rccl *R)
{
    if (!h->comm) return PIEHIP_OK;
    if (R && R->CommAbort && h->comm_owned) (void)R->CommAbort((ncclComm_t)h->comm);
    forget_comm(h);
    return PIEHIP_OK;
}

int piehip_rccl_abort(piehip_handle h)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!h->comm) return PIEHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    return abort_comm(h, rccl());
}

int piehip_rccl_wait(piehip_handle h, uint32_t timeout_ms)
{
    NEED_RO(h);
    HIPCHK(hipSetDevice(h->device));
    if (!h->comm) {   // nothing of RCCL's can be in the stream: a plain wait
        HIPCHK(hipStreamSynchronize(h->stream));
        return PIEHIP_OK;
    }
    NEED_RCCL(R);
    const auto t0 = std::chrono::steady_clock::now();
    std::string why;
    auto comm_failed = [&] {   // the communicator reports a failed state: says so in `why`
        ncclResult_t ae = ncclSuccess;
        if (!R->CommGetAsyncError || R->CommGetAsyncError((ncclComm_t)h->comm, &ae) != ncclSuccess || ae == ncclSuccess || ae == ncclInProgress) return false;
        why = std::string("rccl_wait: the communicator reports ") + R->GetErrorString(ae);
        return true;
    };
    // The common case is a query's worth of work (well under a millisecond at the headline shape): the stream is polled back to back
    // for the first milliseconds -- this wait sits inside the server's online timer -- and the communicator's error state and the
    // clock are looked at every 64th poll; after 5 ms the loop backs off to one poll per 50 us.
    for (u32 polls = 0;; polls++) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(PIEHIP_EHIP, std::string("rccl_wait: ") + hipGetErrorString(q));
        if ((polls & 63) != 63) {
            std::this_thread::yield();
            continue;
        }
        if (comm_failed()) break;
        const auto waited = std::chrono::steady_clock::now() - t0;
        if (waited > std::chrono::milliseconds(timeout_ms)) {
            why = "rccl_wait: timed out after " + std::to_string(timeout_ms) + " ms -- a rank of the server group did not join the collective";
            break;
        }
        if (waited > std::chrono::milliseconds(5)) std::this_thread::sleep_for(std::chrono::microseconds(50) * 64);
    }
    // (the stream has drained; a transfer that FAILED also drains it: ask once more)
    if (why.empty() && !comm_failed()) return PIEHIP_OK;
    const bool owned = h->comm_owned;
    abort_comm(h, R);
    if (!owned)   // piehip_rccl_attach: the communicator is the caller's to abort -- until then the stream may still be blocked
        return fail(PIEHIP_EHIP, why + " (attached communicator dropped: the caller must ncclCommAbort it to release the stream)");
    (void)hipStreamSynchronize(h->stream);   // the abort released whatever of the collective sat in the stream
    return fail(PIEHIP_EHIP, why + " (communicator aborted)");
}

int piehip_rccl_agree(piehip_handle h, int ok, int *all_ok, uint32_t timeout_ms)
{
    NEED(h);
    if (!all_ok) return fail(PIEHIP_EINVAL, "null result");
    if (!h->comm) return fail(PIEHIP_ESTATE, "rccl_agree: no communicator");
    NEED_RCCL(R);
    if (!R->AllReduce) return fail(PIEHIP_EHIP, "rccl_agree: this RCCL has no ncclAllReduce");
    HIPCHK(hipSetDevice(h->device));
    Tmp tmp(h);
    TMPGET(d_word, 1);
    int32_t *pin = nullptr;
    HIPCHK(hipHostMalloc((void **)&pin, 64, hipHostMallocPortable));
    pin[0] = ok ? 1 : 0;
    int rc = PIEHIP_OK;
    do {
        if (hipMemcpyAsync(d_word, pin, 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) { rc = fail(PIEHIP_EHIP, "rccl_agree: upload"); break; }
        const ncclResult_t r = R->AllReduce(d_word, d_word, 1, ncclInt32, ncclMin, (ncclComm_t)h->comm, h->stream);
        if (r != ncclSuccess) { rc = fail(PIEHIP_EHIP, std::string("rccl_agree: ") + R->GetErrorString(r)); break; }
        if (hipMemcpyAsync(pin, d_word, 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess) { rc = fail(PIEHIP_EHIP, "rccl_agree: download"); break; }
        rc = piehip_rccl_wait(h, timeout_ms);
    } while (0);
    if (rc == PIEHIP_OK) *all_ok = pin[0] != 0;
    (void)hipHostFree(pin);
    return rc;
}

int piehip_rccl_bin_slice(uint32_t b_total, int nranks, int rank, uint32_t *bin_lo, uint32_t *bin_hi)
{
    if (!bin_lo || !bin_hi || nranks < 1 || rank < 0 || rank >= nranks) return fail(PIEHIP_EINVAL, "bad rank");
    plan_range(b_total, nranks, rank, bin_lo, bin_hi);
    return PIEHIP_OK;
}

// Rows of another shape than two components on L limbs (piehip_set_result_limbs, piehip_set_result_relin, piehip_set_chain_limbs /
// _schedule).  Both ends of a transfer must name one size, and a setting is a rank's own: so the ranks compare (components, limbs,
// queries) once, after the settings and before the first gather, and every handle remembers what all of them had.  Mechanism of
// piehip_rccl_agree: one min-reduction over the three values and their negations -- min(v) = -min(-v) exactly where all ranks gave one v.
int piehip_rccl_agree_rows(piehip_handle h, uint32_t timeout_ms, int *same)
{
    NEED(h);
    if (!same) return fail(PIEHIP_EINVAL, "null result");
    if (!h->comm) return fail(PIEHIP_ESTATE, "rccl_agree_rows: no communicator");
    NEED_RCCL(R);
    if (!R->AllReduce) return fail(PIEHIP_EHIP, "rccl_agree_rows: this RCCL has no ncclAllReduce");
    HIPCHK(hipSetDevice(h->device));
    h->forget_rows();
    const u32 mine[3] = {h->res_comps(), h->out_limbs(), h->nq};
    Tmp tmp(h);
    TMPGET(d_words, 3);   // (six int32)
    int32_t *pin = nullptr;
    HIPCHK(hipHostMalloc((void **)&pin, 64, hipHostMallocPortable));
    for (int i = 0; i < 3; i++) pin[i] = (int32_t)mine[i], pin[3 + i] = -(int32_t)mine[i];
    int rc = PIEHIP_OK;
    do {
        if (hipMemcpyAsync(d_words, pin, 24, hipMemcpyHostToDevice, h->stream) != hipSuccess) { rc = fail(PIEHIP_EHIP, "rccl_agree_rows: upload"); break; }
        const ncclResult_t r = R->AllReduce(d_words, d_words, 6, ncclInt32, ncclMin, (ncclComm_t)h->comm, h->stream);
        if (r != ncclSuccess) { rc = fail(PIEHIP_EHIP, std::string("rccl_agree_rows: ") + R->GetErrorString(r)); break; }
        if (hipMemcpyAsync(pin, d_words, 24, hipMemcpyDeviceToHost, h->stream) != hipSuccess) { rc = fail(PIEHIP_EHIP, "rccl_agree_rows: download"); break; }
        rc = piehip_rccl_wait(h, timeout_ms);
    } while (0);
    if (rc == PIEHIP_OK) {
        bool all = true;
        for (int i = 0; i < 3; i++) all = all && pin[i] == -pin[3 + i];
        *same = all ? 1 : 0;
        if (all) h->rows_agreed = true, h->rows_ncomp = mine[0], h->rows_limbs = mine[1], h->rows_nq = mine[2];
    }
    (void)hipHostFree(pin);
    return rc;
}

// what both gather calls refuse first
static int gather_check(const piehip_ctx *h, int root, bool has_dest)
{
    // the default row needs no agreement (every rank that has it posts the sizes it always posted); any other travels only as agreed.
    // First of all, as the settings' refusals it replaces: a handle without a communicator has agreed on nothing
    const u32 ncomp = h->res_comps(), rl = h->out_limbs(), L = h->hp.L;
    if ((ncomp != 2 || rl != L) && !(h->rows_agreed && h->rows_ncomp == ncomp && h->rows_limbs == rl && h->rows_nq == h->nq)) {
        std::string by;   // the settings that shaped the row
        if (ncomp != 2) by += " piehip_set_result_relin";
        if (h->res_limbs != L) by += " piehip_set_result_limbs";
        if (h->K >= 2 && h->chain_last() != L) by += " piehip_set_chain_limbs";
        return fail(PIEHIP_ESTATE, "gather_results: result rows of " + std::to_string(ncomp) + " components on " + std::to_string(rl) + " limbs (" +
                                       by.substr(1) + "): the ranks have not agreed on this shape since it was set (piehip_rccl_agree_rows)");
    }
    if (!h->comm) return fail(PIEHIP_ESTATE, "gather_results: no communicator (piehip_rccl_init / piehip_rccl_attach)");
    if (root < 0 || root >= h->comm_ranks) return fail(PIEHIP_EINVAL, "gather_results: root outside the communicator");
    if (h->comm_rank == root && !has_dest) return fail(PIEHIP_EINVAL, "gather_results: the root needs a destination");
    return PIEHIP_OK;
}

int piehip_gather_results(piehip_handle h, uint32_t b_total, int root, void *d_out)
{
    NEED(h);   // the handle's stream is behind the run whose results travel
    int rc = gather_check(h, root, d_out != nullptr);
    if (rc) return rc;
    const int G = h->comm_ranks, me = h->comm_rank;
    u32 lo, hi;
    plan_range(b_total, G, me, &lo, &hi);
    if (hi - lo != (h->d_out ? h->b : 0u))
        return fail(PIEHIP_EINVAL, "gather_results: this handle does not evaluate its rank's slice of the bin layers (piehip_rccl_bin_slice)");
    NEED_RCCL(R);
    HIPCHK(hipSetDevice(h->device));
    // exact sizes, no padding: each slice crosses its own xGMI link once, straight into its rows of d_out; the root's own rows are a device copy
    const ExchangeShape shape = {h->K, h->hp.L, b_total, h->nq, h->hp.N, h->E, h->res_comps(), h->out_limbs()};
    auto base = [&](const PlanTransfer &t) -> u64 * { return t.buf == PLAN_GATHERED ? (u64 *)d_out : h->d_out; };
    if ((rc = post_transfers(h, R, gather_plan(shape, G, me, root), base, "gather_results"))) return rc;
    const size_t row = plan_row_words(shape);   // words per bin layer: its nq result ciphertexts
    if (me == root && hi > lo)
        HIPCHK(hipMemcpyAsync((u64 *)d_out + (size_t)lo * row, h->d_out, (size_t)(hi - lo) * row * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
    return PIEHIP_OK;
}

int piehip_gather_results_host(piehip_handle h, uint32_t b_total, int root, uint64_t **results)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    int rc = gather_check(h, root, results != nullptr);
    if (rc) return rc;
    const bool is_root = h->comm_rank == root;
    if (is_root) {   // the device half is a kept buffer; the page-locked half goes when that is replaced
        HIPCHK(hipSetDevice(h->device));
        const size_t words = (size_t)b_total * h->nq * h->res_ct_words();
        const bool same = h->gather_words == words;
        if ((rc = keep_buffer(h, &h->d_gather, &h->gather_words, words))) return rc;   // (drains the stream before it replaces)
        if (!same && h->pin_gather) (void)hipHostFree(h->pin_gather), h->pin_gather = nullptr;
        if (!h->pin_gather && words) HIPCHK(hipHostMalloc((void **)&h->pin_gather, words * sizeof(u64), hipHostMallocPortable));
    }
    if ((rc = piehip_gather_results(h, b_total, root, is_root ? h->d_gather : nullptr))) return rc;
    if (is_root) {
        HIPCHK(hipMemcpyAsync(h->pin_gather, h->d_gather, h->gather_words * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        *results = h->pin_gather;
    } else if (results) {
        *results = nullptr;
    }
    return PIEHIP_OK;
}

int piehip_rccl_broadcast(piehip_handle h, int root, void *d_buf, size_t bytes)
{
    NEED(h);
    if (!h->comm) return fail(PIEHIP_ESTATE, "rccl_broadcast: no communicator");
    if (!d_buf && bytes) return fail(PIEHIP_EINVAL, "null buffer");
    if (root < 0 || root >= h->comm_ranks) return fail(PIEHIP_EINVAL, "rccl_broadcast: root outside the communicator");
    NEED_RCCL(R);
    HIPCHK(hipSetDevice(h->device));
    if (bytes) NCCLCHK(R, R->Broadcast(d_buf, d_buf, bytes, ncclChar, root, (ncclComm_t)h->comm, h->stream));
    return PIEHIP_OK;
}

int piehip_rccl_broadcast_query(piehip_handle h, int root)
{
    NEED(h);
    if (!h->comm) return fail(PIEHIP_ESTATE, "rccl_broadcast_query: no communicator");
    if (!h->K) return fail(PIEHIP_ESTATE, "load the database before the query");
    if (root < 0 || root >= h->comm_ranks) return fail(PIEHIP_EINVAL, "rccl_broadcast_query: root outside the communicator");
    NEED_RCCL(R);
    HIPCHK(hipSetDevice(h->device));
    // the root's staged uploads are on its stream (piehip_stage_*: in order); the collective is queued behind them.  A root
    // with a half-staged query is a call-order error everywhere (the other ranks would wait for a broadcast that never comes),
    // so it is checked before anything is queued.
    if (h->comm_rank == root) {
        if (!h->stage_open) return fail(PIEHIP_ESTATE, "rccl_broadcast_query: the root has no staged query");
        if (stage_has_seeded(h))   // the expansion is queued by piehip_run_staged, which a broadcast query never reaches
            return fail(PIEHIP_ESTATE, "rccl_broadcast_query: seeded pieces are not distributed (stage full ciphertexts)");
        for (u32 q = 0; q < h->nq; q++) {
            if (!h->query[q].minus_staged) return fail(PIEHIP_ESTATE, "rccl_broadcast_query: minus element not staged");
            for (u32 hf = 0; hf < h->K; hf++)
                if (!h->query[q].rows[hf]) return fail(PIEHIP_ESTATE, "rccl_broadcast_query: index matrix row not staged");
        }
    }
    const size_t iw = (size_t)h->K * h->E * 2 * h->LN(), mw = 2 * h->LN();
    const ncclComm_t comm = (ncclComm_t)h->comm;
    int brc = PIEHIP_OK;   // query_input_buffers failed in the middle: the group is still closed, its own outcome does not count
    const int rc = in_group(R, "rccl_broadcast_query", [&] {
        ncclResult_t gr = ncclSuccess;
        for (u32 q = 0; q < h->nq && gr == ncclSuccess; q++) {
            u64 *di = nullptr, *dm = nullptr;
            if ((brc = query_input_buffers(h, q, &di, &dm))) break;
            gr = R->Broadcast(di, di, iw, ncclUint64, root, comm, h->stream);
            if (gr == ncclSuccess) gr = R->Broadcast(dm, dm, mw, ncclUint64, root, comm, h->stream);
        }
        return gr;
    });
    if (brc || rc) return brc ? brc : rc;
    // every rank now evaluates the received copy: as if the query had been staged here
    h->stage_open = false;
    use_owned_inputs(h);
    return PIEHIP_OK;
}

// ---- query slices across the ranks (exchange_plan.h; DESIGN.md section 6 "Query slices across processes") ------------------------------
// what both calls refuse, before anything is queued: no communicator, an unsliced handle, ranges other than the rule's for this rank
// (every rank derives its peers' ranges from the rule: nobody exchanges them)
static int sliced_rank_check(const piehip_ctx *h, const char *who)
{
    if (!h->comm) return fail(PIEHIP_ESTATE, std::string(who) + ": no communicator (piehip_rccl_init / piehip_rccl_attach)");
    const SliceState &s = h->slice;
    if (!s.on) return fail(PIEHIP_ESTATE, std::string(who) + ": not a query-sliced handle (piehip_build_db_sliced / piehip_load_db_sliced)");
    u32 u_lo, u_hi, bin_lo, bin_hi;
    plan_range(h->K * h->hp.L, h->comm_ranks, h->comm_rank, &u_lo, &u_hi);
    plan_range(s.b_total, h->comm_ranks, h->comm_rank, &bin_lo, &bin_hi);
    if (u_lo != s.u_lo || u_hi != s.u_hi || bin_lo != s.bin_lo || bin_hi != s.bin_hi)
        return fail(PIEHIP_EINVAL, std::string(who) + ": the handle's unit or bin-layer range is not its rank's (piehip_query_slice, piehip_rccl_bin_slice)");
    return PIEHIP_OK;
}

static ExchangeShape exchange_shape(const piehip_ctx *h) { return {h->K, h->hp.L, h->slice.b_total, h->nq, h->hp.N, h->E}; }

int piehip_rccl_scatter_query(piehip_handle h, int root)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    int rc = sliced_rank_check(h, "rccl_scatter_query");
    if (rc) return rc;
    const int G = h->comm_ranks, me = h->comm_rank;
    if (root < 0 || root >= G) return fail(PIEHIP_EINVAL, "rccl_scatter_query: root outside the communicator");
    SliceState &s = h->slice;
    const u32 N = h->hp.N, L = h->hp.L, E = h->E, KL = h->K * L, un = s.u_n();
    for (u32 q = 0; me == root && q < h->nq; q++)
        if (!s.pin_idx[q] || !s.pin_minus[q])
            return fail(PIEHIP_ESTATE, "rccl_scatter_query: the root has no host arrays for a query of the batch (piehip_slice_host_buffers_q)");
    NEED_RCCL(R);
    join_pending(h);
    mark_dirty(h);
    HIPCHK(hipSetDevice(h->device));
    for (u32 q = 0; un && q < h->nq; q++)
        for (int p = 0; p < SLICE_PIECES; p++) {
            SliceInput &in = s.in[q][p];
            if (!in.own && (rc = dev_alloc(&in.own, (size_t)un * piece_cts(p, E) * 2 * N))) return rc;
        }
    // the root's staging area, per query idx[K L][E][2][N] then minus[K L][2][N]: every unit cut out of the page-locked whole-query
    // arrays by the strided copies of a slice setter (slice_geometry.h, one per unit and piece), so that a rank's units are contiguous
    const size_t mw = 2 * (size_t)N, iw = mw * E, perq = (size_t)KL * (iw + mw);
    if (me == root) {
        if ((rc = keep_buffer(h, &s.scatter_stage, &s.scatter_words, perq * h->nq))) return rc;
        for (u32 q = 0; q < h->nq; q++)
            for (int p = 0; p < SLICE_PIECES; p++) {
                const u64 *src = p == SLICE_INDEX ? s.pin_idx[q] : s.pin_minus[q];
                u64 *dst = s.scatter_stage + q * perq + (p == SLICE_INDEX ? 0 : (size_t)KL * iw);
                for (u32 u = 0; u < KL; u++) {
                    const SliceCopy g = slice_copy((SlicePiece)p, SLICE_WHOLE, false, N, L, E, 0, KL, u);
                    HIPCHK(hipMemcpy2DAsync(dst + g.dst_off, g.dst_pitch * sizeof(u64), src + g.src_off, g.src_pitch * sizeof(u64), N * sizeof(u64),
                                            g.rows, hipMemcpyHostToDevice, h->stream));
                }
            }
    }
    auto base = [&](const PlanTransfer &t) -> u64 * {
        switch (t.buf) {
        case PLAN_STAGE_INDEX: return s.scatter_stage + t.q * perq;
        case PLAN_STAGE_MINUS: return s.scatter_stage + t.q * perq + (size_t)KL * iw;
        case PLAN_OWN_INDEX: return s.in[t.q][SLICE_INDEX].own;
        default: return s.in[t.q][SLICE_MINUS].own;
        }
    };
    if ((rc = post_transfers(h, R, scatter_plan(exchange_shape(h), G, me, root), base, "rccl_scatter_query"))) return rc;
    for (u32 q = 0; un && q < h->nq; q++) {
        if (me == root) {   // the root's own units: a device copy
            const u64 *st = s.scatter_stage + q * perq;
            HIPCHK(hipMemcpyAsync(s.in[q][SLICE_INDEX].own, st + s.u_lo * iw, un * iw * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(s.in[q][SLICE_MINUS].own, st + (size_t)KL * iw + s.u_lo * mw, un * mw * sizeof(u64), hipMemcpyDeviceToDevice,
                                  h->stream));
        }
        // the next piehip_run_slice reads the owned copies; nothing is expanded over them (as after any unseeded setter)
        for (SliceInput &in : s.in[q]) in.cur = in.own, in.seeded = false;
    }
    return PIEHIP_OK;
}

int piehip_rccl_exchange_accumulators(piehip_handle h)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    int rc = sliced_rank_check(h, "rccl_exchange_accumulators");
    if (rc) return rc;
    SliceState &s = h->slice;
    const int G = h->comm_ranks, me = h->comm_rank;
    const u32 KL = h->K * h->hp.L, bn = s.bin_hi - s.bin_lo;
    if (KL > PLACE_MAX_UNITS) return fail(PIEHIP_EINVAL, "rccl_exchange_accumulators: more units than one placement launch takes");
    for (u32 u = 0; u < KL; u++)
        if (s.put[u]) return fail(PIEHIP_ESTATE, "rccl_exchange_accumulators: a unit has been put since the last piehip_run_chain");
    if (s.u_n() && (!s.acc || s.acc_nq != h->nq)) return fail(PIEHIP_ESTATE, "rccl_exchange_accumulators: no accumulator buffer");
    if (bn && (!h->d_acc || !h->ws.eqp)) return fail(PIEHIP_ESTATE, "rccl_exchange_accumulators: no workspace (an earlier allocation failed)");
    NEED_RCCL(R);
    join_pending(h);   // the placement writes what the queues of the last piehip_run_chain read
    mark_dirty(h);
    HIPCHK(hipSetDevice(h->device));
    const ExchangeShape shape = exchange_shape(h);
    if ((rc = keep_buffer(h, &s.xchg_stage, &s.xchg_words, G > 1 ? plan_acc_stage_words(shape, bn) : 0))) return rc;
    auto base = [&](const PlanTransfer &t) -> u64 * { return t.buf == PLAN_ACC_SLICE ? s.acc : s.xchg_stage; };
    if ((rc = post_transfers(h, R, exchange_plan(shape, G, me), base, "rccl_exchange_accumulators"))) return rc;
    if (bn) {   // every unit from the block that holds it, in one launch
        PlaceSources src = {};
        for (u32 u = 0; u < KL; u++) {
            const PlanUnitSource us = plan_unit_source(shape, G, me, u);
            src.of[u] = {us.own ? s.acc : s.xchg_stage + us.off, us.own ? s.bin_lo * h->nq : 0u, us.u_lo, us.u_n};
        }
        StageAXOut xo;
        const bool x_direct = run_x_direct(h);
        if (x_direct) xo.out = h->ws.eqp, xo.M = h->hp.M, xo.logns = h->plan.lane_logn;
        ProfScope ps(h, PIEHIP_K_OTHER, 16.0 * h->hp.N * (double)bn * h->nq * KL * 2);
        launch_place_units(h->hp.N, h->hp.L, h->K, bn * h->nq, src, h->d_acc, x_direct ? &xo : nullptr, h->stream);
        HIPCHK(hipGetLastError());
    }
    std::fill(s.put.begin(), s.put.end(), true);
    return PIEHIP_OK;
}

}  // extern "C"
