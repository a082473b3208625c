// ShardedBatchedFHEPSIServer.hpp -- the reference's server (src/Server/FHE/BatchedFHEPSIServer.{hpp,cpp}, phases of
// src/Server/PSIServer.hpp:66-87) as ONE PROCESS PER GPU, in C++ over the C ABI only: no Python, no torch.
//
// Rank 0 is the process that holds the client's channel (the reference server, .cpp:94-95); ranks 1 .. G-1 are workers on the
// other GPUs of the node.  Every rank keeps a contiguous slice of the bin layers of the same table (the outer
// loop of run(), BatchedFHEHIPPIE.cpp:91, has independent iterations) and a copy of the EvalMult key.
//
//   set-up   rank 0 receives context, public key, EvalMult key from the client (.cpp:21-54) and forwards context, key, the
//            table seeds and the RCCL unique id to the workers over the side channels (one connected socket per worker, the
//            framing of WireFraming.hpp -- host-side, once per session); every rank creates its context and joins the
//            communicator (piehip_rccl_init)
//   offline  every rank hashes the server set and packs ITS bin layers (piehip_build_db_bins, same seeds: slices of one table)
//   online   rank 0 receives the query and stages every piece as it lands (PCIe under the receive loop); then, inside the
//            reference's timer (.cpp:98-106): the query goes to every rank over xGMI (piehip_rccl_broadcast_query), every rank
//            runs its layers (piehip_run), the result ciphertexts are gathered to rank 0 (piehip_gather_results -- the
//            evaluation's only exchange) and come down to host memory; rank 0 answers the client (.cpp:143-152)
// Query-sliced mode (querySlices = true, set before run(); include/piehip.h "Query slices"): no rank needs the whole query.  Rank r holds
// the units of piehip_query_slice(K, L, G, r) of the database for all bin layers and runs the product chain of its bin layers; either
// share may be empty, so G > b and G > K L are legal.
//   offline  every rank hashes the server set and encodes ITS units and the masks of ITS bin layers (piehip_build_db_sliced)
//   online   rank 0 unpacks the query into its page-locked whole-query arrays (piehip_slice_host_buffers_q); then, inside the timer:
//            every rank is sent its units' slices (piehip_rccl_scatter_query), computes those limbs of every accumulator
//            (piehip_run_slice), sends every rank the rows of its bin layers (piehip_rccl_exchange_accumulators), runs its chains
//            (piehip_run_chain); gather and answer as above
// Error handling is the reference's -- exceptions end the process (BatchedFHEHIPPIE.cpp:15,20 throw, nothing catches) -- made safe
// for a GROUP of processes: a collective only completes when every rank joins it, so
//   * at the end of the offline phase the ranks agree that everybody built its slice (piehip_rccl_agree): a rank whose build threw
//     says no on its way out and all of them end the session there, before anybody waits in a collective for it;
//   * every wait for a collective has a bound (piehip_rccl_wait, collectiveTimeoutMs): a rank that died in the online phase costs
//     its peers that time-out and an exception, not a hung group of server processes;
//   * a rank that leaves run() by exception aborts its side of the communicator first (piehip_rccl_abort), which ends its peers'
//     waits at once.
#pragma once
#include <chrono>
#include <exception>
#include <memory>
#include <random>

#include "BatchedFHEPSIServer.hpp"

namespace piehip {

class ShardedBatchedFHEPSIServer {
public:
    // rank 0: client_fd = the client's channel, side_fds = one connected socket per worker (index r - 1 for rank r);
    // rank r > 0: client_fd = -1, side_fds = {the socket to rank 0}
    ShardedBatchedFHEPSIServer(int rank, int nranks, int device, int client_fd, const std::vector<int> &side_fds,
                               const std::vector<uint64_t> &serverSet, const HashTableParameter &htParams, uint64_t hashSeed = 987654321)
        : rank(rank), G(nranks), device(device), fd(client_fd), side(side_fds), serverSet(serverSet), ht(htParams), hashSeed(hashSeed)
    {
        if (G < 1 || rank < 0 || rank >= G) throw std::invalid_argument("rank outside the server group");
        if ((rank == 0 && side.size() != (size_t)G - 1) || (rank > 0 && side.size() != 1))
            throw std::invalid_argument("side channels: one per worker on rank 0, one to rank 0 on a worker");
        if (ht.serverStashSize != 0) throw std::invalid_argument("Error, batched FHE PIE does not support a stash (yet).");
        if (rank == 0) {  // secret per session, as in the reference (CuckooHashTable.cpp:51-52, BatchedFHEHIPPIE.cpp:25-26)
            std::random_device rd;
            auto u64 = [&rd] { return ((uint64_t)rd() << 32) ^ (uint64_t)rd(); };
            seeds[0] = u64(), seeds[1] = u64(), seeds[2] = u64();
        }
    }
    void setSecretSeedsForTesting(uint64_t evict, uint64_t shuffle, uint64_t mask) { seeds[0] = evict, seeds[1] = shuffle, seeds[2] = mask; }

    void run()  // PSIServer.hpp:66-87
    {
        if (querySlices && rowSettings())   // (a sliced handle refuses them one by one; here before the first message is read)
            throw std::invalid_argument("resultLimbs, chainLimbs, chainSchedule and resultRelin = false apply in bin-layer mode only, not with querySlices");
        try {
            runSetUpPhase();
            if (rank == 0) wire::signalPhaseOver(fd);
            runOfflinePhase();
            if (rank == 0) wire::signalPhaseOver(fd);
            runOnlinePhase();
        } catch (...) {
            if (cc) (void)piehip_rccl_abort(cc->handle());   // the peers' waits end now, not at their time-out
            throw;
        }
    }

    bool querySlices = false;               // stage A sharded by (inner hash function, limb) unit: see above
    // The shape of a result row (include/piehip.h "Result limbs", "Chain limbs", "Result relinearisation"), bin-layer mode only, set
    // before run() and THE SAME ON EVERY RANK: every rank applies them in the set-up phase and the ranks then compare their row shapes
    // (piehip_rccl_agree_rows); ranks started with different values all end the session there with std::invalid_argument.  The result
    // messages carry piehip_get_result_components components of min(resultLimbs, chain limbs) limbs.  With resultRelin = false and two
    // Cuckoo hash functions the client may send an empty EvalMult key message (BatchedFHEPSIServer::setResultRelin); rank 0 forwards it
    // like any other.  The noise budget of a setting is the operator's business.
    uint32_t resultLimbs = 0;               // 0 = every limb
    uint32_t chainLimbs = 0;                // 0 = every limb; ignored where chainSchedule is set
    std::vector<uint32_t> chainSchedule;    // piehip_set_chain_schedule: a limb count per product
    bool resultRelin = true;
    bool failOfflineForTesting = false;     // this rank's database build "fails": the group must end the session, not hang
    uint32_t collectiveTimeoutMs = 30000;   // bound on every wait for the other ranks (piehip_rccl_wait / piehip_rccl_agree)

    long long offlineComputation = 0, onlineComputation = 0;  // microseconds (rank 0: PSIServer.hpp:89-103)

    void runSetUpPhase()
    {
        // rank 0 reads the client's messages (.cpp:21-54) and forwards id, context, seeds, key; a worker reads those from rank 0
        const int from = rank == 0 ? fd : side[0];
        std::vector<uint8_t> m;
        auto readExactly = [&](void *dst, size_t bytes, const char *what) {
            wire::readWithSizeIntoVector(from, m);
            if (m.size() != bytes) throw std::runtime_error(what);
            std::memcpy(dst, m.data(), bytes);
        };
        uint8_t id[PIEHIP_RCCL_ID_BYTES];
        if (rank > 0) readExactly(id, sizeof(id), "unique id message size");
        const ContextMessage c = readContextMessage(from);
        if (rank > 0) readExactly(seeds, sizeof(seeds), "seed message size");
        else wire::readWithSizeIntoVector(from, m);  // public key: unused by the operator
        // (rank 0 has checked what it forwards; an empty key message is forwarded like any other and judged on every rank alike, below)
        const std::vector<uint64_t> evk = readEvalMultKey(from, c, rank == 0 ? c.moduli : nullptr, true);
        if (rank == 0) {
            PieContext::check(piehip_rccl_unique_id(id));
            for (int s : side) {  // session set-up for the workers
                wire::writeWithSize(s, id, sizeof(id));
                wire::writeWithSize(s, &c, sizeof(c));
                wire::writeWithSize(s, seeds, sizeof(seeds));
                wire::writeWithSize(s, evk.data(), evk.size() * sizeof(uint64_t));
            }
        }
        cc.reset(new PieContext(c.N, c.L, c.t, c.moduli, c.moduli + c.L, device));
        qMod.assign(c.moduli, c.moduli + c.L);
        if (evk.empty() && !(ht.numberOfCuckooHashFunctions == 2 && !resultRelin))
            throw std::invalid_argument("empty EvalMult key message: only a server with two Cuckoo hash functions and resultRelin = false runs without a key");
        if (!evk.empty()) cc->setEvalMultKey(evk.data());
        PieContext::check(piehip_rccl_init(cc->handle(), id, G, rank));
        if (rowSettings()) {
            // a setter that refuses throws here and run() aborts this rank's side: the peers' agreement ends at once, not at its bound
            if (resultLimbs) PieContext::check(piehip_set_result_limbs(cc->handle(), resultLimbs));
            if (!chainSchedule.empty()) PieContext::check(piehip_set_chain_schedule(cc->handle(), chainSchedule.data(), (uint32_t)chainSchedule.size()));
            else if (chainLimbs) PieContext::check(piehip_set_chain_limbs(cc->handle(), chainLimbs));
            if (!resultRelin) PieContext::check(piehip_set_result_relin(cc->handle(), 0));
        }
        PieContext::check(piehip_rccl_bin_slice(ht.maxItemsPerPosition, G, rank, &lo, &hi));
        if (hi > lo)
            PieContext::check(piehip_reserve(cc->handle(), serverSet.size(), ht.numberOfSimpleHashFunctions, ht.eachSimpleTableSize,
                                             ht.numberOfCuckooHashFunctions, ht.maxItemsPerPosition, ht.eachCuckooTableSize, lo, hi));
    }

    void runOfflinePhase()
    {
        const auto begin = std::chrono::steady_clock::now();
        const uint32_t K = ht.numberOfCuckooHashFunctions, E = ht.eachCuckooTableSize;
        buildAndAgree([&] {
            if (!querySlices && hi <= lo) throw std::runtime_error("more ranks than bin layers: start at most eachBinSize server processes");
            if (failOfflineForTesting) throw std::runtime_error("offline phase failed on this rank (test)");
            uint32_t ulo = 0, uhi = 0;
            if (querySlices) {
                PieContext::check(piehip_query_slice(K, cc->towers(), G, rank, &ulo, &uhi));
                PieContext::check(piehip_build_db_sliced(cc->handle(), serverSet.data(), serverSet.size(), ht.numberOfSimpleHashFunctions,
                                                         ht.eachSimpleTableSize, K, ht.maxItemsPerPosition, E, hashSeed, seeds[0], seeds[1],
                                                         seeds[2], ulo, uhi, lo, hi));
            } else {
                PieContext::check(piehip_build_db_bins(cc->handle(), serverSet.data(), serverSet.size(), ht.numberOfSimpleHashFunctions,
                                                       ht.eachSimpleTableSize, K, ht.maxItemsPerPosition, E, hashSeed, seeds[0], seeds[1],
                                                       seeds[2], lo, hi));
            }
            PieContext::check(piehip_sync(cc->handle()));
        });
        // The database is in place (its K decides the components and limbs of a row, and loading it forgets an agreement): the ranks
        // compare what their settings made of a result row, once per session, before the first gather
        if (rowSettings()) {
            int same = 0;
            PieContext::check(piehip_rccl_agree_rows(cc->handle(), collectiveTimeoutMs, &same));
            if (!same)
                throw std::invalid_argument("the ranks of the server group were started with different resultLimbs, chainLimbs, chainSchedule or "
                                            "resultRelin: their result rows differ in shape");
        }
        // one evaluation of an all-zero query through the whole online path (code objects, queues, the communicator's first
        // collective) while nobody waits for it.  Only rank 0 ever holds a whole query in host memory: the workers of the broadcast mode
        // get their device-side input buffers and run queues, no page-locked index matrix (29 MiB at C3 that nothing would ever write)
        if (rank == 0) {
            uint64_t *pinIdx = nullptr, *pinMinus = nullptr;
            hostArrays(&pinIdx, &pinMinus);
            zeroQuery(pinIdx, pinMinus, K, E, ctWords());
            if (!querySlices) {
                PieContext::check(piehip_stage_minus(cc->handle(), pinMinus));
                for (uint32_t h = 0; h < K; h++) PieContext::check(piehip_stage_index_row(cc->handle(), h, pinIdx + (size_t)h * E * ctWords()));
            }
        } else if (!querySlices) {
            PieContext::check(piehip_host_buffers(cc->handle(), nullptr, nullptr, nullptr));
        }
        evaluateQuery();
        offlineComputation = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begin).count();
    }

    void runOnlinePhase()
    {
        const uint32_t L = cc->towers(), N = cc->ringDimension(), K = ht.numberOfCuckooHashFunctions, E = ht.eachCuckooTableSize;
        if (rank == 0) {
            uint64_t *pinIdx = nullptr, *pinMinus = nullptr;
            hostArrays(&pinIdx, &pinMinus);
            if (querySlices) {   // the scatter reads the host arrays: nothing is staged
                receiveQuery(fd, L, N, K, E, qMod.data(), pinIdx, pinMinus);
            } else {
                try {   // every message staged as it lands
                    receiveQuery(fd, L, N, K, E, qMod.data(), pinIdx, pinMinus, stagePieces(cc->handle(), 0));
                } catch (...) {
                    piehip_stage_reset(cc->handle());
                    throw;
                }
            }
        }
        const auto begin = std::chrono::steady_clock::now();
        const uint64_t *results = evaluateQuery();  // .cpp:101-103 across the ranks
        onlineComputation = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begin).count();
        if (rank == 0) {   // framed with the shape the ranks agreed on: this handle's
            uint32_t ncomp = 0, rl = 0;
            rowShape(&ncomp, &rl);
            sendResults(fd, results, ht.maxItemsPerPosition, (size_t)ncomp * rl * N, rl, N, ncomp);
        }
    }

private:
    size_t ctWords() const { return 2 * (size_t)cc->towers() * cc->ringDimension(); }   // a query ciphertext
    bool rowSettings() const { return resultLimbs || chainLimbs || !chainSchedule.empty() || !resultRelin; }
    // components and limbs of a result ciphertext as the handle stands
    void rowShape(uint32_t *ncomp, uint32_t *rl) const
    {
        uint32_t keep = 0, lc = 0;
        PieContext::check(piehip_get_result_components(cc->handle(), ncomp));
        PieContext::check(piehip_get_result_limbs(cc->handle(), &keep));
        PieContext::check(piehip_get_chain_limbs(cc->handle(), &lc));
        *rl = ht.numberOfCuckooHashFunctions >= 2 && lc < keep ? lc : keep;
    }

    // rank 0's page-locked whole-query arrays
    void hostArrays(uint64_t **pinIdx, uint64_t **pinMinus)
    {
        uint64_t *pinRes = nullptr;
        if (querySlices) PieContext::check(piehip_slice_host_buffers_q(cc->handle(), 0, pinIdx, pinMinus));
        else PieContext::check(piehip_host_buffers(cc->handle(), pinIdx, pinMinus, &pinRes));
    }

    // Runs this rank's database build; then every rank says whether its slice is ready, and a no anywhere ends the session everywhere (a
    // Cuckoo insertion that failed -- CuckooHashTable.cpp:113 -- fails on every rank alike; out of memory on one GPU does not)
    template <typename Build>
    void buildAndAgree(Build build)
    {
        std::exception_ptr failed;
        try {
            build();
        } catch (...) {
            failed = std::current_exception();
        }
        int allBuilt = 0;
        PieContext::check(piehip_rccl_agree(cc->handle(), failed ? 0 : 1, &allBuilt, collectiveTimeoutMs));
        if (failed) std::rethrow_exception(failed);
        if (!allBuilt) throw std::runtime_error("another rank of the server group could not build its slice of the database");
    }

    // One query across the ranks; returns the b result ciphertexts (rank 0).
    const uint64_t *evaluateQuery() { return querySlices ? evaluateSlicedQuery() : evaluateStagedQuery(); }
    // the query in rank 0's host arrays -> every rank's units; stage A there; accumulators -> the ranks of their bin layers; the chains
    const uint64_t *evaluateSlicedQuery()
    {
        PieContext::check(piehip_rccl_scatter_query(cc->handle(), 0));
        PieContext::check(piehip_run_slice(cc->handle()));
        PieContext::check(piehip_rccl_exchange_accumulators(cc->handle()));
        PieContext::check(piehip_run_chain(cc->handle()));
        return gatherToRoot();
    }
    // the query staged on rank 0 -> every rank; run()
    const uint64_t *evaluateStagedQuery()
    {
        PieContext::check(piehip_rccl_broadcast_query(cc->handle(), 0));
        PieContext::check(piehip_run(cc->handle()));
        return gatherToRoot();
    }
    // results -> rank 0's host memory: page-locked, owned by the library, [b][ncomp][rl][N] in bin order (rowShape)
    const uint64_t *gatherToRoot()
    {
        uint64_t *gathered = nullptr;
        PieContext::check(piehip_gather_results_host(cc->handle(), ht.maxItemsPerPosition, 0, &gathered));
        PieContext::check(piehip_rccl_wait(cc->handle(), collectiveTimeoutMs));   // piehip_sync with a bound
        return gathered;
    }

    int rank, G, device, fd;
    std::vector<int> side;
    std::vector<uint64_t> serverSet;
    HashTableParameter ht;
    uint64_t hashSeed;
    uint64_t seeds[3] = {0, 0, 0};  // evict, shuffle, mask: drawn on rank 0, the same on every rank (slices of ONE table)
    uint32_t lo = 0, hi = 0;
    std::vector<uint64_t> qMod;
    std::unique_ptr<PieContext> cc;
};

}  // namespace piehip
