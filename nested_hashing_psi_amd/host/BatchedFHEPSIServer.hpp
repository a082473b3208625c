// BatchedFHEPSIServer.hpp -- the caller of the hot path, in the reference's shape, over the C ABI and WireFraming.hpp.
//
// Mirrors src/Server/FHE/BatchedFHEPSIServer.{hpp,cpp} and the phase driver src/Server/PSIServer.hpp:66-87:
//     run():  runSetUpPhase(); signalPhaseOver(); runOfflinePhase(); signalPhaseOver(); runOnlinePhase();
//     setup   (.cpp:56-74)   three messages: context, public key (unused by the operator), EvalMult key
//     offline (.cpp:75-90)   insertAll(serverSet) + BatchedFHEHIPPIE construction  -> piehip_build_db (all on the device)
//     online  (.cpp:92-112)  minus ciphertext, K*E index ciphertexts (one message each, .cpp:124-141); timer around
//                            setMinusCompareElement / setIndex / run (.cpp:98-106); b results, one message each (.cpp:143-152)
// Payloads are the flat limb format of WireFraming.hpp instead of OpenFHE's cereal blobs (OpenFHE is not available here);
// with OpenFHE the same class deserialises the blobs and copies DCRTPoly towers.
//
// Several clients at once.  The reference server serves ONE client per process (.cpp:94-95: one channel).  Given a list of
// channels this class runs the same three phases with every client -- each sends its own context (they must agree), its own
// EvalMult key, its own query -- builds the database once, and evaluates the clients' queries as ONE batch
// (piehip_set_query_batch): stage A streams the packed database once for all of them.  Every client's answer is bit-identical to
// what a server of its own would have sent.
#pragma once
#include <chrono>
#include <functional>
#include <memory>
#include <random>

#include "BatchedFHEHIPPIE.hpp"
#include "WireFraming.hpp"

namespace piehip {

struct HashTableParameter {  // src/Common/Parameter/HashTableParameter.hpp
    uint32_t numberOfSimpleHashFunctions, eachSimpleTableSize, numberOfCuckooHashFunctions, eachCuckooTableSize, maxItemsPerPosition;
    uint64_t serverStashSize = 0;
};

// first setup message: what the reference's serialized CryptoContext carries for this path
struct ContextMessage {
    uint32_t N, L;
    uint64_t t;
    uint64_t moduli[2 * 7 + 1];  // q_0..q_{L-1}, p_0..p_L
};

// ---- the steps this server and both modes of ShardedBatchedFHEPSIServer share ----------------------------------------------------
inline ContextMessage readContextMessage(int fd)
{
    std::vector<uint8_t> m;
    wire::readWithSizeIntoVector(fd, m);
    if (m.size() != sizeof(ContextMessage)) throw std::runtime_error("context message size");
    ContextMessage c;
    std::memcpy(&c, m.data(), sizeof(c));
    if (c.L < 1 || c.L > 7) throw std::invalid_argument("context: L out of range");
    return c;
}

// The EvalMult key message as words [L][2][L][N], the modulus index being the innermost L.  moduli (q_0..q_{L-1}) given: the key-switch
// accumulators take canonical residues only; null where the sender has checked what it forwards.  An EMPTY message is a client that
// sends no key: with mayBeEmpty the result is empty and the caller decides (a K = 2 database whose results are not relinearised needs
// no key: include/piehip.h "Result relinearisation"), otherwise std::invalid_argument.
inline std::vector<uint64_t> readEvalMultKey(int fd, const ContextMessage &c, const uint64_t *moduli, bool mayBeEmpty = false)
{
    std::vector<uint8_t> m;
    wire::readWithSizeIntoVector(fd, m);
    if (m.empty()) {
        if (!mayBeEmpty) throw std::invalid_argument("empty EvalMult key message: this server relinearises and needs every client's key");
        return {};
    }
    const size_t words = (size_t)c.L * 2 * c.L * c.N;
    if (m.size() != words * sizeof(uint64_t)) throw std::runtime_error("EvalMult key message size");
    std::vector<uint64_t> evk(words);
    std::memcpy(evk.data(), m.data(), m.size());
    if (moduli) wire::checkCanonical(evk.data(), (size_t)c.L * 2 * c.L, c.L, c.N, moduli, "EvalMult key");
    return evk;
}

// One query, every message unpacked (and range-checked) straight into the page-locked arrays pinMinus[2][L][N] and pinIdx[K][E][2][L][N].
// onPiece(row, j, ct) is called as each ciphertext lands, with row = MINUS_ELEMENT for the minus element: a server that stages starts
// the piece's upload there (piehip_stage_*), and drops a partial staging itself when this throws.
constexpr int64_t MINUS_ELEMENT = -1;
using OnPiece = std::function<void(int64_t row, uint32_t j, uint64_t *ct)>;
inline void receiveQuery(int fd, uint32_t L, uint32_t N, uint32_t K, uint32_t E, const uint64_t *qMod, uint64_t *pinIdx, uint64_t *pinMinus,
                         const OnPiece &onPiece = nullptr)
{
    const size_t ct = 2 * (size_t)L * N;
    std::vector<uint8_t> m;
    wire::readWithSizeIntoVector(fd, m);  // receiveEncryptedMinusElements, .cpp:114-122
    wire::unpackCiphertextsInto(m, L, N, pinMinus, 1, qMod);
    if (onPiece) onPiece(MINUS_ELEMENT, 0, pinMinus);
    for (uint32_t h = 0; h < K; h++)  // receiveIndexMatrix, .cpp:124-141: one message per ciphertext
        for (uint32_t j = 0; j < E; j++) {
            uint64_t *p = pinIdx + ((size_t)h * E + j) * ct;
            wire::readWithSizeIntoVector(fd, m);
            wire::unpackCiphertextsInto(m, L, N, p, 1, qMod);
            if (onPiece) onPiece(h, j, p);
        }
}
// onPiece for a server that stages query q of handle h
inline OnPiece stagePieces(piehip_handle h, uint32_t q)
{
    return [h, q](int64_t row, uint32_t j, uint64_t *ct) {
        PieContext::check(row == MINUS_ELEMENT ? piehip_stage_minus_q(h, q, ct) : piehip_stage_index_ct_q(h, q, (uint32_t)row, j, ct));
    };
}

// sendResult, .cpp:143-152: b ciphertexts of ncomp components on `keep` limbs, one message each, rowStride words apart (two
// components: the message packCiphertexts makes, byte for byte)
inline void sendResults(int fd, const uint64_t *results, uint32_t b, size_t rowStride, uint32_t keep, uint32_t N, uint32_t ncomp = 2)
{
    for (uint32_t i = 0; i < b; i++) {
        const auto out = wire::packRows(results + (size_t)i * rowStride, 1, ncomp, keep, N);
        wire::writeWithSize(fd, out.data(), out.size());
    }
}

// the all-zero query of a warm-up
inline void zeroQuery(uint64_t *pinIdx, uint64_t *pinMinus, uint32_t K, uint32_t E, size_t ct)
{
    std::memset(pinMinus, 0, ct * sizeof(uint64_t));
    std::memset(pinIdx, 0, (size_t)K * E * ct * sizeof(uint64_t));
}

class BatchedFHEPSIServer {
public:
    // Cuckoo evictions, the bin-layer shuffle and the random masks are seeded from std::random_device, as in the reference
    // (CuckooHashTable.cpp:51-52, BatchedFHEHIPPIE.cpp:25-26): the masks hide non-matching slots from the client and the
    // shuffle hides the bin order.  setSecretSeedsForTesting() makes a run reproducible (parity tests only).
    BatchedFHEPSIServer(int channel_fd, const std::vector<uint64_t> &serverSet, const HashTableParameter &htParams, uint64_t hashSeed = 987654321)
        : BatchedFHEPSIServer(std::vector<int>{channel_fd}, serverSet, htParams, hashSeed)
    {
    }
    // one channel per client; their queries are evaluated together (at most 8: the library's batch limit)
    // chainLimbs (include/piehip.h "Chain limbs"; 0 = all L, the reference's behaviour): the product chain runs on the first chainLimbs
    // limbs of the clients' chain, and the result messages carry min(keep, chainLimbs) limbs, framed with that count: the clients
    // decrypt in the context of those limbs.  The noise budget is the operator's business; std::invalid_argument from the set-up
    // phase when it exceeds the clients' L.
    BatchedFHEPSIServer(const std::vector<int> &channel_fds, const std::vector<uint64_t> &serverSet, const HashTableParameter &htParams,
                        uint64_t hashSeed = 987654321, uint32_t chainLimbs = 0)
        : fds(channel_fds), serverSet(serverSet), ht(htParams), hashSeed(hashSeed), chainLimbs(chainLimbs)
    {
        if (fds.empty() || fds.size() > 8) throw std::invalid_argument("between one and eight client channels");
        std::random_device rd;
        auto u64 = [&rd] { return ((uint64_t)rd() << 32) ^ (uint64_t)rd(); };
        evictSeed = u64();
        shuffleSeed = u64();
        maskSeed = u64();
        if (ht.serverStashSize != 0) throw std::invalid_argument("Error, batched FHE PIE does not support a stash (yet).");
    }

    void run()  // PSIServer.hpp:66-87
    {
        runSetUpPhase();
        for (int fd : fds) wire::signalPhaseOver(fd);
        runOfflinePhase();
        for (int fd : fds) wire::signalPhaseOver(fd);
        runOnlinePhase();
    }

    void setSecretSeedsForTesting(uint64_t evict, uint64_t shuffle, uint64_t mask)
    {
        evictSeed = evict;
        shuffleSeed = shuffle;
        maskSeed = mask;
    }

    // Result limbs (include/piehip.h "Result limbs"): the result messages carry the first `keep` limbs of every result ciphertext
    // (0 = all L, the reference's behaviour) -- reduced on the device before they come down, framed with `keep` limbs by sendResult.
    // The clients decrypt in the context (N, keep, t, q[:keep]).  Call before run(); std::invalid_argument from the set-up phase when
    // keep exceeds the clients' L.
    void setResultLimbs(uint32_t keep) { resultLimbs = keep; }

    // Layer tiling (include/piehip.h "Layer tiling"; off = the reference's packing): the database packs R bin layers side by side into
    // every plaintext, R being piehip_layer_tiling's balanced choice for the clients' ring and this server's table sizes, and the server
    // sends tiledLayers() = ceil(maxItemsPerPosition / R) result messages instead of maxItemsPerPosition.  The wire format does not
    // change: the clients make the same choice from the same numbers, repeat the slots of every query vector R times, and read block r of
    // result g as bin layer g R + r.  Call before run().
    void setLayerTiling(bool on) { layerTiling = on; }

    // Result relinearisation (include/piehip.h "Result relinearisation"; on = the reference's behaviour): off, the last product of the
    // chain is not relinearised and every result message carries THREE components (WireFraming.hpp, packRows), which the clients decrypt
    // as d0 + d1 s + d2 s^2.  With two Cuckoo hash functions the chain then uses no EvalMult key at all: a client may send an EMPTY key
    // message, recognised by its place in the set-up phase, and no key is loaded for it; a key that does arrive is loaded as ever.  In
    // every other case an empty key message is std::invalid_argument.  Call before run().
    void setResultRelin(bool on) { resultRelin = on; }
    uint32_t tiledLayers() const { return tiled ? tiled : ht.maxItemsPerPosition; }   // known once the set-up phase has the context

    long long offlineComputation = 0, onlineComputation = 0;  // microseconds, PSIServer.hpp:89-103

    void runSetUpPhase()  // receiveAndSetContextAndKeys, BatchedFHEPSIServer.cpp:21-54, once per client
    {
        const uint32_t nq = (uint32_t)fds.size();
        std::vector<uint8_t> m;
        ContextMessage c0;
        for (uint32_t q = 0; q < nq; q++) {
            const int fd = fds[q];
            const ContextMessage c = readContextMessage(fd);
            if (q == 0) {
                c0 = c;
                cc.reset(new PieContext(c.N, c.L, c.t, c.moduli, c.moduli + c.L));
                qMod.assign(c.moduli, c.moduli + c.L);
                // the table sizes are known since construction (htParams): allocate the database, workspace and scratch now, so
                // the timed offline phase does not pay for hipMalloc
                PieContext::check(piehip_set_query_batch(cc->handle(), nq));
                if (resultLimbs) PieContext::check(piehip_set_result_limbs(cc->handle(), resultLimbs));
                if (chainLimbs) PieContext::check(piehip_set_chain_limbs(cc->handle(), chainLimbs));
                if (!resultRelin) PieContext::check(piehip_set_result_relin(cc->handle(), 0));
                if (layerTiling) {
                    uint32_t R = 1;
                    PieContext::check(piehip_layer_tiling(c.N, ht.numberOfSimpleHashFunctions, ht.eachSimpleTableSize, ht.maxItemsPerPosition,
                                                          &R, &tiled));
                    PieContext::check(piehip_set_layer_tiling(cc->handle(), R));
                }
                PieContext::check(piehip_reserve(cc->handle(), serverSet.size(), ht.numberOfSimpleHashFunctions, ht.eachSimpleTableSize,
                                                 ht.numberOfCuckooHashFunctions, ht.maxItemsPerPosition, ht.eachCuckooTableSize, 0,
                                                 tiledLayers()));
            } else if (c.N != c0.N || c.L != c0.L || c.t != c0.t || std::memcmp(c.moduli, c0.moduli, sizeof(uint64_t) * (2 * c.L + 1))) {
                throw std::invalid_argument("the clients of one batch must use the same crypto context parameters");
            }
            wire::readWithSizeIntoVector(fd, m);  // public key: stored by the reference, never used by the operator
            const std::vector<uint64_t> evk = readEvalMultKey(fd, c, qMod.data(), !resultRelin && ht.numberOfCuckooHashFunctions == 2);
            if (evk.empty()) continue;   // (allowed above: the chain of this server uses no key)
            if (nq == 1) cc->setEvalMultKey(evk.data());
            else PieContext::check(piehip_load_relin_key_q(cc->handle(), q, evk.data()));  // every client's own key
        }
    }

    void runOfflinePhase()  // BatchedFHEPSIServer.cpp:75-90
    {
        const auto begin = std::chrono::steady_clock::now();
        // nested hashing (HierarchicalCuckooHashTable::insertAll) + the operator's constructor, on the device
        PieContext::check(piehip_build_db(cc->handle(), serverSet.data(), serverSet.size(), ht.numberOfSimpleHashFunctions,
                                          ht.eachSimpleTableSize, ht.numberOfCuckooHashFunctions, ht.maxItemsPerPosition,
                                          ht.eachCuckooTableSize, hashSeed, evictSeed, shuffleSeed, maskSeed));
        PieContext::check(piehip_sync(cc->handle()));
        // One evaluation of an all-zero batch while nobody waits for it: the first launch of every kernel loads its code object
        // and the first run creates the queues -- milliseconds that would otherwise land in the first client's online phase.
        {
            const uint32_t L = cc->towers(), N = cc->ringDimension(), K = ht.numberOfCuckooHashFunctions, E = ht.eachCuckooTableSize;
            const size_t ct = 2 * (size_t)L * N;
            uint64_t *pinRes = nullptr;
            for (uint32_t q = 0; q < fds.size(); q++) {
                uint64_t *pinIdx = nullptr, *pinMinus = nullptr;
                PieContext::check(piehip_host_buffers_q(cc->handle(), q, &pinIdx, &pinMinus, &pinRes));
                zeroQuery(pinIdx, pinMinus, K, E, ct);
                PieContext::check(piehip_stage_minus_q(cc->handle(), q, pinMinus));
                for (uint32_t h = 0; h < K; h++) PieContext::check(piehip_stage_index_row_q(cc->handle(), q, h, pinIdx + (size_t)h * E * ct));
            }
            PieContext::check(piehip_run_staged(cc->handle(), pinRes));
            PieContext::check(piehip_run_host_wait(cc->handle()));
        }
        offlineComputation = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begin).count();
    }

    void runOnlinePhase()  // BatchedFHEPSIServer.cpp:92-112
    {
        const uint32_t L = cc->towers(), N = cc->ringDimension(), K = ht.numberOfCuckooHashFunctions, E = ht.eachCuckooTableSize,
                       b = tiledLayers(), nq = (uint32_t)fds.size();
        // Every message is unpacked (and range-checked) straight into the library's page-locked staging arrays, and a piece's
        // upload starts as soon as it has landed: every message's ciphertext at once -- the 29 MiB of a C3 query cross PCIe
        // underneath the receive loop, and when the timer starts only the last megabyte is still on its way (the reference deserialises into
        // Ciphertext objects in the same place, .cpp:114-141, before its timer starts at .cpp:98).  A failed receive drops the
        // partial staging (piehip_stage_reset) before the exception leaves.
        uint64_t *pinRes = nullptr;
        try {
            for (uint32_t q = 0; q < nq; q++) {
                uint64_t *pinIdx = nullptr, *pinMinus = nullptr;
                PieContext::check(piehip_host_buffers_q(cc->handle(), q, &pinIdx, &pinMinus, &pinRes));
                receiveQuery(fds[q], L, N, K, E, qMod.data(), pinIdx, pinMinus, stagePieces(cc->handle(), q));
            }
        } catch (...) {
            piehip_stage_reset(cc->handle());
            throw;
        }
        const auto begin = std::chrono::steady_clock::now();
        // setMinusCompareElement / setIndex / run (.cpp:101-103) on the staged queries; the result lists are in host memory at the end
        PieContext::check(piehip_run_staged(cc->handle(), pinRes));
        PieContext::check(piehip_run_host_wait(cc->handle()));
        onlineComputation = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begin).count();
        // components and limbs of a result ciphertext as it leaves the device and the server: what the handle says they are
        uint32_t ncomp = 0, keep = 0, lc = 0;
        PieContext::check(piehip_get_result_components(cc->handle(), &ncomp));
        PieContext::check(piehip_get_result_limbs(cc->handle(), &keep));
        PieContext::check(piehip_get_chain_limbs(cc->handle(), &lc));
        if (K >= 2 && lc < keep) keep = lc;
        const size_t rct = (size_t)ncomp * keep * N;
        for (uint32_t q = 0; q < nq; q++) sendResults(fds[q], pinRes + q * rct, b, nq * rct, keep, N, ncomp);   // rows are [bin layer][query]
    }

private:
    std::vector<int> fds;   // one channel per client of the batch
    std::vector<uint64_t> serverSet;
    HashTableParameter ht;
    uint64_t hashSeed;
    uint64_t evictSeed = 0, shuffleSeed = 0, maskSeed = 0;
    uint32_t resultLimbs = 0;   // setResultLimbs: 0 = every limb
    uint32_t chainLimbs = 0;    // the constructor's option: 0 = every limb
    bool layerTiling = false;   // setLayerTiling
    bool resultRelin = true;    // setResultRelin
    uint32_t tiled = 0;         // result messages per client with a layer tiling (0: no tiling)
    std::vector<uint64_t> qMod;
    std::unique_ptr<PieContext> cc;
};

}  // namespace piehip
