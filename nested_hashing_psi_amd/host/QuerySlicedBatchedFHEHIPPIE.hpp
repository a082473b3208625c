// QuerySlicedBatchedFHEHIPPIE.hpp -- the reference operator's shape over G handles of ONE process with stage A sharded by what the
// QUERY is made of (include/piehip.h "Query slices").
//
// ShardedBatchedFHEHIPPIE.hpp shards by bin layer and therefore uploads every query to every device.  Here a unit u = h L + l is limb
// l of inner hash function h, and handle g of G -- one per device, or several on one device -- holds
//   query slice g   the units piehip_query_slice gives rank g: those limbs of the packed database for ALL bin layers, and of every
//                   query only those limbs -- u_n / (K L) of it;
//   bin slice g     the bin layers [b g / G, b (g + 1) / G): their masks, the product chain's workspace, the EvalMult key.
// run() (BatchedFHEHIPPIE.cpp:88-129) is piehip_run_slice on every handle (:96-116), the G x G placements
// (piehip_put_accumulators_from: each handle takes the rows of its bin layers from every handle's accumulator limbs, on one device
// or across devices with peer access), piehip_run_chain on every handle (:117-126), and the result list in bin order.  Same methods,
// call order and exceptions as BatchedFHEHIPPIE.hpp, plus the batch forms of BatchedFHEHIPPIEQueryBatch (query index first); one host
// thread drives all handles.  Either slice of a handle may be empty (G > K L, G > b).
#pragma once
#include "BatchedFHEHIPPIE.hpp"

namespace piehip {

class QuerySlicedBatchedFHEHIPPIE {
public:
    using Seeds = BatchedFHEHIPPIE::Seeds;
    struct Slice {
        uint32_t lo, hi;
    };

    // contexts: the G handles (same ring, moduli and plaintext modulus; each with bin layers must hold the EvalMult key(s))
    QuerySlicedBatchedFHEHIPPIE(const std::vector<PieContext *> &contexts, const HashTableView &hct, uint32_t queriesPerRun = 1)
        : QuerySlicedBatchedFHEHIPPIE(contexts, hct, Seeds::fromRandomDevice(), queriesPerRun)
    {
    }
    // test-only: reproducible shuffle and masks
    QuerySlicedBatchedFHEHIPPIE(const std::vector<PieContext *> &contexts, const HashTableView &hct, const Seeds &seeds,
                                uint32_t queriesPerRun = 1)
        : ccs(contexts), nq(queriesPerRun)
    {
        if (ccs.empty()) throw std::invalid_argument("at least one context");
        if (hct.serverStashSize != 0) throw std::invalid_argument("Error, batched FHE PIE does not support a stash (yet).");
        if (!hct.simpleMultiTables || !hct.cuckooMultiTables)
            throw std::invalid_argument("Error, batched FHE PIE currently does not support combined tables.");
        for (PieContext *c : ccs)
            if (c->ringDimension() != ccs[0]->ringDimension() || c->towers() != ccs[0]->towers() ||
                c->GetPlaintextModulus() != ccs[0]->GetPlaintextModulus())
                throw std::invalid_argument("contexts of a query-sliced operator must share their parameters");
        K = hct.numberOfCuckooTables;
        b = hct.eachBinSize;
        E = hct.eachCuckooTableSize;
        const uint32_t k = hct.numberOfSimpleTables, e = hct.eachSimpleTableSize, L = ccs[0]->towers();
        const int G = (int)ccs.size();
        for (int g = 0; g < G; g++) {
            Slice u, s;
            PieContext::check(piehip_query_slice(K, L, G, g, &u.lo, &u.hi));
            PieContext::check(piehip_rccl_bin_slice(b, G, g, &s.lo, &s.hi));
            PieContext::check(piehip_set_query_batch(ccs[g]->handle(), nq));
            // every handle shuffles the whole table with the same seed and keeps its units of it
            PieContext::check(piehip_load_db_table_sliced(ccs[g]->handle(), hct.table, k, e, K, b, E, seeds.shuffle, seeds.mask, u.lo, u.hi,
                                                          s.lo, s.hi));
            units.push_back(u);
            bins.push_back(s);
        }
        uploaded.assign(G, 0);
        idxBytes.assign(G, 0);
        minusBytes.assign(G, 0);
        lists.assign(nq, std::vector<LimbCt>(b));
    }

    // setIndex (.hpp:40-43): the whole matrix in host memory; handle g is sent its units only -- one strided copy per unit
    void setIndex(std::vector<std::vector<LimbCt>> &&indexMatrix) { setIndex(0, std::move(indexMatrix)); }
    void setIndex(uint32_t q, std::vector<std::vector<LimbCt>> &&indexMatrix)
    {
        const size_t ct = ctWords();
        if (indexMatrix.size() != K) throw std::invalid_argument("index matrix must have one row per inner hash function");
        flat.resize((size_t)K * E * ct);
        for (uint32_t h = 0; h < K; h++) {
            if (indexMatrix[h].size() != E) throw std::invalid_argument("index matrix row length must be eachCuckooTableSize");
            for (uint32_t j = 0; j < E; j++) {
                if (indexMatrix[h][j].limbs.size() != ct) throw std::invalid_argument("ciphertext does not match the context");
                std::memcpy(flat.data() + ((size_t)h * E + j) * ct, indexMatrix[h][j].limbs.data(), ct * sizeof(uint64_t));
            }
        }
        for (size_t g = 0; g < ccs.size(); g++) {
            PieContext::check(piehip_set_index_slice_from_q(ccs[g]->handle(), q, flat.data()));
            idxBytes[g] = (size_t)(units[g].hi - units[g].lo) * E * 2 * ccs[0]->ringDimension() * sizeof(uint64_t);
            uploaded[g] = idxBytes[g] + minusBytes[g];
        }
    }
    // setMinusCompareElement (.hpp:45-48)
    void setMinusCompareElement(LimbCt minusCompareElement) { setMinusCompareElement(0, minusCompareElement); }
    void setMinusCompareElement(uint32_t q, const LimbCt &minusCompareElement)
    {
        if (minusCompareElement.limbs.size() != ctWords()) throw std::invalid_argument("ciphertext does not match the context");
        for (size_t g = 0; g < ccs.size(); g++) {
            PieContext::check(piehip_set_minus_slice_from_q(ccs[g]->handle(), q, minusCompareElement.limbs.data()));
            minusBytes[g] = (size_t)(units[g].hi - units[g].lo) * 2 * ccs[0]->ringDimension() * sizeof(uint64_t);
            uploaded[g] = idxBytes[g] + minusBytes[g];
        }
    }
    // seeded queries (include/piehip.h "Seeded ciphertexts"): c0Index[K][E][L][N] + seeds[K][E][32], c0[L][N] + seed[32] in host memory.
    // Handle g is sent the c0 limbs of its units -- one strided copy per unit -- and expands the c1 limbs itself at run()
    void setIndexSeeded(const uint64_t *c0Index, const uint8_t *seeds) { setIndexSeeded(0, c0Index, seeds); }
    void setIndexSeeded(uint32_t q, const uint64_t *c0Index, const uint8_t *seeds)
    {
        for (size_t g = 0; g < ccs.size(); g++) {
            PieContext::check(piehip_set_index_slice_seeded_from_q(ccs[g]->handle(), q, c0Index, seeds));
            const size_t un = units[g].hi - units[g].lo;
            idxBytes[g] = un * E * ccs[0]->ringDimension() * sizeof(uint64_t) + (un ? (size_t)K * E * 32 : 0);
            uploaded[g] = idxBytes[g] + minusBytes[g];
        }
    }
    void setMinusCompareElementSeeded(const uint64_t *c0, const uint8_t *seed) { setMinusCompareElementSeeded(0, c0, seed); }
    void setMinusCompareElementSeeded(uint32_t q, const uint64_t *c0, const uint8_t *seed)
    {
        for (size_t g = 0; g < ccs.size(); g++) {
            PieContext::check(piehip_set_minus_slice_seeded_from_q(ccs[g]->handle(), q, c0, seed));
            const size_t un = units[g].hi - units[g].lo;
            minusBytes[g] = un * ccs[0]->ringDimension() * sizeof(uint64_t) + (un ? 32 : 0);
            uploaded[g] = idxBytes[g] + minusBytes[g];
        }
    }
    // the EvalMult key of query q's client on every handle that runs a chain
    void setEvalMultKey(uint32_t q, const uint64_t *evk)
    {
        for (PieContext *c : ccs) PieContext::check(piehip_load_relin_key_q(c->handle(), q, evk));
    }

    void run()  // BatchedFHEHIPPIE.cpp:88-129
    {
        for (PieContext *c : ccs) PieContext::check(piehip_run_slice(c->handle()));                       // :96-116, every device busy
        for (PieContext *d : ccs)
            for (PieContext *s : ccs) PieContext::check(piehip_put_accumulators_from(d->handle(), s->handle()));
        for (PieContext *c : ccs) PieContext::check(piehip_run_chain(c->handle()));                       // :117-126
        uint32_t keep = 0;
        PieContext::check(piehip_get_result_limbs(ccs[0]->handle(), &keep));
        const size_t ct = 2 * (size_t)keep * ccs[0]->ringDimension();
        for (size_t g = 0; g < ccs.size(); g++) {
            const uint32_t n = bins[g].hi - bins[g].lo;
            if (!n) continue;
            rows.resize((size_t)n * nq * ct);
            PieContext::check(piehip_get_results(ccs[g]->handle(), rows.data()));   // rows [bin layer][query]
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t q = 0; q < nq; q++) {
                    const uint64_t *src = rows.data() + ((size_t)i * nq + q) * ct;
                    lists[q][bins[g].lo + i].limbs.assign(src, src + ct);
                }
        }
    }

    std::vector<LimbCt> &getResultList() { return lists[0]; }   // .hpp:35-38, bin order
    std::vector<LimbCt> &getResultList(uint32_t q)
    {
        if (q >= nq) throw std::invalid_argument("query index outside the batch");
        return lists[q];
    }

    void setResultLimbs(uint32_t keep)
    {
        for (PieContext *c : ccs) PieContext::check(piehip_set_result_limbs(c->handle(), keep));
    }

    const std::vector<Slice> &unitSlices() const { return units; }
    const std::vector<Slice> &binSlices() const { return bins; }
    // bytes that went up to handle g for the last query set (index matrix + minus element): u_n / (K L) of the matrix, and per unit its limb of the minus element.
    // Seeded inputs: the c0 rows only, u_n (E + 1) N 8 bytes, plus the seed tables a handle with units is handed whole (32 K E and 32 bytes)
    size_t uploadedBytes(size_t g) const { return uploaded.at(g); }
    uint32_t queriesPerRun() const { return nq; }

private:
    size_t ctWords() const { return 2 * (size_t)ccs[0]->towers() * ccs[0]->ringDimension(); }
    std::vector<PieContext *> ccs;
    std::vector<Slice> units, bins;
    uint32_t K = 0, b = 0, E = 0, nq = 1;
    std::vector<uint64_t> flat, rows;
    std::vector<size_t> uploaded, idxBytes, minusBytes;
    std::vector<std::vector<LimbCt>> lists;
};

}  // namespace piehip
