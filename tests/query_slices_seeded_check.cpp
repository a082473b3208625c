// The seeded calls of host/QuerySlicedBatchedFHEHIPPIE.hpp over three handles on one device (run by
// tests/test_gpu_query_slices_seeded_cpp.py on the GPU box): at N = 4096, K = 2, L = 2 -- units split 1 + 1 + 2 -- a batch of two seeded
// queries gives, bit for bit, the result lists of the facade's unseeded calls on three more handles, fed with the same queries in full
// (c1 = piehip_expand_uniform of the seeds), over two rounds with different queries.  The seeded operator runs on handles that never
// held a full query; every handle was sent half the bytes plus the seed tables.  Exit code 0 = ok, 77 = no GPU.
#include <cstdio>
#include <vector>

#include "../nested_hashing_psi_amd/host/QuerySlicedBatchedFHEHIPPIE.hpp"

using namespace piehip;

static uint64_t mix(uint64_t &s)
{
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int main()
{
    const uint32_t N = 4096, L = 2, K = 2, E = 3, b = 5, nq = 2, G = 3;
    const size_t LN = (size_t)L * N, nct = (size_t)K * E + 1;   // the minus element is ciphertext K E
    try {
        HashTableView v;
        v.numberOfSimpleTables = 2, v.eachSimpleTableSize = 5, v.numberOfCuckooTables = K, v.eachBinSize = b, v.eachCuckooTableSize = E;
        std::vector<uint64_t> tbl((size_t)2 * 5 * K * b * E);
        for (size_t i = 0; i < tbl.size(); i++) tbl[i] = (i * 7919u) % 65000u + 1;
        v.table = tbl.data();
        const BatchedFHEHIPPIE::Seeds seeds{11, 22};

        std::vector<PieContext *> ccs, refs;
        std::vector<uint64_t> mod(2 * L + 2), evk((size_t)L * 2 * L * N);
        for (uint32_t g = 0; g < 2 * G; g++) {
            PieContext *c = new PieContext(N, L, 65537);
            if (!g) {
                PieContext::check(piehip_get_moduli(c->handle(), mod.data()));
                uint64_t ks = 1;
                for (size_t i = 0; i < evk.size(); i++) evk[i] = mix(ks) % mod[(i / N) % L];
            }
            c->setEvalMultKey(evk.data());
            (g < G ? ccs : refs).push_back(c);
        }
        int rc = 0;
        {
            QuerySlicedBatchedFHEHIPPIE seeded(ccs, v, seeds, nq), full(refs, v, seeds, nq);
            for (uint64_t round = 0; round < 2 && !rc; round++) {
                for (uint32_t q = 0; q < nq; q++) {
                    uint64_t s = 100 + 10 * round + q;
                    std::vector<uint64_t> c0(nct * LN), c1(nct * LN);
                    std::vector<uint8_t> sd(nct * 32);
                    for (size_t i = 0; i < c0.size(); i++) c0[i] = mix(s) % mod[(i / N) % L];
                    for (uint8_t &x : sd) x = (uint8_t)mix(s);
                    PieContext::check(piehip_expand_uniform(refs[0]->handle(), sd.data(), (uint32_t)nct, c1.data()));
                    std::vector<LimbCt> cts(nct);
                    for (size_t i = 0; i < nct; i++) {
                        cts[i].limbs.assign(c0.begin() + i * LN, c0.begin() + (i + 1) * LN);
                        cts[i].limbs.insert(cts[i].limbs.end(), c1.begin() + i * LN, c1.begin() + (i + 1) * LN);
                    }
                    std::vector<std::vector<LimbCt>> idx(K, std::vector<LimbCt>(E));
                    for (uint32_t h = 0; h < K; h++)
                        for (uint32_t j = 0; j < E; j++) idx[h][j] = cts[h * E + j];
                    seeded.setMinusCompareElementSeeded(q, c0.data() + (size_t)K * E * LN, sd.data() + (size_t)K * E * 32);
                    seeded.setIndexSeeded(q, c0.data(), sd.data());
                    full.setMinusCompareElement(q, cts[K * E]);
                    full.setIndex(q, std::move(idx));
                }
                // the c0 rows are half of the unseeded bytes; a handle with units is handed the seed tables whole
                for (uint32_t g = 0; g < G; g++) {
                    const size_t un = seeded.unitSlices()[g].hi - seeded.unitSlices()[g].lo;
                    if (un != (g < 2 ? 1u : 2u)) rc = 3;
                    if (full.uploadedBytes(g) != un * (E + 1) * 2 * N * sizeof(uint64_t)) rc = 4;
                    if (seeded.uploadedBytes(g) != full.uploadedBytes(g) / 2 + nct * 32) rc = 4;
                }
                seeded.run();
                full.run();
                for (uint32_t q = 0; q < nq && !rc; q++) {
                    auto &got = seeded.getResultList(q);
                    auto &want = full.getResultList(q);
                    if (got.size() != b || want.size() != b) rc = 5;
                    for (uint32_t i = 0; i < b && !rc; i++)
                        if (got[i].limbs != want[i].limbs) {
                            std::printf("round %llu query %u bin layer %u differs\n", (unsigned long long)round, q, i);
                            rc = 6;
                        }
                }
                if (round == 1 && !rc && seeded.getResultList(0)[0].limbs == seeded.getResultList(1)[0].limbs) rc = 7;  // the queries differ
            }
            // the same exception type as the unseeded calls for a query outside the batch
            try {
                seeded.setIndexSeeded(nq, evk.data(), (const uint8_t *)evk.data());
                rc = rc ? rc : 8;
            } catch (const std::invalid_argument &) {
            }
        }
        for (PieContext *c : ccs) delete c;
        for (PieContext *c : refs) delete c;
        if (!rc) std::printf("seeded query slices check ok: %u handles, %u queries per run, %u result ciphertexts each\n", G, nq, b);
        else std::printf("seeded query slices check failed: %d\n", rc);
        return rc;
    } catch (const std::runtime_error &e) {
        std::printf("no device or refused: %s\n", e.what());
        return 77;
    }
}
