// host/QuerySlicedBatchedFHEHIPPIE.hpp over four handles on one device (run by tests/test_gpu_query_slices_cpp.py on the GPU box): at
// N = 4096, K = 2, L = 2 -- one unit per handle -- a batch of two queries gives, bit for bit, the result lists of the unsliced C++ facade
// (BatchedFHEHIPPIE + BatchedFHEHIPPIEQueryBatch) on the same table and seeds, over two rounds with different queries; every handle was
// sent its unit of each query only: a quarter of the index matrix and one limb of the minus element.  Exit code 0 = ok, 77 = no GPU.
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

static void fill_ct(std::vector<uint64_t> &v, const std::vector<uint64_t> &mod, uint32_t L, uint32_t N, uint64_t &seed)
{
    v.resize(2 * (size_t)L * N);
    for (uint32_t c = 0; c < 2; c++)
        for (uint32_t i = 0; i < L; i++)
            for (uint32_t j = 0; j < N; j++) v[((size_t)c * L + i) * N + j] = mix(seed) % mod[i];
}

int main()
{
    const uint32_t N = 4096, L = 2, K = 2, E = 3, b = 5, nq = 2, G = 4;
    try {
        HashTableView v;
        v.numberOfSimpleTables = 2, v.eachSimpleTableSize = 5, v.numberOfCuckooTables = K, v.eachBinSize = b, v.eachCuckooTableSize = E;
        std::vector<uint64_t> tbl((size_t)2 * 5 * K * b * E);
        for (size_t i = 0; i < tbl.size(); i++) tbl[i] = (i * 7919u) % 65000u + 1;
        v.table = tbl.data();
        const BatchedFHEHIPPIE::Seeds seeds{11, 22};

        PieContext base(N, L, 65537), slot(N, L, 65537);
        std::vector<uint64_t> mod(2 * L + 2);
        PieContext::check(piehip_get_moduli(base.handle(), mod.data()));
        std::vector<uint64_t> evk((size_t)L * 2 * L * N);
        uint64_t ks = 1;
        for (size_t i = 0; i < evk.size(); i++) evk[i] = mix(ks) % mod[(i / N) % L];
        base.setEvalMultKey(evk.data());
        BatchedFHEHIPPIE database(base, v, seeds);
        BatchedFHEHIPPIEQueryBatch whole(slot, database, nq);

        std::vector<PieContext *> ccs;
        for (uint32_t g = 0; g < G; g++) {
            ccs.push_back(new PieContext(N, L, 65537));
            ccs.back()->setEvalMultKey(evk.data());
        }
        int rc = 0;
        {
            QuerySlicedBatchedFHEHIPPIE sliced(ccs, v, seeds, nq);
            for (uint32_t g = 0; g < G && !rc; g++)
                if (sliced.unitSlices()[g].hi - sliced.unitSlices()[g].lo != 1) rc = 3;
            for (uint64_t round = 0; round < 2 && !rc; round++) {
                for (uint32_t q = 0; q < nq; q++) {
                    uint64_t seed = 100 + 10 * round + q;
                    LimbCt minus;
                    fill_ct(minus.limbs, mod, L, N, seed);
                    std::vector<std::vector<LimbCt>> idx(K, std::vector<LimbCt>(E));
                    for (auto &row : idx)
                        for (auto &c : row) fill_ct(c.limbs, mod, L, N, seed);
                    auto idx2 = idx;
                    sliced.setMinusCompareElement(q, minus);
                    sliced.setIndex(q, std::move(idx));
                    whole.setMinusCompareElement(q, minus);
                    whole.setIndex(q, std::move(idx2));
                }
                // one unit per handle: 1 / (K L) of the index matrix and limb l of the minus element (1 / L of it)
                const size_t index_bytes = (size_t)K * E * 2 * L * N * sizeof(uint64_t), minus_bytes = 2 * (size_t)L * N * sizeof(uint64_t);
                for (uint32_t g = 0; g < G; g++)
                    if (sliced.uploadedBytes(g) != index_bytes / (K * L) + minus_bytes / L) rc = 4;
                sliced.run();
                whole.run();
                for (uint32_t q = 0; q < nq && !rc; q++) {
                    auto &got = sliced.getResultList(q);
                    auto &want = whole.getResultList(q);
                    if (got.size() != b || want.size() != b) rc = 5;
                    for (uint32_t i = 0; i < b && !rc; i++)
                        if (got[i].limbs != want[i].limbs) {
                            std::printf("round %llu query %u bin layer %u differs\n", (unsigned long long)round, q, i);
                            rc = 6;
                        }
                }
                if (round == 1 && !rc && sliced.getResultList(0)[0].limbs == sliced.getResultList(1)[0].limbs) rc = 7;  // the queries differ
            }
        }
        for (PieContext *c : ccs) delete c;
        if (!rc) std::printf("query slices check ok: %u handles, %u queries per run, %u result ciphertexts each\n", G, nq, b);
        else std::printf("query slices check failed: %d\n", rc);
        return rc;
    } catch (const std::runtime_error &e) {
        std::printf("no device or refused: %s\n", e.what());
        return 77;
    }
}
