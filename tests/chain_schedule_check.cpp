// Chain schedule through the C++ host facade (run by tests/test_gpu_chain_schedule_cpp.py):
//   chain_schedule_check <dir>
// BatchedFHEHIPPIE / BatchedFHEHIPPIEQueryBatch::setChainSchedule on a tiny table with three inner hash functions at N = 4096, L = 3
// (fixed seeds, deterministic inputs and key; chain_limbs_check.cpp's towers): the schedule (3,2) against the vectors the Python side
// computed from the exact definition and wrote to <dir>/want.bin -- [query 0 | query 1][b][2][2][N] -- and against a second handle set
// through the C ABI; row sizes follow the last product's level; the refusals keep the library's exception types.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../nested_hashing_psi_amd/host/BatchedFHEHIPPIE.hpp"

using namespace piehip;

static std::vector<uint64_t> towers(size_t n, uint64_t seed)
{
    std::vector<uint64_t> v(n);
    for (size_t w = 0; w < n; w++) v[w] = ((uint64_t)(w + 1) * 2654435761ULL + seed * 40503ULL) % 65521ULL;
    return v;
}

static int facade(const std::string &dir)
{
    const uint32_t N = 4096, L = 3, K = 3, E = 2, b = 2, last = 2;
    const std::vector<uint32_t> sched = {3, 2};
    const size_t ct = 2 * (size_t)L * N, rct = 2 * (size_t)last * N;
    std::vector<uint64_t> want(2 * b * rct);
    FILE *f = std::fopen((dir + "/want.bin").c_str(), "rb");
    if (!f) return 10;
    const size_t got = std::fread(want.data(), sizeof(uint64_t), want.size(), f);
    std::fclose(f);
    if (got != want.size()) return 11;
    HashTableView v;
    v.numberOfSimpleTables = 2, v.eachSimpleTableSize = 2, v.numberOfCuckooTables = K, v.eachBinSize = b, v.eachCuckooTableSize = E;
    std::vector<uint64_t> tbl(2 * 2 * K * b * E, 0);
    for (size_t i = 0; i < tbl.size(); i++) tbl[i] = (i * 7919u) % 65536u + 1;
    v.table = tbl.data();
    PieContext cc(N, L, 65537);
    const std::vector<uint64_t> evk = towers((size_t)L * 2 * L * N, 21);
    cc.setEvalMultKey(evk.data());
    BatchedFHEHIPPIE pie(cc, v, BatchedFHEHIPPIE::Seeds{6, 7});
    auto matrix = [&](uint64_t base) {
        std::vector<std::vector<LimbCt>> m(K, std::vector<LimbCt>(E));
        for (uint32_t h = 0; h < K; h++)
            for (uint32_t j = 0; j < E; j++) m[h][j].limbs = towers(ct, base + h + K * j);
        return m;
    };
    LimbCt minus, minus1;
    minus.limbs = towers(ct, 3);
    minus1.limbs = towers(ct, 4);
    if (pie.chainSchedule() != std::vector<uint32_t>{L} || pie.chainLimbs() != L) return 20;
    // the refusals keep the library's exception types and leave the setting alone
    try {
        pie.setChainSchedule({2, 3});
        return 21;
    } catch (const std::invalid_argument &) {
    }
    try {
        pie.setChainSchedule({});
        return 22;
    } catch (const std::invalid_argument &) {
    }
    if (pie.chainSchedule() != std::vector<uint32_t>{L}) return 23;
    pie.setChainSchedule(sched);
    if (pie.chainSchedule() != sched || pie.chainLimbs() != last) return 24;
    pie.setMinusCompareElement(minus);
    pie.setIndex(matrix(5));
    pie.run();
    if (pie.getResultList().size() != b) return 25;
    for (uint32_t i = 0; i < b; i++) {
        const LimbCt &c = pie.getResultList()[i];
        if (c.limbs.size() != rct) return 26;   // rows of the last product's level
        for (size_t w = 0; w < rct; w++) {
            if (pie.resultTowers(i)[w] != c.limbs[w]) return 27;
            if (c.limbs[w] != want[i * rct + w]) return 28;
        }
    }
    // the same rows from a slot whose handle was set through the C ABI (a slot has its own schedule: the owner's does not reach it)
    PieContext cc3(N, L, 65537);
    BatchedFHEHIPPIE slot(cc3, pie);
    if (slot.chainLimbs() != L) return 40;
    PieContext::check(piehip_set_chain_schedule(cc3.handle(), sched.data(), (uint32_t)sched.size()));
    uint32_t l_last = 0;
    PieContext::check(piehip_get_chain_limbs(cc3.handle(), &l_last));
    if (l_last != last) return 41;
    std::vector<uint64_t> idx, mn = minus.limbs;
    for (auto &row : matrix(5))
        for (auto &c : row) idx.insert(idx.end(), c.limbs.begin(), c.limbs.end());
    PieContext::check(piehip_set_minus(cc3.handle(), mn.data()));
    PieContext::check(piehip_set_index(cc3.handle(), idx.data()));
    PieContext::check(piehip_run(cc3.handle()));
    std::vector<uint64_t> rows((size_t)b * rct);
    PieContext::check(piehip_get_results(cc3.handle(), rows.data()));
    for (uint32_t i = 0; i < b; i++)
        for (size_t w = 0; w < rct; w++)
            if (rows[i * rct + w] != pie.getResultList()[i].limbs[w]) return 42;
    // a batch of two on the same database and key, with its own schedule; query 0 is the query above
    PieContext cc2(N, L, 65537);
    BatchedFHEHIPPIEQueryBatch batch(cc2, pie, 2);
    if (batch.chainLimbs() != L) return 31;
    batch.setChainSchedule(sched);
    if (batch.chainSchedule() != sched || batch.chainLimbs() != last) return 32;
    batch.setMinusCompareElement(0, minus);
    batch.setIndex(0, matrix(5));
    batch.setMinusCompareElement(1, minus1);
    batch.setIndex(1, matrix(12));
    batch.run();
    for (uint32_t q = 0; q < 2; q++)
        for (uint32_t i = 0; i < b; i++) {
            const LimbCt &c = batch.getResultList(q)[i];
            if (c.limbs.size() != rct) return 33;
            for (size_t w = 0; w < rct; w++)
                if (c.limbs[w] != want[((size_t)q * b + i) * rct + w]) return 34 + (int)q;
        }
    // back to one level for every product: rows of that level
    pie.setChainLimbs(L);
    if (pie.chainSchedule() != std::vector<uint32_t>{L}) return 36;
    pie.setMinusCompareElement(minus);
    pie.setIndex(matrix(5));
    pie.run();
    if (pie.getResultList()[0].limbs.size() != ct) return 37;
    std::printf("facade ok: %u + %u + 2 x %u result ciphertexts from the schedule (3,2) on %u limbs\n", b, b, b, L);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    try {
        return facade(argv[1]);
    } catch (const std::invalid_argument &e) {
        std::printf("refused: %s\n", e.what());
        return 3;
    } catch (const std::runtime_error &e) {
        std::printf("no device: %s\n", e.what());
        return 77;
    }
}
