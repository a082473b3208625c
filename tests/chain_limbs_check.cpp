// Chain limbs through the C++ host facade (run by tests/test_gpu_chain_limbs_cpp.py):
//   chain_limbs_check <dir>
// BatchedFHEHIPPIE / BatchedFHEHIPPIEQueryBatch::setChainLimbs on facade_check.cpp's tiny table at N = 4096, L = 3 (fixed seeds,
// deterministic inputs and key): row sizes, the refusals' exception types, and every word of the result lists against the vectors
// the Python side computed from the exact definition and wrote to <dir>/want.bin: [query 0 | query 1][b][2][Lc][N], Lc = 2, then
// query 0 at keep = 1: [b][2][1][N].
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../nested_hashing_psi_amd/host/BatchedFHEHIPPIE.hpp"

using namespace piehip;

// deterministic, non-constant canonical towers (every value below 2^16, every modulus above it); the Python side has the same formula
static std::vector<uint64_t> towers(size_t n, uint64_t seed)
{
    std::vector<uint64_t> v(n);
    for (size_t w = 0; w < n; w++) v[w] = ((uint64_t)(w + 1) * 2654435761ULL + seed * 40503ULL) % 65521ULL;
    return v;
}

static int facade(const std::string &dir)
{
    const uint32_t N = 4096, L = 3, Lc = 2, b = 2;
    const size_t ct = 2 * (size_t)L * N, rct = 2 * (size_t)Lc * N, r1 = 2 * (size_t)N;
    std::vector<uint64_t> want(2 * b * rct + b * r1);
    FILE *f = std::fopen((dir + "/want.bin").c_str(), "rb");
    if (!f) return 10;
    const size_t got = std::fread(want.data(), sizeof(uint64_t), want.size(), f);
    std::fclose(f);
    if (got != want.size()) return 11;
    HashTableView v;
    v.numberOfSimpleTables = 2, v.eachSimpleTableSize = 2, v.numberOfCuckooTables = 2, v.eachBinSize = b, v.eachCuckooTableSize = 3;
    std::vector<uint64_t> tbl(2 * 2 * 2 * 2 * 3, 0);
    for (size_t i = 0; i < tbl.size(); i++) tbl[i] = (i * 7919u) % 65536u + 1;
    v.table = tbl.data();
    PieContext cc(N, L, 65537);
    const std::vector<uint64_t> evk = towers((size_t)L * 2 * L * N, 21);
    cc.setEvalMultKey(evk.data());
    BatchedFHEHIPPIE pie(cc, v, BatchedFHEHIPPIE::Seeds{6, 7});
    auto matrix = [&](uint64_t base) {
        std::vector<std::vector<LimbCt>> m(2, std::vector<LimbCt>(3));
        for (uint32_t h = 0; h < 2; h++)
            for (uint32_t j = 0; j < 3; j++) m[h][j].limbs = towers(ct, base + h + 2 * j);
        return m;
    };
    LimbCt minus, minus1;
    minus.limbs = towers(ct, 3);
    minus1.limbs = towers(ct, 4);
    if (pie.chainLimbs() != L) return 20;
    // the refusals keep the library's exception types and leave the setting alone
    try {
        pie.setChainLimbs(0);
        return 21;
    } catch (const std::invalid_argument &) {
    }
    try {
        pie.setChainLimbs(L + 1);
        return 22;
    } catch (const std::invalid_argument &) {
    }
    if (pie.chainLimbs() != L) return 23;
    pie.setChainLimbs(Lc);
    if (pie.chainLimbs() != Lc) return 24;
    pie.setMinusCompareElement(minus);
    pie.setIndex(matrix(5));
    pie.run();
    if (pie.getResultList().size() != b) return 25;
    for (uint32_t i = 0; i < b; i++) {
        const LimbCt &c = pie.getResultList()[i];
        if (c.limbs.size() != rct) return 26;
        for (size_t w = 0; w < rct; w++) {
            if (pie.resultTowers(i)[w] != c.limbs[w]) return 27;
            if (c.limbs[w] != want[i * rct + w]) return 28;
        }
    }
    // keep = 1 below the level: the reduction inside the level context
    pie.setResultLimbs(1);
    pie.setMinusCompareElement(minus);
    pie.setIndex(matrix(5));
    pie.run();
    for (uint32_t i = 0; i < b; i++) {
        const LimbCt &c = pie.getResultList()[i];
        if (c.limbs.size() != r1) return 29;
        for (size_t w = 0; w < r1; w++)
            if (c.limbs[w] != want[2 * b * rct + i * r1 + w]) return 30;
    }
    pie.setResultLimbs(L);
    // a batch of two on the same database and key; a slot has its own setting; query 0 is the query above
    PieContext cc2(N, L, 65537);
    BatchedFHEHIPPIEQueryBatch batch(cc2, pie, 2);
    if (batch.chainLimbs() != L) return 31;
    batch.setChainLimbs(Lc);
    if (batch.chainLimbs() != Lc || pie.chainLimbs() != Lc) return 32;
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
    std::printf("facade ok: %u + %u + 2 x %u result ciphertexts from a chain on %u of %u limbs\n", b, b, b, Lc, L);
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
