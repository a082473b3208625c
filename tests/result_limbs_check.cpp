// Result limbs through the C++ host facade and the server (run by tests/test_gpu_result_limbs_cpp.py):
//   result_limbs_check <keep>
// Part 1: BatchedFHEHIPPIE / BatchedFHEHIPPIEQueryBatch::setResultLimbs on facade_check.cpp's tiny table (N = 1024, L = 2, fixed
// seeds, deterministic inputs): prints a digest of the result lists, which the Python side computes from the exact definition.
// Part 2: host/BatchedFHEPSIServer.hpp with setResultLimbs(keep) against an in-process client over a socket pair: every framed
// result message carries `keep` limbs.
#include <sys/socket.h>

#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../nested_hashing_psi_amd/host/BatchedFHEPSIServer.hpp"

using namespace piehip;

static uint64_t fnv(uint64_t h, const uint64_t *w, size_t n)
{
    for (size_t i = 0; i < n; i++) h = (h ^ w[i]) * 0x100000001B3ULL;
    return h;
}
static const uint64_t FNV0 = 0xCBF29CE484222325ULL;
// deterministic, non-constant canonical towers (every value below 2^16, every modulus above it); the Python side has the same formula
static std::vector<uint64_t> towers(size_t n, uint64_t seed)
{
    std::vector<uint64_t> v(n);
    for (size_t w = 0; w < n; w++) v[w] = ((uint64_t)(w + 1) * 2654435761ULL + seed * 40503ULL) % 65521ULL;
    return v;
}

static int facade(uint32_t keep)
{
    const uint32_t N = 1024, L = 2;
    HashTableView v;
    v.numberOfSimpleTables = 2, v.eachSimpleTableSize = 2, v.numberOfCuckooTables = 2, v.eachBinSize = 2, v.eachCuckooTableSize = 3;
    std::vector<uint64_t> tbl(2 * 2 * 2 * 2 * 3, 0);
    for (size_t i = 0; i < tbl.size(); i++) tbl[i] = (i * 7919u) % 65536u + 1;
    v.table = tbl.data();
    PieContext cc(N, L, 65537);
    BatchedFHEHIPPIE pie(cc, v, BatchedFHEHIPPIE::Seeds{6, 7});
    const size_t ct = 2 * (size_t)L * N, rct = 2 * (size_t)keep * N;
    const std::vector<uint64_t> evk = towers((size_t)L * 2 * L * N, 1);
    cc.setEvalMultKey(evk.data());
    auto matrix = [&](uint64_t base) {
        std::vector<std::vector<LimbCt>> m(2, std::vector<LimbCt>(3));
        for (uint32_t h = 0; h < 2; h++)
            for (uint32_t j = 0; j < 3; j++) m[h][j].limbs = towers(ct, base + h + 2 * j);
        return m;
    };
    LimbCt minus;
    minus.limbs = towers(ct, 3);
    if (pie.resultLimbs() != L) return 20;
    pie.setMinusCompareElement(minus);
    pie.setIndex(matrix(5));
    pie.run();
    const std::vector<LimbCt> full = pie.getResultList();
    uint64_t dfull = FNV0;
    for (const auto &c : full) {
        if (c.limbs.size() != ct) return 21;
        dfull = fnv(dfull, c.limbs.data(), ct);
    }
    pie.setResultLimbs(keep);
    if (pie.resultLimbs() != keep) return 22;
    pie.run();   // nothing set since: the same query again, reduced
    if (pie.getResultList()[0].limbs == pie.getResultList()[1].limbs) return 29;   // a degenerate query would prove nothing
    uint64_t dkeep = FNV0;
    for (size_t i = 0; i < pie.getResultList().size(); i++) {
        const LimbCt &c = pie.getResultList()[i];
        if (c.limbs.size() != rct) return 23;
        for (size_t w = 0; w < rct; w++)
            if (pie.resultTowers((uint32_t)i)[w] != c.limbs[w]) return 24;
        dkeep = fnv(dkeep, c.limbs.data(), rct);
    }
    // a batch of two queries on the same database with its own setting; query 0 is the query above
    PieContext cc2(N, L, 65537);
    BatchedFHEHIPPIEQueryBatch batch(cc2, pie, 2);
    batch.setResultLimbs(keep);
    LimbCt minus1;
    minus1.limbs = towers(ct, 4);
    batch.setMinusCompareElement(0, minus);
    batch.setIndex(0, matrix(5));
    batch.setMinusCompareElement(1, minus1);
    batch.setIndex(1, matrix(12));
    batch.run();
    uint64_t dq1 = FNV0;
    for (size_t i = 0; i < full.size(); i++) {
        if (batch.getResultList(0)[i].limbs != pie.getResultList()[i].limbs) return 25;
        if (batch.getResultList(1)[i].limbs.size() != rct) return 26;
        dq1 = fnv(dq1, batch.getResultList(1)[i].limbs.data(), rct);
    }
    bool threw = false;
    try {
        pie.setResultLimbs(L + 1);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw || pie.resultLimbs() != keep) return 27;
    pie.setResultLimbs(L);   // back: the full result list, bit for bit
    pie.run();
    for (size_t i = 0; i < full.size(); i++)
        if (pie.getResultList()[i].limbs != full[i].limbs) return 28;
    std::printf("facade full %016llx keep %016llx batch1 %016llx\n", (unsigned long long)dfull, (unsigned long long)dkeep,
                (unsigned long long)dq1);
    return 0;
}

// the client of BatchedFHEPSIServer's three phases, with constant (canonical) towers: only the framing is looked at
static void client(int fd, uint32_t N, uint32_t L, uint32_t K, uint32_t E, uint32_t b, uint32_t keep, int *verdict)
{
    *verdict = 1;
    try {
        ContextMessage c = {};
        c.N = N, c.L = L, c.t = 65537;
        if (piehip_default_moduli(N, L, c.moduli, c.moduli + L)) return;
        wire::writeWithSize(fd, &c, sizeof(c));
        wire::writeWithSize(fd, "public key", 10);
        std::vector<uint64_t> evk((size_t)L * 2 * L * N, 1);
        wire::writeWithSize(fd, evk.data(), evk.size() * sizeof(uint64_t));
        wire::waitForPhaseOver(fd);
        wire::waitForPhaseOver(fd);
        std::vector<uint64_t> one(2 * (size_t)L * N, 3);
        const auto m = wire::packCiphertexts(one.data(), 1, L, N);
        for (uint32_t i = 0; i < 1 + K * E; i++) wire::writeWithSize(fd, m.data(), m.size());
        std::vector<uint8_t> r;
        std::vector<uint64_t> towers;
        for (uint32_t i = 0; i < b; i++) {
            wire::readWithSizeIntoVector(fd, r);
            if (r.size() != sizeof(wire::LimbHeader) + 2 * (size_t)keep * N * sizeof(uint64_t)) return;
            if (wire::unpackCiphertexts(r, keep, N, towers, c.moduli) != 1) return;   // header says `keep` limbs; residues below q[:keep]
        }
        *verdict = 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "client: %s\n", e.what());
    }
}

static int server(uint32_t keep)
{
    const uint32_t N = 1024, L = 2, k = 2, e = 3, K = 3, E = 5, b = 2;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv)) return 30;
    std::vector<uint64_t> set(40);
    for (size_t i = 0; i < set.size(); i++) set[i] = (i * 1237u) % 65536u + 1;
    int verdict = 1;
    std::thread cl(client, sv[1], N, L, K, E, b, keep, &verdict);
    int rc = 0;
    try {
        HashTableParameter ht;
        ht.numberOfSimpleHashFunctions = k, ht.eachSimpleTableSize = e, ht.numberOfCuckooHashFunctions = K, ht.eachCuckooTableSize = E;
        ht.maxItemsPerPosition = b;
        BatchedFHEPSIServer srv(sv[0], set, ht);
        srv.setSecretSeedsForTesting(1, 2, 3);
        srv.setResultLimbs(keep);
        srv.run();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "server: %s\n", e.what());
        rc = 31;
    }
    ::shutdown(sv[0], SHUT_RDWR);   // a client still waiting for a message ends
    cl.join();
    if (rc) return rc;
    if (verdict) return 32;
    std::printf("server ok: %u result messages of %u limb(s)\n", b, keep);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const uint32_t keep = (uint32_t)std::atoi(argv[1]);
    try {
        int rc = facade(keep);
        if (rc) return rc;
        return server(keep);
    } catch (const std::invalid_argument &e) {
        std::printf("refused: %s\n", e.what());
        return 3;
    } catch (const std::runtime_error &e) {
        std::printf("no device: %s\n", e.what());
        return 77;
    }
}
