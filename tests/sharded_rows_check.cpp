// host/ShardedBatchedFHEHIPPIE.hpp over three contexts on one device with the settings that change the shape of a result row, for
// tests/test_gpu_sharded_rows.py:   sharded_rows_check <dir>
// <dir> holds table.bin [k][e][K][b][E], evk.bin, idx.bin [K][E][2][L][N], minus.bin and want_<name>.bin, the result lists the wrapper
// computed from the definitions; every list this program gets is compared with one of them word for word.
//   1. three shards with the key: every setter alone (keep = 1; chain limbs 2; a schedule whose step lies behind the only product;
//      degree-2 rows), all together, and back to the default;
//   2. the roll-back: shard 2 replays a captured graph and so refuses every one of the settings -- the exception leaves, and shards 0
//      and 1 are as they were;
//   3. three shards and NO key anywhere: K = 2, setResultRelin(false);
//   4. layerTiling = 3: b = 7 -> three tiled layers, one per shard; alone and with keep = 1.
// Exit code 0 = ok.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../nested_hashing_psi_amd/host/ShardedBatchedFHEHIPPIE.hpp"

using namespace piehip;

static const uint32_t N = 4096, L = 3, k = 2, e = 5, K = 2, b = 7, E = 3;
static const uint64_t T = 65537;
static std::string dir;

static std::vector<uint64_t> slurp(const std::string &name)
{
    std::ifstream f(dir + "/" + name, std::ios::binary | std::ios::ate);
    if (!f) throw std::invalid_argument(name + ": missing");
    std::vector<uint64_t> v((size_t)f.tellg() / 8);
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * 8));
    return v;
}

static std::vector<uint64_t> g_idx, g_minus;
static std::vector<uint64_t> query(ShardedBatchedFHEHIPPIE &op)
{
    const size_t ct = 2 * (size_t)L * N;
    LimbCt minus;
    minus.limbs = g_minus;
    std::vector<std::vector<LimbCt>> idx(K, std::vector<LimbCt>(E));
    for (uint32_t h = 0; h < K; h++)
        for (uint32_t j = 0; j < E; j++) idx[h][j].limbs.assign(g_idx.begin() + ((size_t)h * E + j) * ct, g_idx.begin() + ((size_t)h * E + j + 1) * ct);
    op.setMinusCompareElement(minus);
    op.setIndex(std::move(idx));
    op.run();
    std::vector<uint64_t> out;
    for (auto &c : op.getResultList()) out.insert(out.end(), c.limbs.begin(), c.limbs.end());
    return out;
}

static int failures = 0;
static void expect_list(ShardedBatchedFHEHIPPIE &op, const char *want, uint32_t layers, uint32_t ncomp, uint32_t limbs)
{
    const std::vector<uint64_t> got = query(op), w = slurp(std::string("want_") + want + ".bin");
    const bool shape = op.getResultList().size() == layers && got.size() == (size_t)layers * ncomp * limbs * N && op.resultComponents() == ncomp &&
                       std::min(op.resultLimbs(), op.chainLimbs()) == limbs;
    if (!shape || got != w) {
        std::printf("%s: %s (%zu words, the definition has %zu)\n", want, shape ? "rows differ from the definition" : "wrong shape", got.size(), w.size());
        failures++;
    }
}
template <typename F>
static bool throws(F f)
{
    try {
        f();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    dir = argv[1];
    try {
        const std::vector<uint64_t> tbl = slurp("table.bin"), evk = slurp("evk.bin");
        g_idx = slurp("idx.bin"), g_minus = slurp("minus.bin");
        HashTableView v;
        v.numberOfSimpleTables = k, v.eachSimpleTableSize = e, v.numberOfCuckooTables = K, v.eachBinSize = b, v.eachCuckooTableSize = E;
        v.table = tbl.data();
        const BatchedFHEHIPPIE::Seeds seeds{11, 22};
        {   // 1.
            PieContext c0(N, L, T), c1(N, L, T), c2(N, L, T);
            for (PieContext *c : {&c0, &c1, &c2}) c->setEvalMultKey(evk.data());
            ShardedBatchedFHEHIPPIE sh({&c0, &c1, &c2}, v, seeds);
            if (sh.tiledLayers() != b || sh.binSlices().size() != 3) return std::printf("unexpected slices\n"), 1;
            expect_list(sh, "full", b, 2, L);
            sh.setResultLimbs(1);
            expect_list(sh, "keep1", b, 2, 1);
            sh.setResultLimbs(L);
            sh.setChainLimbs(2);
            expect_list(sh, "chain2", b, 2, 2);
            sh.setChainSchedule({L, 2});   // K = 2: one product, on L limbs; the step behind it changes nothing
            if (sh.chainSchedule() != std::vector<uint32_t>({L, 2})) return std::printf("chainSchedule()\n"), 1;
            expect_list(sh, "full", b, 2, L);
            sh.setChainLimbs(L);
            sh.setResultRelin(false);
            expect_list(sh, "deg2", b, 3, L);
            sh.setChainLimbs(2);
            sh.setResultLimbs(1);
            expect_list(sh, "all", b, 3, 1);
            sh.setResultRelin(true);
            sh.setResultLimbs(L);
            sh.setChainLimbs(L);
            expect_list(sh, "full", b, 2, L);
            // 2.
            PieContext::check(piehip_set_graph(c2.handle(), 1));
            const bool refused = throws([&] { sh.setResultLimbs(1); }) && throws([&] { sh.setChainLimbs(2); }) &&
                                 throws([&] { sh.setChainSchedule({L, 2, 1}); }) && throws([&] { sh.setResultRelin(false); });
            uint32_t keep[2] = {0, 0}, lc[2] = {0, 0}, nsched = 0, sched[7];
            int relin[2] = {0, 0};
            for (int g = 0; g < 2; g++) {
                PieContext *c = g ? &c1 : &c0;
                PieContext::check(piehip_get_result_limbs(c->handle(), &keep[g]));
                PieContext::check(piehip_get_chain_limbs(c->handle(), &lc[g]));
                PieContext::check(piehip_get_result_relin(c->handle(), &relin[g]));
                PieContext::check(piehip_get_chain_schedule(c->handle(), sched, 7, &nsched));
                if (nsched != 1 || sched[0] != L) {
                    std::printf("shard %d keeps the schedule of a refused call\n", g);
                    failures++;
                }
            }
            if (!refused || keep[0] != L || keep[1] != L || lc[0] != L || lc[1] != L || !relin[0] || !relin[1]) {
                std::printf("roll-back: refused %d, keep %u %u, chain limbs %u %u, relin %d %d\n", (int)refused, keep[0], keep[1], lc[0], lc[1], relin[0], relin[1]);
                failures++;
            }
            PieContext::check(piehip_set_graph(c2.handle(), 0));
            expect_list(sh, "full", b, 2, L);
        }
        {   // 3.
            PieContext c0(N, L, T), c1(N, L, T), c2(N, L, T);
            ShardedBatchedFHEHIPPIE sh({&c0, &c1, &c2}, v, seeds);
            sh.setResultRelin(false);
            expect_list(sh, "deg2", b, 3, L);
            sh.setResultLimbs(2);
            expect_list(sh, "deg2_keep2", b, 3, 2);
        }
        {   // 4.
            PieContext c0(N, L, T), c1(N, L, T), c2(N, L, T);
            for (PieContext *c : {&c0, &c1, &c2}) c->setEvalMultKey(evk.data());
            ShardedBatchedFHEHIPPIE sh({&c0, &c1, &c2}, v, seeds, 3);
            if (sh.tiledLayers() != 3 || sh.binSlices().size() != 3 || sh.binSlices()[1].lo != 1 || sh.binSlices()[1].hi != 2)
                return std::printf("unexpected tiled slices\n"), 1;
            expect_list(sh, "tiled", 3, 2, L);
            sh.setResultLimbs(1);
            expect_list(sh, "tiled_keep1", 3, 2, 1);
            PieContext c3(N, L, T);
            if (!throws([&] { ShardedBatchedFHEHIPPIE bad({&c3}, v, seeds, 0); })) {
                std::printf("layerTiling = 0 was not refused\n");
                failures++;
            }
        }
        if (failures) return std::printf("sharded rows: %d checks FAILED\n", failures), 1;
        std::printf("sharded rows ok\n");
        return 0;
    } catch (const std::exception &ex) {
        std::printf("exception: %s\n", ex.what());
        return 3;
    }
}
