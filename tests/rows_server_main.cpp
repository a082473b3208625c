// The C++ servers with the settings that change the shape of a result row, for tests/test_gpu_sharded_server_rows.py:
//   rows_server_main <transport library | -> <rank> <nranks> <device> <client fd[,client fd ...] | -1> <side fd[,side fd ...] | -> <server set file>
//                    k e K E b <setting> [slices]
// nranks >= 1: one rank of host/ShardedBatchedFHEPSIServer.hpp, the arguments those of tests/sliced_server_main.cpp.
// nranks == 0: host/BatchedFHEPSIServer.hpp in this one process, one client per channel, their queries evaluated as one batch.
// <setting> is keep:relin:schedule as in tests/rows_ranks_main.cpp (0 = as ever; a schedule of one entry is the chain-limbs option);
// "slices" asks for the query-sliced mode as well, which the server must refuse together with a setting.
// Exit status 1 and "invalid_argument: ..." on standard error for std::invalid_argument, "error: ..." for any other exception.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "../nested_hashing_psi_amd/host/ShardedBatchedFHEPSIServer.hpp"

static std::vector<int> fd_list(const char *arg)
{
    std::vector<int> out;
    if (!std::strcmp(arg, "-")) return out;
    for (const char *p = arg; *p;) {
        char *end = nullptr;
        out.push_back((int)std::strtol(p, &end, 10));
        p = (*end == ',') ? end + 1 : end;
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 14) return 2;
    try {
        if (std::strcmp(argv[1], "-") && !dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL)) throw std::runtime_error(dlerror());
        const int rank = std::atoi(argv[2]), nranks = std::atoi(argv[3]), device = std::atoi(argv[4]);
        const std::vector<int> clients = fd_list(argv[5]), side = fd_list(argv[6]);
        std::ifstream f(argv[7], std::ios::binary | std::ios::ate);
        const size_t bytes = (size_t)f.tellg();
        f.seekg(0);
        std::vector<uint64_t> set(bytes / 8);
        f.read(reinterpret_cast<char *>(set.data()), (std::streamsize)(set.size() * 8));
        piehip::HashTableParameter ht;
        ht.numberOfSimpleHashFunctions = (uint32_t)std::atoi(argv[8]);
        ht.eachSimpleTableSize = (uint32_t)std::atoi(argv[9]);
        ht.numberOfCuckooHashFunctions = (uint32_t)std::atoi(argv[10]);
        ht.eachCuckooTableSize = (uint32_t)std::atoi(argv[11]);
        ht.maxItemsPerPosition = (uint32_t)std::atoi(argv[12]);
        unsigned keep = 0, relin = 1;
        char sched_text[64] = "";
        if (std::sscanf(argv[13], "%u:%u:%63s", &keep, &relin, sched_text) != 3) return 2;
        std::vector<uint32_t> sched;
        for (const char *p = sched_text; *p;) {
            char *end = nullptr;
            const uint32_t v = (uint32_t)std::strtoul(p, &end, 10);
            if (v) sched.push_back(v);
            p = (*end == '-') ? end + 1 : end;
        }
        const bool slices = argc > 14 && !std::strcmp(argv[14], "slices");
        unsigned long long sa = 0, sb = 0, sc = 0;   // tests only: fixed table secrets, so that the rows can be compared bit for bit
        const char *sd = std::getenv("PIEHIP_TEST_SEEDS");
        const bool seeded = sd && std::sscanf(sd, "%llu,%llu,%llu", &sa, &sb, &sc) == 3;
        if (nranks == 0) {
            piehip::BatchedFHEPSIServer server(clients, set, ht, 987654321, sched.empty() ? 0 : sched[0]);
            if (keep) server.setResultLimbs(keep);
            server.setResultRelin(relin != 0);
            if (seeded) server.setSecretSeedsForTesting(sa, sb, sc);
            server.run();
            return 0;
        }
        piehip::ShardedBatchedFHEPSIServer server(rank, nranks, device, clients.empty() ? -1 : clients[0], side, set, ht);
        server.querySlices = slices;
        server.resultLimbs = keep;
        server.resultRelin = relin != 0;
        if (sched.size() == 1) server.chainLimbs = sched[0];
        else server.chainSchedule = sched;
        if (seeded) server.setSecretSeedsForTesting(sa, sb, sc);
        if (const char *tm = std::getenv("PIEHIP_TEST_TIMEOUT_MS")) server.collectiveTimeoutMs = (uint32_t)std::atoi(tm);
        server.run();
        return 0;
    } catch (const std::invalid_argument &e) {
        std::fprintf(stderr, "invalid_argument: %s\n", e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
