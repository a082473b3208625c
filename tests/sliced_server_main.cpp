// One rank of the multi-process C++ server in query-sliced mode (host/ShardedBatchedFHEPSIServer.hpp, querySlices = true):
//   sliced_server_main <transport library | -> <rank> <nranks> <device> <client fd | -1> <side fd[,side fd ...] | -> <server set file> k e K E b
// The arguments behind the first are those of tests/sharded_server_main.cpp.  Given a transport library -- on a box with one GPU the
// stand-in of tests/fake_rccl, compiled by tests/test_gpu_sliced_server.py -- the program loads it with dlopen before the server
// starts, and the library then binds that copy; with "-" and one rank per GPU the same program runs over the real RCCL.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "../nested_hashing_psi_amd/host/ShardedBatchedFHEPSIServer.hpp"

int main(int argc, char **argv)
{
    if (argc != 13) return 2;
    try {
        if (std::strcmp(argv[1], "-") && !dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL)) throw std::runtime_error(dlerror());
        const int rank = std::atoi(argv[2]), nranks = std::atoi(argv[3]), device = std::atoi(argv[4]), client = std::atoi(argv[5]);
        std::vector<int> side;
        if (std::strcmp(argv[6], "-"))
            for (const char *p = argv[6]; *p;) {
                char *end = nullptr;
                side.push_back((int)std::strtol(p, &end, 10));
                p = (*end == ',') ? end + 1 : end;
            }
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
        piehip::ShardedBatchedFHEPSIServer server(rank, nranks, device, client, side, set, ht);
        server.querySlices = true;
        // tests only: fixed table secrets (so that the result ciphertexts can be compared with the oracle's bit for bit) and a shorter
        // bound on the waits for the other ranks
        if (const char *sd = std::getenv("PIEHIP_TEST_SEEDS")) {
            unsigned long long a = 0, b = 0, c = 0;
            if (std::sscanf(sd, "%llu,%llu,%llu", &a, &b, &c) == 3) server.setSecretSeedsForTesting(a, b, c);
        }
        if (const char *tm = std::getenv("PIEHIP_TEST_TIMEOUT_MS")) server.collectiveTimeoutMs = (uint32_t)std::atoi(tm);
        server.run();
        if (rank == 0) std::printf("OfflineComputation,%lld\nOnlineComputation,%lld\n", server.offlineComputation, server.onlineComputation);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "server rank %s: %s\n", argv[2], e.what());
        return 1;
    }
}
