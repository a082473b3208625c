// One rank of a native multi-rank run of query slices across processes (csrc/piehip_rccl.cpp: piehip_rccl_scatter_query,
// piehip_rccl_exchange_accumulators), for tests/test_gpu_slice_ranks.py:
//   slice_ranks_main <transport library | -> <rank> <nranks> <root> <N> <L> <t> <K> <E> <b> <nq> <dir> [keys]
// Every rank loads ITS units (piehip_query_slice) of the database in <dir> for all bin layers and the masks of ITS bin layers
// (piehip_rccl_bin_slice) with piehip_load_db_sliced, joins the communicator (the unique id travels through a file), and then, twice:
// the root writes the nq queries into its piehip_slice_host_buffers_q arrays; every rank calls piehip_rccl_scatter_query,
// piehip_run_slice, piehip_rccl_exchange_accumulators, piehip_run_chain, piehip_gather_results_host and piehip_rccl_wait; the root
// writes the gathered list [b][nq][2][L][N] to <dir>/out<round>.bin.  In round 1 the queries change places.  "keys": every query of
// the batch has its own EvalMult key, evk<q>.bin (piehip_load_relin_key_q); otherwise evk0.bin serves all.  On the way every rank
// checks two refusals that need a communicator: a root outside it (PIEHIP_EINVAL) and a second exchange in one round (PIEHIP_ESTATE).
// The library binds RCCL at run time, the copy already in the process first.  Given a transport library -- on a box with one GPU the
// stand-in of tests/fake_rccl, which the test compiles -- the program loads it with dlopen before its first piehip_rccl_* call, and
// that is then the copy the library finds; with "-" and one rank per GPU the same program runs over the real RCCL.
#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "../include/piehip.h"

static std::vector<uint64_t> slurp(const std::string &path, size_t words)
{
    std::ifstream f(path, std::ios::binary);
    std::vector<uint64_t> v(words);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(words * 8));
    if ((size_t)f.gcount() != words * 8) {
        std::fprintf(stderr, "%s: short file\n", path.c_str());
        std::exit(2);
    }
    return v;
}
#define CHECK(expr)                                                                                   \
    do {                                                                                              \
        int rc_ = (expr);                                                                             \
        if (rc_ != PIEHIP_OK) {                                                                       \
            std::fprintf(stderr, "rank %d: %s -> %d: %s\n", rank, #expr, rc_, piehip_last_error());   \
            return 3;                                                                                 \
        }                                                                                             \
    } while (0)

int main(int argc, char **argv)
{
    if (argc < 13) return 2;
    const std::string transport = argv[1];
    const int rank = std::atoi(argv[2]), G = std::atoi(argv[3]), root = std::atoi(argv[4]);
    const uint32_t N = (uint32_t)std::atoi(argv[5]), L = (uint32_t)std::atoi(argv[6]);
    const uint64_t t = std::strtoull(argv[7], nullptr, 10);
    const uint32_t K = (uint32_t)std::atoi(argv[8]), E = (uint32_t)std::atoi(argv[9]), b = (uint32_t)std::atoi(argv[10]),
                   nq = (uint32_t)std::atoi(argv[11]);
    const std::string dir = argv[12];
    const bool own_keys = argc > 13 && !std::strcmp(argv[13], "keys");
    const size_t LN = (size_t)L * N, ct = 2 * LN;
    if (transport != "-" && !dlopen(transport.c_str(), RTLD_NOW | RTLD_GLOBAL)) {
        std::fprintf(stderr, "rank %d: %s\n", rank, dlerror());
        return 2;
    }
    piehip_handle h = nullptr;
    CHECK(piehip_create(&h, N, L, t, nullptr, nullptr, 0, nullptr));
    uint32_t u_lo = 0, u_hi = 0, lo = 0, hi = 0;
    CHECK(piehip_query_slice(K, L, G, rank, &u_lo, &u_hi));
    CHECK(piehip_rccl_bin_slice(b, G, rank, &lo, &hi));
    {
        const std::vector<uint64_t> db = slurp(dir + "/db.bin", (size_t)K * b * E * LN), masks = slurp(dir + "/masks.bin", (size_t)b * LN);
        // unit u: limb u % L of the plaintexts of inner hash function u / L, [u_n][b][E][N]
        std::vector<uint64_t> mine((size_t)(u_hi - u_lo) * b * E * N);
        for (uint32_t u = u_lo; u < u_hi; u++)
            for (size_t p = 0; p < (size_t)b * E; p++)
                std::memcpy(&mine[((size_t)(u - u_lo) * b * E + p) * N], &db[(((size_t)(u / L) * b * E + p) * L + u % L) * N], (size_t)N * 8);
        CHECK(piehip_load_db_sliced(h, K, b, E, u_lo, u_hi, mine.data(), lo, hi, masks.data() + (size_t)lo * LN));
    }
    if (nq > 1) CHECK(piehip_set_query_batch(h, nq));
    for (uint32_t q = 0; q < (own_keys ? nq : 1u); q++) {
        const std::vector<uint64_t> evk = slurp(dir + "/evk" + std::to_string(q) + ".bin", (size_t)L * 2 * LN);
        if (own_keys)
            CHECK(piehip_load_relin_key_q(h, q, evk.data()));
        else
            CHECK(piehip_load_relin_key(h, evk.data()));
    }
    // the unique id: made on the root, handed over through the file system (a server uses its side sockets)
    unsigned char id[PIEHIP_RCCL_ID_BYTES];
    const std::string idfile = dir + "/unique_id";
    if (rank == root) {
        CHECK(piehip_rccl_unique_id(id));
        std::ofstream f(idfile + ".tmp", std::ios::binary);
        f.write(reinterpret_cast<const char *>(id), sizeof(id));
        f.close();
        std::rename((idfile + ".tmp").c_str(), idfile.c_str());
    } else {
        for (int i = 0; i < 6000; i++) {
            std::ifstream f(idfile, std::ios::binary);
            if (f && f.read(reinterpret_cast<char *>(id), sizeof(id))) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(10));
            if (i == 5999) return 4;
        }
    }
    CHECK(piehip_rccl_init(h, id, G, rank));
    // refused on every rank alike before anything is queued: a root outside the communicator
    if (piehip_rccl_scatter_query(h, G) != PIEHIP_EINVAL || piehip_rccl_scatter_query(h, -1) != PIEHIP_EINVAL) {
        std::fprintf(stderr, "rank %d: a root outside the communicator was not refused with PIEHIP_EINVAL\n", rank);
        return 5;
    }
    // only the root holds whole queries
    std::vector<uint64_t *> pinIdx(nq, nullptr), pinMinus(nq, nullptr);
    std::vector<std::vector<uint64_t>> idx(nq), minus(nq);
    if (rank == root)
        for (uint32_t q = 0; q < nq; q++) {
            CHECK(piehip_slice_host_buffers_q(h, q, &pinIdx[q], &pinMinus[q]));
            idx[q] = slurp(dir + "/idx" + std::to_string(q) + ".bin", (size_t)K * E * ct);
            minus[q] = slurp(dir + "/minus" + std::to_string(q) + ".bin", ct);
        }
    for (int round = 0; round < 2; round++) {
        if (rank == root)
            for (uint32_t q = 0; q < nq; q++) {  // round 1: the queries change places
                const uint32_t src = (q + (uint32_t)round) % nq;
                std::memcpy(pinIdx[q], idx[src].data(), idx[src].size() * 8);
                std::memcpy(pinMinus[q], minus[src].data(), minus[src].size() * 8);
            }
        CHECK(piehip_rccl_scatter_query(h, root));
        CHECK(piehip_run_slice(h));
        CHECK(piehip_rccl_exchange_accumulators(h));
        if (piehip_rccl_exchange_accumulators(h) != PIEHIP_ESTATE) {   // every unit has been put in this round: refused, nothing queued
            std::fprintf(stderr, "rank %d: a second exchange in one round was not refused with PIEHIP_ESTATE\n", rank);
            return 5;
        }
        CHECK(piehip_run_chain(h));
        uint64_t *gathered = nullptr;
        CHECK(piehip_gather_results_host(h, b, root, &gathered));
        CHECK(piehip_rccl_wait(h, 4000));
        if (rank == root) {
            std::ofstream f(dir + "/out" + std::to_string(round) + ".bin", std::ios::binary);
            f.write(reinterpret_cast<const char *>(gathered), (std::streamsize)((size_t)b * nq * ct * 8));
        }
    }
    CHECK(piehip_rccl_destroy(h));
    CHECK(piehip_destroy(h));
    return 0;
}
