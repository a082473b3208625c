// One rank of a native multi-rank run of the sharded path behind the C ABI (csrc/piehip_rccl.cpp) with result rows of another shape
// than [2][L][N], for tests/test_gpu_gather_rows.py:
//   rows_ranks_main <transport library | -> <rank> <nranks> <root> <N> <L> <t> <K> <E> <b> <nq> <dir> <keys> <setting0> <setting1> [mode]
// keys: "none" (no EvalMult key on any rank), "one" (evk0.bin serves every query), "each" (evk<q>.bin per query).
// A setting is keep:relin:schedule with the schedule's entries joined by '-', 0 for "leave it": "1:1:0" keeps one limb, "0:0:0" hands
// out degree-2 rows, "1:1:3" runs the chain on three limbs and keeps one of them, "2:1:4-3" is the schedule (4, 3) with keep = 2.
// <setting0> is applied before round 0, <setting1> before round 1 where it differs; each application is followed by
// piehip_rccl_agree_rows.  Every rank loads ITS slice of the bin layers of the database in <dir>, joins the communicator (the unique id
// travels through a file) and then, twice: the root stages the nq queries, piehip_rccl_broadcast_query, piehip_run,
// piehip_gather_results_host, piehip_rccl_wait; the root writes the gathered list [b][nq][ncomp][rl][N] to <dir>/out<round>.bin and
// its shape "ncomp rl" to <dir>/shape<round>.txt.
// mode: "differ"  the LAST rank applies <setting1> where the others apply <setting0>: every rank must see same = 0 and have its
//                 gather refused with PIEHIP_ESTATE -- locally, nothing is posted --, after which a wait returns at once; exit 0.
//       "stale"   after round 0 every rank changes a setting and changes it back: the gather is refused (PIEHIP_ESTATE) until the ranks
//                 have agreed again, then round 1 runs.
//       "default" no setting and NO agreement call: the gather of default rows works as ever.
// The library binds RCCL at run time, the copy already in the process first.  Given a transport library -- on a box with one GPU the
// stand-in of tests/fake_rccl, which the test compiles -- the program loads it with dlopen before its first piehip_rccl_* call; with
// "-" and one rank per GPU the same program runs over the real RCCL.
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

struct Setting {
    uint32_t keep = 0;
    int relin = 1;
    std::vector<uint32_t> sched;
};
static Setting parse(const std::string &s)
{
    Setting out;
    const size_t a = s.find(':'), b = s.find(':', a + 1);
    out.keep = (uint32_t)std::atoi(s.substr(0, a).c_str());
    out.relin = std::atoi(s.substr(a + 1, b - a - 1).c_str());
    std::string rest = s.substr(b + 1);
    for (size_t at = 0; at < rest.size();) {
        const size_t dash = rest.find('-', at);
        const uint32_t v = (uint32_t)std::atoi(rest.substr(at, dash - at).c_str());
        if (v) out.sched.push_back(v);
        if (dash == std::string::npos) break;
        at = dash + 1;
    }
    return out;
}
// every part of a setting, set outright (0 / empty: the default), so that going from one setting to another leaves nothing behind
static int apply(piehip_handle h, const Setting &s, uint32_t L)
{
    int rc = piehip_set_result_relin(h, s.relin);
    if (rc) return rc;
    const uint32_t all = L;
    if ((rc = piehip_set_chain_schedule(h, s.sched.empty() ? &all : s.sched.data(), s.sched.empty() ? 1 : (uint32_t)s.sched.size()))) return rc;
    return piehip_set_result_limbs(h, s.keep ? s.keep : L);
}

int main(int argc, char **argv)
{
    if (argc < 16) return 2;
    const std::string transport = argv[1];
    const int rank = std::atoi(argv[2]), G = std::atoi(argv[3]), root = std::atoi(argv[4]);
    const uint32_t N = (uint32_t)std::atoi(argv[5]), L = (uint32_t)std::atoi(argv[6]);
    const uint64_t t = std::strtoull(argv[7], nullptr, 10);
    const uint32_t K = (uint32_t)std::atoi(argv[8]), E = (uint32_t)std::atoi(argv[9]), b = (uint32_t)std::atoi(argv[10]),
                   nq = (uint32_t)std::atoi(argv[11]);
    const std::string dir = argv[12], keys = argv[13], mode = argc > 16 ? argv[16] : "";
    const Setting set0 = parse(argv[14]), set1 = parse(argv[15]);
    const bool changes = std::strcmp(argv[14], argv[15]) != 0;
    const size_t LN = (size_t)L * N, ct = 2 * LN;
    const uint32_t timeout_ms = 4000;
    if (transport != "-" && !dlopen(transport.c_str(), RTLD_NOW | RTLD_GLOBAL)) {
        std::fprintf(stderr, "rank %d: %s\n", rank, dlerror());
        return 2;
    }
    piehip_handle h = nullptr;
    CHECK(piehip_create(&h, N, L, t, nullptr, nullptr, 0, nullptr));
    uint32_t lo = 0, hi = 0;
    CHECK(piehip_rccl_bin_slice(b, G, rank, &lo, &hi));
    if (nq > 1) CHECK(piehip_set_query_batch(h, nq));
    for (uint32_t q = 0; keys != "none" && q < (keys == "each" ? nq : 1u); q++) {
        const std::vector<uint64_t> evk = slurp(dir + "/evk" + std::to_string(q) + ".bin", (size_t)L * 2 * LN);
        if (keys == "each")
            CHECK(piehip_load_relin_key_q(h, q, evk.data()));
        else
            CHECK(piehip_load_relin_key(h, evk.data()));
    }
    {
        const std::vector<uint64_t> db = slurp(dir + "/db.bin", (size_t)K * b * E * LN), masks = slurp(dir + "/masks.bin", (size_t)b * LN);
        const uint32_t nb = hi - lo;
        std::vector<uint64_t> mine((size_t)K * nb * E * LN);
        for (uint32_t hf = 0; hf < K; hf++)
            std::memcpy(&mine[(size_t)hf * nb * E * LN], &db[((size_t)hf * b + lo) * E * LN], (size_t)nb * E * LN * 8);
        CHECK(piehip_load_db(h, K, nb, E, mine.data(), masks.data() + (size_t)lo * LN));
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
    // the settings, after the communicator: piehip_rccl_init forgets an agreement as every setter does
    const bool odd_one = mode == "differ" && rank == G - 1;
    int same = -1;
    if (mode != "default") {
        CHECK(apply(h, odd_one ? set1 : set0, L));
        uint32_t ncomp = 0, keep = 0, lc = 0;
        CHECK(piehip_get_result_components(h, &ncomp));
        CHECK(piehip_get_result_limbs(h, &keep));
        CHECK(piehip_get_chain_limbs(h, &lc));
        const bool plain_rows = ncomp == 2 && keep == L && (K < 2 || lc == L);
        uint64_t *early = nullptr;   // a setting and no agreement yet: refused here, before anything is queued
        if (!plain_rows && (piehip_gather_results_host(h, b, root, &early) != PIEHIP_ESTATE || !std::strstr(piehip_last_error(), "piehip_rccl_agree_rows"))) {
            std::fprintf(stderr, "rank %d: a gather before the agreement was not refused with PIEHIP_ESTATE naming piehip_rccl_agree_rows\n", rank);
            return 5;
        }
        CHECK(piehip_rccl_agree_rows(h, timeout_ms, &same));
        std::printf("rank %d: agree_rows -> %d\n", rank, same);
    }
    if (mode == "differ") {
        uint64_t *none = nullptr;
        const int rc = piehip_gather_results_host(h, b, root, &none);
        std::printf("rank %d: gather -> %d\n", rank, rc);
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(piehip_rccl_wait(h, timeout_ms));   // nothing was posted: nothing to wait for
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("rank %d: wait %s\n", rank, ms < 1000 ? "returned at once" : "took long");
        CHECK(piehip_rccl_destroy(h));
        CHECK(piehip_destroy(h));
        return same == 0 && rc == PIEHIP_ESTATE ? 0 : 5;
    }
    if (mode != "default" && same != 1) return 5;
    // only the root stages queries from host memory; the others need their device-side input buffers
    std::vector<uint64_t *> pinIdx(nq, nullptr), pinMinus(nq, nullptr);
    for (uint32_t q = 0; q < nq; q++) {
        if (rank == root)
            CHECK(piehip_host_buffers_q(h, q, &pinIdx[q], &pinMinus[q], nullptr));
        else
            CHECK(piehip_host_buffers_q(h, q, nullptr, nullptr, nullptr));
    }
    std::vector<std::vector<uint64_t>> idx(nq), minus(nq);
    if (rank == root)
        for (uint32_t q = 0; q < nq; q++) {
            idx[q] = slurp(dir + "/idx" + std::to_string(q) + ".bin", (size_t)K * E * ct);
            minus[q] = slurp(dir + "/minus" + std::to_string(q) + ".bin", ct);
        }
    for (int round = 0; round < 2; round++) {
        if (round == 1 && mode == "stale") {
            // a setting changed after the agreement -- and changed back: the rows are what was agreed, the agreement is gone all the same
            uint32_t keep = 0;
            CHECK(piehip_get_result_limbs(h, &keep));
            CHECK(piehip_set_result_limbs(h, keep == L ? L - 1 : L));
            CHECK(piehip_set_result_limbs(h, keep));
        }
        if (round == 1 && changes) CHECK(apply(h, set1, L));
        if (round == 1 && (changes || mode == "stale")) {
            uint64_t *stale = nullptr;
            if (piehip_gather_results_host(h, b, root, &stale) != PIEHIP_ESTATE) {
                std::fprintf(stderr, "rank %d: a gather after a changed setting was not refused with PIEHIP_ESTATE\n", rank);
                return 5;
            }
            CHECK(piehip_rccl_agree_rows(h, timeout_ms, &same));
            if (same != 1) return 5;
        }
        if (rank == root)
            for (uint32_t q = 0; q < nq; q++) {  // round 1: the queries change places
                const uint32_t src = (q + (uint32_t)round) % nq;
                std::memcpy(pinIdx[q], idx[src].data(), idx[src].size() * 8);
                std::memcpy(pinMinus[q], minus[src].data(), minus[src].size() * 8);
                CHECK(piehip_stage_minus_q(h, q, pinMinus[q]));
                for (uint32_t hf = 0; hf < K; hf++) CHECK(piehip_stage_index_row_q(h, q, hf, pinIdx[q] + (size_t)hf * E * ct));
            }
        CHECK(piehip_rccl_broadcast_query(h, root));
        CHECK(piehip_run(h));
        uint64_t *gathered = nullptr;
        CHECK(piehip_gather_results_host(h, b, root, &gathered));
        CHECK(piehip_rccl_wait(h, timeout_ms));
        if (rank == root) {
            uint32_t ncomp = 0, keep = 0, lc = 0;
            CHECK(piehip_get_result_components(h, &ncomp));
            CHECK(piehip_get_result_limbs(h, &keep));
            CHECK(piehip_get_chain_limbs(h, &lc));
            const uint32_t rl = K >= 2 && lc < keep ? lc : keep;
            std::ofstream f(dir + "/out" + std::to_string(round) + ".bin", std::ios::binary);
            f.write(reinterpret_cast<const char *>(gathered), (std::streamsize)((size_t)b * nq * ncomp * rl * N * 8));
            std::ofstream s(dir + "/shape" + std::to_string(round) + ".txt");
            s << ncomp << " " << rl << "\n";
        }
    }
    CHECK(piehip_rccl_destroy(h));
    CHECK(piehip_destroy(h));
    return 0;
}
