// Layer tiling through the C++ host facade and the server driver (run by tests/test_gpu_layer_tiling_cpp.py):
//   layer_tiling_check <dir>
// Shape: N = 4096, L = 2, t = 65537, k = 3, e = 110, K = 2, b = 7, E = 3, tiled by R = 3 into b' = 3 layers.  The Python side wrote
// into <dir>: table.bin [k][e][K][b][E] (before the shuffle), server.bin (the set that hashes to it), evk.bin [L][2][L][N], minus.bin
// [2][L][N], idx.bin [K][E][2][L][N] (a real query, its vectors repeated R times) and want.bin [b'][2][L][N], computed by the oracle
// from the tiled arrays; and the same query with its vectors repeated 7 times, minus7.bin, idx7.bin, want7.bin [1][2][L][N].
//   facade   BatchedFHEHIPPIE(cc, hct, seeds, layerTiling = 3): tiledLayers() and the result list are b' long and equal want.bin word
//            for word; layerTiling = 1 keeps b; layerTiling = 0 and 13 (13 k e > N) are std::invalid_argument
//   server   BatchedFHEPSIServer with setLayerTiling(true) over a socket pair, this program being its client: R is
//            piehip_layer_tiling's choice for the shape (7: one tiled layer).  The server sends b' = 1 result message in the framing
//            every result has, equal to want7.bin word for word, and nothing after it
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <sys/socket.h>
#include <thread>
#include <vector>

#include "../nested_hashing_psi_amd/host/BatchedFHEPSIServer.hpp"

using namespace piehip;

static const uint32_t N = 4096, L = 2, k = 3, e = 110, K = 2, b = 7, E = 3, R = 3, bt = 3;
static const uint64_t t = 65537;

static bool load(const std::string &path, std::vector<uint64_t> &v, size_t words)
{
    v.resize(words);
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(v.data(), sizeof(uint64_t), words, f);
    const bool end = std::fgetc(f) == EOF;
    std::fclose(f);
    return got == words && end;
}

static int facade(const std::vector<uint64_t> &tbl, const std::vector<uint64_t> &evk, const std::vector<uint64_t> &minusW,
                  const std::vector<uint64_t> &idxW, const std::vector<uint64_t> &want)
{
    const size_t ct = 2 * (size_t)L * N;
    HashTableView v;
    v.numberOfSimpleTables = k, v.eachSimpleTableSize = e, v.numberOfCuckooTables = K, v.eachBinSize = b, v.eachCuckooTableSize = E;
    v.table = tbl.data();
    PieContext cc(N, L, t);
    cc.setEvalMultKey(evk.data());
    for (uint32_t bad : {0u, 13u}) {
        try {
            BatchedFHEHIPPIE refused(cc, v, BatchedFHEHIPPIE::Seeds{2, 3}, bad);
            return 20;
        } catch (const std::invalid_argument &) {
        }
    }
    BatchedFHEHIPPIE pie(cc, v, BatchedFHEHIPPIE::Seeds{2, 3}, R);
    if (pie.tiledLayers() != bt) return 21;
    uint32_t setting = 0;
    if (piehip_get_layer_tiling(cc.handle(), &setting) != PIEHIP_OK || setting != R) return 22;
    std::vector<std::vector<LimbCt>> m(K, std::vector<LimbCt>(E));
    for (uint32_t h = 0; h < K; h++)
        for (uint32_t j = 0; j < E; j++) m[h][j].limbs.assign(idxW.begin() + ((size_t)h * E + j) * ct, idxW.begin() + ((size_t)h * E + j + 1) * ct);
    LimbCt minus;
    minus.limbs = minusW;
    pie.setMinusCompareElement(minus);
    pie.setIndex(std::move(m));
    pie.run();
    if (pie.getResultList().size() != bt) return 23;
    for (uint32_t g = 0; g < bt; g++) {
        const LimbCt &c = pie.getResultList()[g];
        if (c.limbs.size() != ct) return 24;
        for (size_t w = 0; w < ct; w++)
            if (c.limbs[w] != want[g * ct + w]) return 25;
    }
    // the default argument is the reference's packing: b layers, and the handle's setting is back at 1
    PieContext cc1(N, L, t);
    BatchedFHEHIPPIE plain(cc1, v, BatchedFHEHIPPIE::Seeds{2, 3});
    if (plain.tiledLayers() != b) return 26;
    if (piehip_get_layer_tiling(cc1.handle(), &setting) != PIEHIP_OK || setting != 1) return 27;
    std::printf("facade ok: %u result ciphertexts for %u bin layers tiled by %u\n", bt, b, R);
    return 0;
}

static int server(const std::vector<uint64_t> &set, const std::vector<uint64_t> &evk, const std::vector<uint64_t> &minusW,
                  const std::vector<uint64_t> &idxW, const std::vector<uint64_t> &want)
{
    uint32_t Rs = 0, bts = 0;
    if (piehip_layer_tiling(N, k, e, b, &Rs, &bts) != PIEHIP_OK || Rs != 7 || bts != 1) return 40;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv)) return 41;
    HashTableParameter ht{k, e, K, E, b};
    BatchedFHEPSIServer srv(sv[0], set, ht);
    srv.setSecretSeedsForTesting(1, 2, 3);
    srv.setLayerTiling(true);
    std::string failure;
    std::thread th([&] {
        try {
            srv.run();
        } catch (const std::exception &ex) {
            failure = ex.what();
            shutdown(sv[0], SHUT_RDWR);   // the client below must not wait for a server that has left
        }
    });
    int rc = 0;
    try {
        const int fd = sv[1];
        ContextMessage c{};
        c.N = N, c.L = L, c.t = t;
        {
            PieContext cc(N, L, t);
            uint64_t mod[2 * 7 + 2] = {};
            PieContext::check(piehip_get_moduli(cc.handle(), mod));
            for (uint32_t i = 0; i < 2 * L + 1; i++) c.moduli[i] = mod[i];
        }
        wire::writeWithSize(fd, &c, sizeof(c));
        wire::writeWithSize(fd, nullptr, 0);   // public key: unused
        wire::writeWithSize(fd, evk.data(), evk.size() * sizeof(uint64_t));
        wire::waitForPhaseOver(fd);
        wire::waitForPhaseOver(fd);
        const size_t ct = 2 * (size_t)L * N;
        auto send = [&](const uint64_t *p) {
            const auto msg = wire::packCiphertexts(p, 1, L, N);
            wire::writeWithSize(fd, msg.data(), msg.size());
        };
        send(minusW.data());
        for (uint32_t i = 0; i < K * E; i++) send(idxW.data() + (size_t)i * ct);
        std::vector<uint8_t> msg;
        std::vector<uint64_t> limbs;
        for (uint32_t g = 0; g < bts && !rc; g++) {
            wire::readWithSizeIntoVector(fd, msg);
            if (wire::unpackCiphertexts(msg, L, N, limbs) != 1) rc = 42;
            else if (!std::equal(limbs.begin(), limbs.end(), want.begin() + (size_t)g * ct)) rc = 47;
        }
    } catch (const std::exception &ex) {
        std::printf("client side: %s\n", ex.what());
        rc = 43;
    }
    th.join();
    if (!failure.empty()) {
        std::printf("server side: %s\n", failure.c_str());
        return 44;
    }
    if (rc) return rc;
    if (srv.tiledLayers() != bts) return 45;
    // the server has returned from run(): whatever it sent is in the socket.  Nothing follows the b' messages
    char extra;
    if (recv(sv[1], &extra, 1, MSG_DONTWAIT) >= 0) return 46;
    close(sv[0]);
    close(sv[1]);
    std::printf("server ok: %u result message(s) for %u bin layers\n", bts, b);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    const size_t ct = 2 * (size_t)L * N;
    std::vector<uint64_t> tbl, set, evk, minus, idx, want, minus7, idx7, want7;
    if (!load(dir + "/table.bin", tbl, (size_t)k * e * K * b * E) || !load(dir + "/server.bin", set, 1500) ||
        !load(dir + "/evk.bin", evk, (size_t)L * ct) || !load(dir + "/minus.bin", minus, ct) || !load(dir + "/idx.bin", idx, K * E * ct) ||
        !load(dir + "/want.bin", want, bt * ct) || !load(dir + "/minus7.bin", minus7, ct) || !load(dir + "/idx7.bin", idx7, K * E * ct) ||
        !load(dir + "/want7.bin", want7, ct))
        return 10;
    try {
        if (int rc = facade(tbl, evk, minus, idx, want)) return rc;
        return server(set, evk, minus7, idx7, want7);
    } catch (const std::invalid_argument &ex) {
        std::printf("refused: %s\n", ex.what());
        return 3;
    } catch (const std::runtime_error &ex) {
        std::printf("no device: %s\n", ex.what());
        return 77;
    }
}
