// host/WireFraming.hpp, rows of two or three components (packRows, checkedRowsHeader, unpackRows), for tests/test_wire_rows.py:
//   round trips of two- and three-component rows, through a socket pair as size-prefixed messages;
//   a two-component message is byte for byte packCiphertexts' message, and unpackCiphertexts reads it;
//   refused with std::invalid_argument: a length that does not match the component count the header names (a three-component body under
//   a header that says two and the other way round, a body cut short), reserved outside {0, 2, 3} -- high bits included --, a packRows
//   of one or four components, a residue that is not canonical; and unpackCiphertexts refuses a three-component message.
#include <sys/socket.h>

#include <cstdio>
#include <thread>

#include "../nested_hashing_psi_amd/host/WireFraming.hpp"

using namespace piehip::wire;

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            failures++;                                               \
        }                                                             \
    } while (0)

template <typename F>
static bool refused(F f)
{
    try {
        f();
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

static std::vector<uint8_t> with_reserved(std::vector<uint8_t> msg, uint64_t reserved)
{
    LimbHeader h;
    std::memcpy(&h, msg.data(), sizeof(h));
    h.reserved = reserved;
    std::memcpy(msg.data(), &h, sizeof(h));
    return msg;
}

int main()
{
    const uint32_t L = 2, N = 16, count = 3;
    const uint64_t moduli[2] = {1000003, 1000033};
    for (uint32_t ncomp = 2; ncomp <= 3; ncomp++) {
        std::vector<uint64_t> rows((size_t)count * ncomp * L * N);
        for (size_t i = 0; i < rows.size(); i++) rows[i] = (i * 7919 + ncomp) % moduli[(i / N) % L];
        const std::vector<uint8_t> msg = packRows(rows.data(), count, ncomp, L, N);
        EXPECT(msg.size() == sizeof(LimbHeader) + rows.size() * 8);
        LimbHeader h;
        std::memcpy(&h, msg.data(), sizeof(h));
        EXPECT(h.reserved == (ncomp == 2 ? 0u : 3u) && h.count == count && h.L == L && h.N == N);
        // through a channel, as the servers send it
        int sv[2];
        EXPECT(socketpair(AF_UNIX, SOCK_STREAM, 0, sv) == 0);
        std::thread sender([&] { writeWithSize(sv[0], msg.data(), msg.size()); });
        std::vector<uint8_t> got;
        readWithSizeIntoVector(sv[1], got);
        sender.join();
        close(sv[0]);
        close(sv[1]);
        EXPECT(got == msg);
        std::vector<uint64_t> back;
        uint32_t nc = 0;
        EXPECT(unpackRows(got, L, N, back, &nc, moduli) == count && nc == ncomp && back == rows);
        // reserved = 2 names two components as 0 does
        if (ncomp == 2) {
            EXPECT(msg == packCiphertexts(rows.data(), count, L, N));
            std::vector<uint64_t> old;
            EXPECT(unpackCiphertexts(msg, L, N, old, moduli) == count && old == rows);
            nc = 0;
            EXPECT(unpackRows(with_reserved(msg, 2), L, N, back, &nc) == count && nc == 2 && back == rows);
        } else {
            std::vector<uint64_t> old;
            EXPECT(refused([&] { unpackCiphertexts(msg, L, N, old); }));   // three rows of three components are no three rows of two
        }
        // a length that does not match the named component count
        EXPECT(refused([&] { unpackRows(with_reserved(msg, ncomp == 2 ? 3 : 0), L, N, back, &nc); }));
        std::vector<uint8_t> cut(msg.begin(), msg.end() - 8);
        EXPECT(refused([&] { unpackRows(cut, L, N, back, &nc); }));
        std::vector<uint8_t> longer = msg;
        longer.resize(msg.size() + (size_t)L * N * 8);
        EXPECT(refused([&] { unpackRows(longer, L, N, back, &nc); }));
        // reserved outside {0, 2, 3}
        for (uint64_t r : {(uint64_t)1, (uint64_t)4, (uint64_t)5, ((uint64_t)1 << 32) | ncomp, ~(uint64_t)0})
            EXPECT(refused([&] { unpackRows(with_reserved(msg, r), L, N, back, &nc); }));
        // the context, and a residue at its modulus
        EXPECT(refused([&] { unpackRows(msg, L + 1, N, back, &nc); }));
        std::vector<uint64_t> bad = rows;
        bad[(size_t)(count * ncomp * L - 1) * N + 3] = moduli[1];
        EXPECT(refused([&] { unpackRows(packRows(bad.data(), count, ncomp, L, N), L, N, back, &nc, moduli); }));
    }
    // a message whose count does not fit its length is refused before anything is sized by it
    {
        std::vector<uint64_t> one((size_t)3 * L * N, 1);
        std::vector<uint8_t> msg = packRows(one.data(), 1, 3, L, N);
        LimbHeader h;
        std::memcpy(&h, msg.data(), sizeof(h));
        h.count = 0x7fffffffu;
        std::memcpy(msg.data(), &h, sizeof(h));
        std::vector<uint64_t> back;
        uint32_t nc = 0;
        EXPECT(refused([&] { unpackRows(msg, L, N, back, &nc); }) && back.empty());
        EXPECT(refused([&] { packRows(one.data(), 1, 1, L, N); }) && refused([&] { packRows(one.data(), 1, 4, L, N); }));
        EXPECT(refused([&] { unpackRows(std::vector<uint8_t>(8), L, N, back, &nc); }));
    }
    if (failures) return std::printf("wire rows: %d checks FAILED\n", failures), 1;
    std::printf("wire rows ok\n");
    return 0;
}
