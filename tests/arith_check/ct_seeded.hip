// ct_seeded.hip -- ct_seeded_check FILE: the four forward forms of the 16-coefficient kernels' butterfly block (bfly<false, SC, H2>
// of csrc/ntt16_kernel.h) on operands given by the caller, through the harness of arith_check (dev.h: one small kernel per block,
// per-thread operands from arrays, wave-uniform ones from the kernel argument).  A program of its own: it judges nothing.
// FILE holds one case per line, "q a b w" in decimal; the output is one line per case and form,
// "ct <q> <a> <b> <w> <vec|sc>,<h1|h2> <a'> <b'>", for tests/test_gpu_ct_seeded_block.py to compare with exact integers.
// Exit status 2 on a bad FILE, 3 on a HIP error.
#include <map>
#include <utility>

#include "dev.h"
#include "ntt16_kernel.h"

namespace ac {

namespace n16 = piehip::ntt16;

// in: a, b, w, floor(w 2^63 / q).  SC: the twiddle is wave-uniform, u[U_X] = w, u[U_HAT] = floor(w 2^63 / q)
template <bool SC, bool H2>
struct F_fwd {
    static __device__ __forceinline__ void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)
    {
        n16::ModC m;
        m.nql = (u32)c.u[U_NQ], m.nqh = (u32)(c.u[U_NQ] >> 32), m.nq4 = 0 - 4 * c.u[0], m.q4 = 4 * c.u[0];
        u64 x = AC_IN(0), y = AC_IN(1);
        n16::u64x2 p;
        p.x = SC ? c.u[U_X] : AC_IN(2), p.y = SC ? c.u[U_HAT] : AC_IN(3);
        n16::bfly<false, SC, H2>(x, y, n16::make_tw(p), m);
        AC_OUT(0) = x, AC_OUT(1) = y;
    }
};

template <bool SC, bool H2>
static void run_form(u64 q, u64 w, Cases &cs)
{
    Uni c;
    memset(&c, 0, sizeof c);
    c.u[0] = q, c.u[U_NQ] = 0 - q, c.u[U_N2Q] = 0 - 2 * q;
    c.u[U_X] = w, c.u[U_HAT] = (u64)(((u128)w * P63) / q);
    dev_run<F_fwd<SC, H2>>(cs, c);
    for (u32 i = 0; i < cs.n; i++)
        printf("ct %llu %llu %llu %llu %s,%s %llu %llu\n", ULL(q), ULL(cs.I(0, i)), ULL(cs.I(1, i)), ULL(w), SC ? "sc" : "vec", H2 ? "h2" : "h1",
               ULL(cs.O(0, i)), ULL(cs.O(1, i)));
}

}  // namespace ac

using namespace ac;

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: ct_seeded_check FILE   (lines: q a b w)\n");
        return 2;
    }
    // one launch per (q, w) and form: the scalar forms take w from the kernel argument
    std::map<std::pair<u64, u64>, Cases> groups;
    unsigned long long q, a, b, w;
    int got;
    while ((got = fscanf(f, "%llu %llu %llu %llu", &q, &a, &b, &w)) == 4) {
        if (q < 3 || q >= P60 || a >= 8 * q || b >= P63 || w >= q) {  // the block's contract: a in [0, 8q), b < 2^63, w < q < 2^60
            got = 0;
            break;
        }
        auto it = groups.find({q, w});
        if (it == groups.end()) it = groups.emplace(std::make_pair((u64)q, (u64)w), Cases(4, 2)).first;
        it->second.add({(u64)a, (u64)b, (u64)w, (u64)(((u128)w * P63) / q)});
    }
    fclose(f);
    if (got != EOF || groups.empty()) return 2;
    int ndev = 0;
    AC_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) {
        fprintf(stderr, "ct_seeded_check: no GPU\n");
        return 3;
    }
    for (auto &g : groups) {
        Cases &cs = g.second;
        cs.finish();
        run_form<false, false>(g.first.first, g.first.second, cs);
        run_form<false, true>(g.first.first, g.first.second, cs);
        run_form<true, false>(g.first.first, g.first.second, cs);
        run_form<true, true>(g.first.first, g.first.second, cs);
    }
    printf("ct_seeded_check done\n");
    return 0;
}
