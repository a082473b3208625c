// fold_bfly_check FILE: the three butterfly blocks for q = 2^60 - d (csrc/ntt16_kernel.h: bfly<INV, SC, H2, ArithKind::fold>; forward with
// u = fold(a), inverse with a' = fold(a + b), inverse without a fold) in their four forms each, on operands given by the caller, through
// the harness of tests/arith_check (dev.h: one small kernel per block, per-thread operands from arrays, wave-uniform ones from the
// kernel argument).  A program of its own: it judges nothing.
// FILE holds one case per line, "kind q a b w" in decimal with kind = ctf | gsf | gsn; the output is one line per case and form,
// "r <line> <vec|sc>,<h1|h2> <a'> <b'>" (<line>: the case's line number in FILE, from 0), for tests/test_gpu_fold_bfly_block.py to
// compare with exact integers.  Exit status 2 on a bad FILE, 3 on a HIP error.
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "dev.h"
#include "ntt16_kernel.h"

namespace ac {

namespace n16 = piehip::ntt16;
using piehip::ArithKind;

enum Kind { CTF, GSF, GSN };

// in: a, b, w, floor(w 2^63 / q).  SC: the twiddle is wave-uniform, u[U_X] = w, u[U_HAT] = floor(w 2^63 / q)
template <int KIND, bool SC, bool H2>
struct F_fold {
    static __device__ __forceinline__ void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)
    {
        n16::ModC m;
        m.nql = (u32)c.u[U_NQ], m.nqh = (u32)(c.u[U_NQ] >> 32), m.nq4 = 0 - 4 * c.u[0], m.q4 = 4 * c.u[0];
        u64 x = AC_IN(0), y = AC_IN(1);
        n16::u64x2 p;
        p.x = SC ? c.u[U_X] : AC_IN(2), p.y = SC ? c.u[U_HAT] : AC_IN(3);
        n16::bfly<KIND != CTF, SC, H2, ArithKind::fold>(x, y, n16::make_tw(p), m, KIND == GSN);
        AC_OUT(0) = x, AC_OUT(1) = y;
    }
};

template <int KIND, bool SC, bool H2>
static void run_form(u64 q, u64 w, Cases &cs, const std::vector<u32> &lines)
{
    Uni c;
    memset(&c, 0, sizeof c);
    c.u[0] = q, c.u[U_NQ] = 0 - q, c.u[U_N2Q] = 0 - 2 * q;
    c.u[U_X] = w, c.u[U_HAT] = (u64)(((u128)w * P63) / q);
    dev_run<F_fold<KIND, SC, H2>>(cs, c);
    for (u32 i = 0; i < cs.n; i++) printf("r %u %s,%s %llu %llu\n", lines[i], SC ? "sc" : "vec", H2 ? "h2" : "h1", ULL(cs.O(0, i)), ULL(cs.O(1, i)));
}
template <int KIND>
static void run_kind(u64 q, u64 w, Cases &cs, const std::vector<u32> &lines)
{
    run_form<KIND, false, false>(q, w, cs, lines);
    run_form<KIND, false, true>(q, w, cs, lines);
    run_form<KIND, true, false>(q, w, cs, lines);
    run_form<KIND, true, true>(q, w, cs, lines);
}

struct Group {
    Cases cs{4, 2};
    std::vector<u32> lines;
};

}  // namespace ac

using namespace ac;

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: fold_bfly_check FILE   (lines: ctf|gsf|gsn q a b w)\n");
        return 2;
    }
    // one launch per (kind, q, w) and form: the scalar forms take w from the kernel argument
    std::map<std::tuple<int, u64, u64>, Group> groups;
    char kind[8];
    unsigned long long q, a, b, w;
    int got;
    u32 line = 0;
    const u64 T = P60 + (1ull << 31);
    while ((got = fscanf(f, "%7s %llu %llu %llu %llu", kind, &q, &a, &b, &w)) == 5) {
        const std::string ks = kind;
        const int k = ks == "ctf" ? CTF : ks == "gsf" ? GSF : ks == "gsn" ? GSN : -1;
        // the blocks' contracts: q = 2^60 - d with d < 2^27, w < q; forward: any 64-bit a, b < 2^63; inverse: a, b < 4q (below T without a fold)
        bool ok = k >= 0 && q < P60 && P60 - q < (1ull << 27) && w < q;
        if (k == CTF) ok = ok && b < P63;
        if (k == GSF) ok = ok && a < 4 * q && b < 4 * q;
        if (k == GSN) ok = ok && a < T && b < T;
        if (!ok) {
            got = 0;
            break;
        }
        Group &g = groups[std::make_tuple(k, (u64)q, (u64)w)];
        g.cs.add({(u64)a, (u64)b, (u64)w, (u64)(((u128)w * P63) / q)});
        g.lines.push_back(line++);
    }
    fclose(f);
    if (got != EOF || groups.empty()) return 2;
    int ndev = 0;
    AC_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) {
        fprintf(stderr, "fold_bfly_check: no GPU\n");
        return 3;
    }
    for (auto &g : groups) {
        Cases &cs = g.second.cs;
        cs.finish();
        const int k = std::get<0>(g.first);
        const u64 gq = std::get<1>(g.first), gw = std::get<2>(g.first);
        if (k == CTF) run_kind<CTF>(gq, gw, cs, g.second.lines);
        if (k == GSF) run_kind<GSF>(gq, gw, cs, g.second.lines);
        if (k == GSN) run_kind<GSN>(gq, gw, cs, g.second.lines);
    }
    printf("fold_bfly_check done\n");
    return 0;
}
