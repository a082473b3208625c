// host_check.cpp -- the host pass of csrc/modarith.h against exact integers (chk_modarith.h), as a stand-alone program:
//   host_check CHAIN...          the contracts; exit status 1 on a failure or a missed coverage condition
//   host_check search CHAIN...   the largest error of the one-word Barrett estimates (reduce123 / reduce124) over 2^24 directed
//                                operands per modulus of (2^59, 2^60), in exact integers (DESIGN.md "Arithmetic blocks")
// Built with g++ -fsanitize=address,undefined by tests/test_arith_host.py; links csrc/params.cpp for HostParams::init.
#include "chains.h"
#include "chk_modarith.h"

using namespace ac;

template <class F>
static void loop(Cases &cs, const Uni &c)
{
    for (u32 i = 0; i < cs.n; i++) F::go(cs.in.data(), cs.out.data(), cs.n, i, c);
}
static void host_run(int id, Cases &cs, const Uni &c)
{
    switch (id) {
    case B_BARRETT128: return loop<F_barrett128>(cs, c);
    case B_MULMOD: return loop<F_mulmod>(cs, c);
    case B_REDUCE123: return loop<F_reduce123>(cs, c);
    case B_REDUCE124: return loop<F_reduce124>(cs, c);
    case B_SHOUP_LAZY: return loop<F_shoup_lazy>(cs, c);
    case B_SHOUP: return loop<F_shoup>(cs, c);
    case B_DIVMOD: return loop<F_divmod>(cs, c);
    case B_FIXFRAC: return loop<F_fixfrac>(cs, c);
    case B_ADD128: return loop<F_add128>(cs, c);
    case B_MAC128: return loop<F_mac128>(cs, c);
    }
    abort();
}

static void search(const ModCase &mc)
{
    const u64 q = mc.m.q;
    for (int bits = 123; bits <= 124; bits++) {
        Rng r(0x5EA0 + bits);
        long hist[8] = {0}, krem[8] = {0};
        u64 total = 0;
        for (int round = 0; round < 4; round++) {  // 4 x 2^22 directed operands + the other families
            const std::vector<u128> zs = ops_barrett(q, bits, 1u << 16, 1u << 22, r, (u64)round << 20);
            for (u128 z : zs) {
                u128 rem = 0;
                const u128 e = bits == 123 ? model_barrett123_err(z, q) : model_barrett124_err(z, q, &rem);
                if (bits == 123) rem = z % q + e * q;
                hist[e < 7 ? (int)e : 7]++;
                krem[rem / q < 7 ? (int)(rem / q) : 7]++;
                total++;
            }
        }
        printf("search reduce%d q=%llu operands=%llu err=[%ld,%ld,%ld,%ld,%ld] remainder/q=[%ld,%ld,%ld,%ld,%ld,%ld,%ld]\n", bits, ULL(q),
               ULL(total), hist[0], hist[1], hist[2], hist[3], hist[4] + hist[5] + hist[6] + hist[7], krem[0], krem[1], krem[2], krem[3],
               krem[4], krem[5], krem[6] + krem[7]);
    }
}

int main(int argc, char **argv)
{
    int a = 1;
    const bool srch = argc > 1 && !strcmp(argv[1], "search");
    if (srch) a++;
    std::vector<ModCase> mods;
    for (; a < argc; a++)
        if (!load_chain(argv[a], mods)) {
            fprintf(stderr, "bad chain: %s\n", argv[a]);
            return 2;
        }
    if (mods.empty()) {
        fprintf(stderr, "usage: host_check [search] N,L,t,q..,p.. ...\n");
        return 2;
    }
    bool ok = true;
    for (const ModCase &mc : mods) {
        if (srch) {
            if (mc.w60()) search(mc);
        } else
            ok &= chk_modarith(host_run, mc);
    }
    printf(ok ? "arith host ok\n" : "arith host FAILED\n");
    return ok ? 0 : 1;
}
