// arith_check [group] CHAIN...  -- the hand-written arithmetic blocks of csrc/ on the device against exact integer arithmetic.
// group: modarith | madasm | stage_a | pie | ntt | ntt16 (default: all of them); CHAIN = N,L,t,q_0,..,q_{L-1},p_0,..,p_L.
// One line per (block, modulus): cases, failures (the first five in full), the histogram of the quotient estimate's error from
// the host model (err) with the coverage it must reach (need, cover), and for the lazy forms the multiple of q left in the output,
// from the device (kdev) and from the model (kmod).  Exit status 1 on any failure or missed coverage, 3 on a HIP error.
// With ARITH_CHECK_MODEL_ONLY set no device is touched (every block then fails): only the operand counts and the host model's
// histograms mean anything, for shaping operand sets without a GPU.
#include "chains.h"
#include "dev.h"

using namespace ac;

int main(int argc, char **argv)
{
    static const struct {
        const char *name;
        bool (*fn)(const std::vector<ModCase> &);
    } groups[] = {{"modarith", group_modarith}, {"madasm", group_madasm}, {"stage_a", group_stage_a},
                  {"pie", group_pie},           {"ntt", group_ntt},       {"ntt16", group_ntt16}};
    int a = 1;
    const char *only = nullptr;
    if (a < argc && !strchr(argv[a], ',')) only = argv[a++];
    std::vector<ModCase> mods;
    for (; a < argc; a++)
        if (!load_chain(argv[a], mods)) {
            fprintf(stderr, "bad chain: %s\n", argv[a]);
            return 2;
        }
    bool known = !only;
    for (const auto &g : groups) known |= only && !strcmp(only, g.name);
    if (mods.empty() || !known) {
        fprintf(stderr, "usage: arith_check [modarith|madasm|stage_a|pie|ntt|ntt16] N,L,t,q..,p.. ...\n");
        return 2;
    }
    int ndev = 0;
    if (!model_only()) AC_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1 && !model_only()) {
        fprintf(stderr, "arith_check: no GPU\n");
        return 3;
    }
    bool ok = true;
    for (const auto &g : groups)
        if (!only || !strcmp(only, g.name)) {
            const bool r = g.fn(mods);
            printf("arith group %s %s\n", g.name, r ? "ok" : "FAILED");
            ok &= r;
        }
    return ok ? 0 : 1;
}
