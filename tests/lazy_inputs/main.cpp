// lazy_inputs_check OP DIR N L t q_0 .. q_{L-1} p_0 .. p_L [name=value ...]
// One launch of ONE kernel of the product chain on arrays the caller gives, so that a test can hand it the ends of its lazy input
// range -- representatives that the transforms inside the library produce with negligible probability (tests/lazy_inputs.py,
// tests/test_gpu_lazy_inputs.py).  A program of its own, linked with the library's objects: it makes a handle with piehip_create,
// takes the constants, the plan and the lane-order map from it and calls one piehip::launch_* of kernels.hpp.  It judges nothing.
//
// Inputs are DIR/in_<name>.u64 (raw little-endian words, exactly the words the launch indexes: any other size is refused), outputs
// DIR/out_<name>.u64: GUARD words, the array, GUARD words, everything pre-filled with FILL so that guards and places a mode does not
// write can be told from written ones (FILL has its top bit set: no residue below 2^63 equals it).  DIR/out_sigma_inv.u64 is the
// handle's lane-order map, one word per position.  The line "plan ..." says what the context decided.
// Exit status: 0 ran; 2 usage, or a shape the launcher refuses; 3 a HIP error the runtime reported.
#include <map>
#include <string>

#include "piehip_ctx.hpp"

using namespace piehip;

static const size_t GUARD = 64;
static const u64 FILL = 0xF1F1F1F1F1F1F1F1ull;

#define LI_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "lazy_inputs_check: %s: %s\n", #expr, hipGetErrorString(e_));     \
            exit(3);                                                                          \
        }                                                                                     \
    } while (0)

static std::string g_dir;
static std::map<std::string, unsigned long long> g_opt;

[[noreturn]] static void refuse(const char *why)
{
    fprintf(stderr, "lazy_inputs_check: refused: %s\n", why);
    exit(2);
}
static u32 opt(const char *name, u32 dflt = 0)
{
    auto it = g_opt.find(name);
    return it == g_opt.end() ? dflt : (u32)it->second;
}

// an input array: exactly `words` words of DIR/in_<name>.u64, in device memory
static u64 *input(const char *name, size_t words)
{
    const std::string path = g_dir + "/in_" + name + ".u64";
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) refuse(("no " + path).c_str());
    std::vector<u64> host(words + 1);
    const size_t got = fread(host.data(), sizeof(u64), words + 1, f);
    fclose(f);
    if (got != words) refuse((path + ": not the words this launch reads").c_str());
    u64 *d = nullptr;
    LI_HIP(hipMalloc((void **)&d, words * sizeof(u64)));
    LI_HIP(hipMemcpy(d, host.data(), words * sizeof(u64), hipMemcpyHostToDevice));
    return d;
}
// an output array between its guards; `from`: an in-place kernel's data, loaded from DIR/in_<from>.u64
struct Out {
    u64 *base = nullptr;
    size_t words = 0;
    u64 *data() const { return base + GUARD; }
};
static Out output(size_t words, const char *from = nullptr)
{
    Out o;
    o.words = words;
    std::vector<u64> host(words + 2 * GUARD, FILL);
    if (from) {
        const std::string path = g_dir + "/in_" + from + ".u64";
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) refuse(("no " + path).c_str());
        std::vector<u64> in(words + 1);
        const size_t got = fread(in.data(), sizeof(u64), words + 1, f);
        fclose(f);
        if (got != words) refuse((path + ": not the words this launch transforms").c_str());
        std::copy(in.begin(), in.begin() + words, host.begin() + GUARD);
    }
    LI_HIP(hipMalloc((void **)&o.base, host.size() * sizeof(u64)));
    LI_HIP(hipMemcpy(o.base, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice));
    return o;
}
static void save_words(const char *name, const std::vector<u64> &host)
{
    const std::string path = g_dir + "/out_" + name + ".u64";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(host.data(), sizeof(u64), host.size(), f) != host.size()) {
        fprintf(stderr, "lazy_inputs_check: cannot write %s\n", path.c_str());
        exit(2);
    }
    fclose(f);
}
static void save(const char *name, const Out &o)
{
    std::vector<u64> host(o.words + 2 * GUARD);
    LI_HIP(hipMemcpy(host.data(), o.base, host.size() * sizeof(u64), hipMemcpyDeviceToHost));
    save_words(name, host);
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        fprintf(stderr, "usage: lazy_inputs_check OP DIR N L t q_0 .. q_{L-1} p_0 .. p_L [name=value ...]\n");
        return 2;
    }
    const std::string op = argv[1];
    g_dir = argv[2];
    const u32 N = (u32)strtoul(argv[3], nullptr, 10), L = (u32)strtoul(argv[4], nullptr, 10);
    const u64 t = strtoull(argv[5], nullptr, 10);
    if (!L || L > 7 || argc < (int)(6 + 2 * L + 1)) refuse("L, or fewer than 2 L + 1 moduli");
    const u32 M = 2 * L + 1;
    std::vector<u64> q(L), p(L + 1);
    for (u32 i = 0; i < M; i++) (i < L ? q[i] : p[i - L]) = strtoull(argv[6 + i], nullptr, 10);
    for (int i = 6 + (int)M; i < argc; i++) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) refuse("an option without '='");
        g_opt[std::string(argv[i], eq - argv[i])] = strtoull(eq + 1, nullptr, 10);
    }
    int ndev = 0;
    LI_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) {
        fprintf(stderr, "lazy_inputs_check: no GPU\n");
        return 3;
    }
    piehip_handle h = nullptr;
    if (piehip_create(&h, N, L, t, q.data(), p.data(), 0, nullptr) != PIEHIP_OK) {
        fprintf(stderr, "lazy_inputs_check: piehip_create: %s\n", piehip_last_error());
        return 2;
    }
    const DevConsts *dc = h->d_dc;
    const NttPlan &pl = h->plan;
    const u32 *sigma_inv = h->d_sigma_inv;
    hipStream_t st = h->stream;
    const bool sm = pl.small_moduli;
    printf("plan lane_order=%d fold=%d lane_kp=%u lane_T=%u small_moduli=%d fused_tensor=%d d01_eval_q=%d result_eval_q=%d\n", (int)pl.lane_order,
           (int)pl.fold, pl.lane_kp, pl.lane_T, (int)sm, (int)pl.fused_tensor, (int)pl.d01_eval_q, (int)pl.result_eval_q);
    {
        std::vector<u32> m32(N);
        LI_HIP(hipMemcpy(m32.data(), sigma_inv, (size_t)N * sizeof(u32), hipMemcpyDeviceToHost));
        save_words("sigma_inv", std::vector<u64>(m32.begin(), m32.end()));
    }
    const size_t LN = (size_t)L * N, MN = (size_t)M * N;
    const bool fold = opt("fold") != 0;
    if (fold && !pl.fold) refuse("fold on a ring whose transforms are not folded");

    if (op == "relin_mac") {
        // nb rows; kp=1: out_map is the lane order of the plan (LDS tile), 0: none; key_group keys key_stride words apart; mask=1 with
        // mask_div rows per mask; eq=1: the own-limb term from in_eqp
        const u32 nb = opt("nb", 1), G = opt("key_group", 1), md = opt("mask_div", 1);
        const bool kp = opt("kp") != 0, with_mask = opt("mask") != 0, eq = opt("eq") != 0;
        const size_t key_words = (size_t)L * 2 * LN, ks = G > 1 ? (size_t)g_opt["key_stride"] : 0;
        if (!nb || !G || !md || (G > 1 && ks < key_words) || (ks & 1)) refuse("nb, key_group, key_stride or mask_div");
        if (kp && !pl.lane_order) refuse("kp on a context without a lane order");
        if (eq && !sm) refuse("eq off the column-accumulator path");
        const u64 *d01 = input("d01", (size_t)nb * 2 * LN), *dig = input("dig", (size_t)nb * L * LN);
        const u64 *key = input("key", (size_t)(G - 1) * ks + key_words);
        const u64 *mask = with_mask ? input("mask", (size_t)((nb + md - 1) / md) * LN) : nullptr;
        const u64 *eqp = eq ? input("eqp", (size_t)nb * 4 * MN) : nullptr;
        Out out = output((size_t)nb * 2 * LN);
        launch_relin_mac(dc, N, L, d01, 2 * LN, dig, key, mask, out.data(), nb, st, sm, kp ? sigma_inv : nullptr, ks, G, kp ? pl.lane_T : 0,
                         pl.lane_kp, md, eqp, eq ? M : 0);
        LI_HIP(hipStreamSynchronize(st));
        save("out", out);
    } else if (op == "tensor") {
        const u32 nb = opt("nb", 1);
        if (!nb || N < 8) refuse("nb or N");
        const u64 *e = input("e", (size_t)nb * 4 * MN);
        Out d = output((size_t)nb * 3 * MN);
        launch_tensor(dc, N, M, e, d.data(), nb, st, sm);
        LI_HIP(hipStreamSynchronize(st));
        save("d", d);
    } else if (op == "ntt16_tensor") {
        const u32 nb = opt("nb", 1), eql = opt("eval_q_L");
        const bool d2 = opt("eval_q_d2") != 0;
        if (!nb || !pl.fused_tensor || (eql && (eql != L || !(d2 ? pl.result_eval_q : pl.d01_eval_q))) || (d2 && !eql))
            refuse("ntt16_tensor: no fused tensor product on this context, or eval_q_L / eval_q_d2");
        const u64 *e = input("e", (size_t)nb * 4 * MN);
        Out d = output((size_t)nb * 3 * MN);
        launch_ntt16_tensor(pl, e, d.data(), nb, M, st, eql, d2);
        LI_HIP(hipStreamSynchronize(st));
        save("d", d);
    } else if (op == "deg2_finish") {
        const u32 nb = opt("nb", 1), md = opt("mask_div", 1);
        if (!nb || !md || !sm || !pl.lane_order || !deg2_finish_applies(N, pl.lane_T, pl.lane_kp)) refuse("deg2_finish does not apply");
        const u64 *d = input("d", (size_t)nb * 3 * LN), *eqp = input("eqp", (size_t)nb * 4 * MN);
        const u64 *mask = input("mask", (size_t)((nb + md - 1) / md) * LN);
        Out out = output((size_t)nb * 3 * LN);
        launch_deg2_finish(dc, N, L, d, eqp, M, mask, out.data(), nb, st, pl.lane_T, pl.lane_kp, md);
        LI_HIP(hipStreamSynchronize(st));
        save("out", out);
    } else if (op == "scale_round") {
        const u32 nb = opt("nb", 1);
        const bool c2 = opt("fold_comp2") != 0, p01 = opt("p_only01") != 0, p2 = opt("p_only2") != 0;
        if (!nb || (p01 && !(sm && c2 == p2)) || (p2 && !p01)) refuse("scale_round: p_only01 / p_only2 / fold_comp2");
        const u64 *d = input("d", (size_t)nb * 3 * MN);
        Out o01 = output((size_t)nb * 2 * LN), o2 = output((size_t)nb * LN);
        launch_scale_round(dc, N, L, d, nb, o01.data(), 2 * LN, o2.data(), LN, st, sm, fold, c2, p01, p2);
        LI_HIP(hipStreamSynchronize(st));
        save("out01", o01);
        save("out2", o2);
    } else if (op == "expand_both") {
        const u32 no = opt("n_outer", 1);
        if (!no) refuse("n_outer");
        const u64 *x = input("x", (size_t)no * 2 * LN), *y = input("y", (size_t)no * 2 * LN);
        Out out = output((size_t)no * 4 * MN);
        launch_expand_both(dc, N, L, x, 2 * LN, y, 2 * LN, LN, no, out.data(), st, sm, fold, opt("skip_q") != 0);
        LI_HIP(hipStreamSynchronize(st));
        save("out", out);
    } else if (op == "digits") {
        const u32 nb = opt("nb", 1);
        if (!nb) refuse("nb");
        const u64 *d2 = input("d2", (size_t)nb * LN);
        Out dig = output((size_t)nb * L * LN);
        launch_digits(dc, N, L, d2, LN, nb, dig.data(), st, fold);
        LI_HIP(hipStreamSynchronize(st));
        save("dig", dig);
    } else if (op == "ntt") {
        // forward transform of nlimbs limbs of Q (limb i: modulus i % L), in place; sigma: lane order out; fold; lazy_out
        const u32 nl = opt("nlimbs", L);
        const bool sigma = opt("sigma") != 0, lazy = opt("lazy_out") != 0;
        if (!nl || (sigma && !pl.lane_order)) refuse("nlimbs, or sigma without a lane order");
        const NttRoute r = ntt_route(pl, false, sigma, fold);
        if (lazy && !r.extra()) refuse("lazy_out on a route that does not honour NttExtra");
        printf("route kernel=%s s0=%u global_stages=%u\n", r.kernel == NttKernel::blocked16 ? "blocked16" : r.kernel == NttKernel::blocked32 ? "blocked32" : "radix2",
               r.s0, r.global_stages);
        Out data = output((size_t)nl * N, "data");
        NttExtra ex;
        ex.lazy_out = lazy;
        launch_ntt(pl, data.data(), nl, 0, L, false, st, sigma, fold, &ex);
        LI_HIP(hipStreamSynchronize(st));
        save("data", data);
    } else {
        refuse("unknown OP");
    }
    LI_HIP(hipDeviceSynchronize());
    printf("lazy_inputs_check %s ok\n", op.c_str());
    fflush(stdout);
    (void)piehip_destroy(h);
    return 0;
}
