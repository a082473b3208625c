// lazy_inputs_check OP DIR N L t q_0 .. q_{L-1} p_0 .. p_L [name=value ...]
// One launch of ONE kernel of the product chain on arrays the caller gives, so that a test can hand it the ends of its lazy input
// range -- representatives that the transforms inside the library produce with negligible probability (tests/lazy_inputs.py,
// tests/test_gpu_lazy_inputs.py).  A program of its own, linked with the library's objects: it makes a handle with piehip_create,
// takes the constants, the plan and the lane-order map from it and calls one piehip::launch_* of kernels.hpp.  It judges nothing.
// The ops `ntt` and `ntt_digits` launch the transforms themselves, every route and NttExtra mode (tests/transform_inputs.py,
// tests/test_gpu_transform_routes.py); they print a line "route ..." with the kernel, the slices and the global stages of the call.
//
// Inputs are DIR/in_<name>.u64 (raw little-endian words, exactly the words the launch indexes: any other size is refused), outputs
// DIR/out_<name>.u64: GUARD words, the array, GUARD words, everything pre-filled with FILL so that guards and places a mode does not
// write can be told from written ones (FILL has its top bit set: no residue below 2^63 equals it).  DIR/out_sigma_inv.u64 is the
// handle's lane-order map, one word per position.  The line "plan ..." says what the context decided.
// fd= picks the reduction kind of the kernels that have two (kernels.hpp: Arith) -- scale_round, expand_both, ntt16_tensor: absent, the
// plan's; fd=0 the Barrett kernels, valid on every small_moduli context; fd=1 the folded ones, refused where the plan has no
// fold_moduli.  Those ops print "route ... reduction=wide|barrett|fold": the kind that ran.
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
    printf("plan lane_order=%d fold=%d lane_kp=%u lane_T=%u small_moduli=%d fold_moduli=%d fused_tensor=%d d01_eval_q=%d result_eval_q=%d xq_reuse=%d x_direct=%d "
           "digits_with_d01=%d digit_lift_lane=%d digit_lift_std=%d\n",
           (int)pl.lane_order, (int)pl.fold, pl.lane_kp, pl.lane_T, (int)sm, (int)pl.fold_moduli, (int)pl.fused_tensor, (int)pl.d01_eval_q, (int)pl.result_eval_q,
           (int)pl.xq_reuse, (int)pl.x_direct, (int)pl.digits_with_d01, (int)pl.digit_lift_lane, (int)pl.digit_lift_std);
    {
        std::vector<u32> m32(N);
        LI_HIP(hipMemcpy(m32.data(), sigma_inv, (size_t)N * sizeof(u32), hipMemcpyDeviceToHost));
        save_words("sigma_inv", std::vector<u64>(m32.begin(), m32.end()));
    }
    const size_t LN = (size_t)L * N, MN = (size_t)M * N;
    const bool fold = opt("fold") != 0;
    if (fold && !pl.fold) refuse("fold on a ring whose transforms are not folded");
    // the reduction kind of the ops that have two: the plan's unless fd= says otherwise
    const bool fd = g_opt.count("fd") ? opt("fd") != 0 : pl.fold_moduli;
    if (fd && !pl.fold_moduli) refuse("fd=1 on a context whose moduli do not take the folded reduction");
    const Arith ar(sm, fd);
    const char *const kind = !ar.mad ? "wide" : ar.fold ? "fold" : "barrett";

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
        NttPlan tpl = pl;   // the launcher takes the kind from the plan
        tpl.fold_moduli = fd;
        printf("route reduction=%s\n", tpl.fold_moduli ? "fold" : "barrett");
        launch_ntt16_tensor(tpl, e, d.data(), nb, M, st, eql, d2);
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
        printf("route reduction=%s\n", kind);
        launch_scale_round(dc, N, L, d, nb, o01.data(), 2 * LN, o2.data(), LN, st, ar, fold, c2, p01, p2);
        LI_HIP(hipStreamSynchronize(st));
        save("out01", o01);
        save("out2", o2);
    } else if (op == "expand_both") {
        const u32 no = opt("n_outer", 1);
        if (!no) refuse("n_outer");
        const u64 *x = input("x", (size_t)no * 2 * LN), *y = input("y", (size_t)no * 2 * LN);
        Out out = output((size_t)no * 4 * MN);
        printf("route reduction=%s\n", kind);
        if (!launch_expand_both(dc, N, L, x, 2 * LN, y, 2 * LN, LN, no, out.data(), st, ar, fold, opt("skip_q") != 0))
            refuse("expand_both: a combination the launcher is not built for");
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
        // one transform launch, in place, of nlimbs limbs (limb i: modulus mod_base + i % mod_count; default 0 and L) at the head of an
        // array of data_limbs limbs (default nlimbs: what lies behind the last item must come back as it went in).  inverse; sigma: the
        // EVALUATION side in lane order; fold; lazy_out.  The NttExtra modes, with nb bins:
        //   copy=1 copy_K=   inverse, standard order in: data [nb][copy_K][2][L][N], copy_out [nb][4][M][N] an output of its own;
        //                    x_lane_in=1: that array comes from in_copy.u64
        //   skip=1           forward: data [nb][4][M][N], nlimbs the compact count nb (2 (M - L) + 2 M)
        //   digits=1         forward, lane order: Ntt16Digits rides along, in_d2.u64 [nb][L][N] -> dig [nb][L][L][N]
        // An NttExtra is passed whether or not the route honours it: the route line says which, the caller looks at the arrays.
        const u32 nl = opt("nlimbs", L), mod_base = opt("mod_base", 0), mod_count = opt("mod_count", L), nb = opt("nb", 1);
        const bool sigma = opt("sigma") != 0, lazy = opt("lazy_out") != 0, inverse = opt("inverse") != 0;
        const bool copy = opt("copy") != 0, x_lane_in = opt("x_lane_in") != 0, skip = opt("skip") != 0, digits = opt("digits") != 0;
        const u32 data_limbs = opt("data_limbs", skip ? nb * 4 * M : nl), copy_K = opt("copy_K", 1);
        if (!nl || !nb || data_limbs < nl || (sigma && !pl.lane_order)) refuse("nlimbs, nb, data_limbs, or sigma without a lane order");
        if (!mod_count || mod_base + mod_count > M + 1) refuse("mod_base / mod_count leave the context's moduli");
        const NttRoute r = ntt_route(pl, inverse, sigma, fold);
        if (lazy && (!r.extra() || inverse || !sigma)) refuse("lazy_out on a call that does not honour it");
        if (copy && (!inverse || sigma || !copy_K || nl != nb * copy_K * 2 * L || mod_base || mod_count != L)) refuse("copy: an inverse in standard order over [nb][copy_K][2][L]");
        if (x_lane_in && (!copy || !pl.x_direct || r.kernel != NttKernel::blocked16)) refuse("x_lane_in without copy, or on a plan without x_direct");
        if (skip && (inverse || mod_base || mod_count != M || nl != nb * (2 * (M - L) + 2 * M) || data_limbs < nb * 4 * M)) refuse("skip: a forward call over [nb][4][M]");
        if (digits && (inverse || !sigma || fold != pl.fold || mod_base || mod_count != L || !pl.digits_with_d01 || r.kernel != NttKernel::blocked16))
            refuse("digits on a plan without digits_with_d01, or not on its forward lane-order launch");
        if (opt("slots") && piehip_set_transform_slots(h, opt("slots")) != PIEHIP_OK) refuse("piehip_set_transform_slots");
        printf("route kernel=%s s0=%u global_stages=%u extra=%d transform_cus=%u\n",
               r.kernel == NttKernel::blocked16 ? "blocked16" : r.kernel == NttKernel::blocked32 ? "blocked32" : "radix2", r.s0, r.global_stages, (int)r.extra(),
               pl.transform_cus());
        Out data = output((size_t)data_limbs * N, "data");
        Out cp, dig;
        NttExtra ex;
        ex.lazy_out = lazy;
        if (copy) {
            cp = output((size_t)nb * 4 * MN, x_lane_in ? "copy" : nullptr);
            ex.copy_out = cp.data(), ex.copy_K = copy_K, ex.copy_L = L, ex.copy_M = M, ex.x_lane_in = x_lane_in;
        }
        if (skip) ex.skip_L = L, ex.skip_M = M;
        if (digits) {
            const u64 *d2 = input("d2", (size_t)nb * LN);
            dig = output((size_t)nb * L * LN);
            Ntt16Digits dg = {d2, LN, dig.data(), nb, L};
            launch_ntt16(pl, data.data(), nl, 0, L, false, true, st, &ex, &dg);
        } else {
            launch_ntt(pl, data.data(), nl, mod_base, mod_count, inverse, st, sigma, fold, &ex);
        }
        LI_HIP(hipStreamSynchronize(st));
        save("data", data);
        if (copy) save("copy", cp);
        if (digits) save("dig", dig);
    } else if (op == "ntt_digits") {
        // launch_ntt_digits: in_d2.u64 [nb][L][N] COEFFICIENT -> dig [nb][L][L][N] EVALUATION, the lift in the 32-coefficient kernel's load phase
        const u32 nb = opt("nb", 1);
        const bool sigma = opt("sigma") != 0;
        if (!nb || !(sigma ? pl.digit_lift_lane : pl.digit_lift_std)) refuse("ntt_digits: nb, or the plan has no digit lift in this order");
        if (opt("slots") && piehip_set_transform_slots(h, opt("slots")) != PIEHIP_OK) refuse("piehip_set_transform_slots");
        const NttRoute r = ntt_route(pl, false, sigma, false);
        printf("route kernel=%s s0=%u global_stages=%u extra=%d transform_cus=%u\n",
               r.kernel == NttKernel::blocked16 ? "blocked16" : r.kernel == NttKernel::blocked32 ? "blocked32" : "radix2", r.s0, r.global_stages, (int)r.extra(),
               pl.transform_cus());
        const u64 *d2 = input("d2", (size_t)nb * LN);
        Out dig = output((size_t)nb * L * LN);
        launch_ntt_digits(pl, d2, dig.data(), nb, L, sigma, st);
        LI_HIP(hipStreamSynchronize(st));
        save("dig", dig);
    } else {
        refuse("unknown OP");
    }
    LI_HIP(hipDeviceSynchronize());
    printf("lazy_inputs_check %s ok\n", op.c_str());
    fflush(stdout);
    (void)piehip_destroy(h);
    return 0;
}
