// dev.h -- device side of the harness: one small kernel per block.  Per-thread operands come from arrays (word k of case i at
// [k n + i]), wave-uniform ones from the kernel argument `c` (scalar registers, as in the product).
#pragma once
#include <hip/hip_runtime.h>

#include "chk_modarith.h"

namespace ac {

#define AC_HIP(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "arith_check: %s: %s\n", #x, hipGetErrorString(e_));       \
            exit(3);                                                                   \
        }                                                                              \
    } while (0)

#define AC_DF(name) \
    struct name {   \
        static __device__ __forceinline__ void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)

template <class F>
__global__ void __launch_bounds__(256) block_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u32 n, Uni c)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) F::go(in, out, n, i, c);
}

// ARITH_CHECK_MODEL_ONLY=1: no device is touched and every output stays 0, so every block fails; what remains true in the report
// are the operand counts and the host model's error histograms (for shaping operand sets where there is no GPU)
static inline bool model_only()
{
    static const bool on = getenv("ARITH_CHECK_MODEL_ONLY") != nullptr;
    return on;
}

// device copies of a set of cases: uploaded once, evaluated with any number of uniform constant groups
struct DevCases {
    Cases &cs;
    u64 *din = nullptr, *dout = nullptr;
    explicit DevCases(Cases &cs_) : cs(cs_)
    {
        if (model_only()) return;
        AC_HIP(hipMalloc(&din, cs.in.size() * sizeof(u64) + 8));
        AC_HIP(hipMalloc(&dout, cs.out.size() * sizeof(u64) + 8));
        AC_HIP(hipMemcpy(din, cs.in.data(), cs.in.size() * sizeof(u64), hipMemcpyHostToDevice));
    }
    ~DevCases()
    {
        if (model_only()) return;
        (void)hipFree(din);
        (void)hipFree(dout);
    }
    template <class F>
    void run(const Uni &c)
    {
        if (model_only()) return;
        AC_HIP(hipMemset(dout, 0xEE, cs.out.size() * sizeof(u64)));
        if (cs.n) hipLaunchKernelGGL((block_kernel<F>), dim3((cs.n + 255) / 256), dim3(256), 0, 0, din, dout, cs.n, c);
        AC_HIP(hipGetLastError());
        AC_HIP(hipDeviceSynchronize());
        AC_HIP(hipMemcpy(cs.out.data(), dout, cs.out.size() * sizeof(u64), hipMemcpyDeviceToHost));
    }
};
template <class F>
static void dev_run(Cases &cs, const Uni &c)
{
    DevCases d(cs);
    d.run<F>(c);
}

// u[0..4]: the Mod (uni_mod); the slots the device blocks add to it
enum { U_NQ = 5, U_N2Q = 6, U_X = 7, U_HAT = 8 };
static inline Uni mod_uni_neg(const Mod &m)
{
    Uni c = mod_uni(m);
    c.u[U_NQ] = 0 - m.q, c.u[U_N2Q] = 0 - 2 * m.q;
    return c;
}

// the groups (one translation unit each: the 16- and 32-coefficient helpers define the same names)
bool group_modarith(const std::vector<ModCase> &mods);
bool group_madasm(const std::vector<ModCase> &mods);
bool group_stage_a(const std::vector<ModCase> &mods);
bool group_pie(const std::vector<ModCase> &mods);
bool group_ntt(const std::vector<ModCase> &mods);
bool group_ntt16(const std::vector<ModCase> &mods);

// a column accumulator that holds z: the normalised split, or one with part of the upper columns pushed down (value unchanged,
// c0, c1 up to 2^63 as after eight multiply-adds)
static inline void columns_of(u128 z, bool spread, Rng &r, u64 &c0, u64 &c1, u64 &c2)
{
    const u64 P30 = 1ull << 30;
    c0 = (u64)(z % P30), c1 = (u64)((z / P30) % P30), c2 = (u64)(z / P60);
    if (!spread) return;
    const u64 t = r.below((c2 < (1ull << 33) ? c2 : (1ull << 33)) + 1);
    c2 -= t, c1 += t * P30;
    const u64 u = r.below((c1 < (1ull << 33) ? c1 : (1ull << 33)) + 1);
    c1 -= u, c0 += u * P30;
}

// the uniform constants w of the 63-bit Shoup blocks: ends, real twiddles, directed ones
// (the directed ones are the last `*nd` entries)
static inline std::vector<u64> uniform_ws(const ModCase &mc, Rng &r, u32 ndirected, size_t *nd = nullptr)
{
    const u64 q = mc.m.q;
    std::vector<u64> ws = {0, 1, q - 1, r.below(q), r.below(q)};
    for (size_t k = 0; k < mc.tw.size() && k < 4; k++) ws.push_back(mc.tw[k]);
    const size_t base = ws.size();
    for (u32 tries = 0, got = 0; got < ndirected && tries < (1u << 24); tries++) {
        u64 w;
        if (directed_w(q, r, w)) ws.push_back(w), got++;
    }
    if (nd) *nd = ws.size() - base;
    return ws;
}

}  // namespace ac
