// chk_bfly.h -- operands and contract of the lazy Harvey butterflies, for the 32-coefficient kernels' C++ form (ct_bfly / gs_bfly)
// and the 16-coefficient kernels' instruction blocks (bfly<INV, SC, H2>):
//   forward  a, b in [0, 8q) -> a' = u + v, b' = u - v + 4q, u = a mod+ 4q, v = b w mod q + k q       (outputs below 8q)
//   inverse  a, b in [0, 4q) -> a' = (a + b) mod+ 4q, b' = d w mod q + k q, d = a - b + 4q             (outputs below 4q)
// with k <= 3 the error of the quotient estimate, which the host model predicts case by case.
#pragma once
#include "dev.h"

namespace ac {

// cases {a, b, w, floor(w 2^63 / q)}; `ws`: the constants to draw w from, the last `nd` of them directed (a uniform-twiddle launch
// overrides w)
static inline void bfly_cases(const ModCase &mc, bool inv, Rng &r, const std::vector<u64> &ws, size_t nd, Cases &cs)
{
    const u64 q = mc.m.q, lim = inv ? 4 * q : 8 * q;
    auto add_w = [&](u64 a, u64 b, u64 w) { cs.add({a, b, w, (u64)(((u128)w * P63) / q)}); };
    auto add = [&](u64 a, u64 b) { add_w(a, b, cs.n % 3 == 2 ? r.below(q) : ws[(cs.n / 3) % ws.size()]); };
    // a and b for the multiplicand d (b forward, d = a - b + 4q inverse)
    auto add_d = [&](u64 d, u64 w) {
        if (!inv) return add_w(r.below(lim), d, w);
        const u64 lo = d < 4 * q ? 4 * q - d : 0, hi = 8 * q - d < 4 * q ? 8 * q - d : 4 * q;
        const u64 b = lo + r.below(hi - lo);
        add_w(d + b - 4 * q, b, w);
    };
    const u64 ends[] = {0, 1, q - 1, q, 2 * q - 1, 2 * q, 4 * q - 1, 4 * q, 4 * q + 1, 8 * q - 1, 8 * q - 2, lim - 1};
    for (int rep = 0; rep < 6; rep++)  // (the constant changes with the case number: every end meets several)
        for (u64 a : ends)
            for (u64 b : ends)
                if (a < lim && b < lim) add(a, b);
    for (u32 i = 0; i < NU / 2; i++) add(r.below(lim), r.below(lim));
    for (u32 i = 0; i < NU / 2; i++) {  // the multiplicand from the directed family
        u64 d;
        if (directed_a(8 * q, r, d) && d != 0) add_d(d, cs.n % 3 == 2 ? r.below(q) : ws[(cs.n / 3) % ws.size()]);
    }
    for (size_t k = ws.size() - nd; k < ws.size(); k++) {  // ... and solved for each directed constant (check.h: ops_solved63)
        std::vector<u64> ds;
        ops_solved63(q, 8 * q, ws[k], 1024, r, ds);
        for (u64 d : ds)
            if (d != 0) add_d(d, ws[k]);
    }
    cs.finish();
}
// outputs (a', b') of case i with the constant w
static inline void bfly_check(Report &rp, bool inv, u64 q, u64 a, u64 b, u64 w, u64 ao, u64 bo)
{
    rp.cases++;
    if (!inv) {
        const u64 u = a >= 4 * q ? a - 4 * q : a;
        const u128 e = model_shoup63_err(b, w, q);
        rp.model_err(e);
        const u64 v = ao - u;
        rp.lazy(v, ref_mulmod(b, w, q), e, 3, "forward: b w of", b, w);
        rp.expect(ao >= u && ao < 8 * q && bo < 8 * q && bo == u + 4 * q - v, "forward (%llu, %llu) w = %llu: got (%llu, %llu)", ULL(a), ULL(b), ULL(w),
                  ULL(ao), ULL(bo));
    } else {
        const u64 s = a + b, d = a + 4 * q - b;
        const u128 e = model_shoup63_err(d, w, q);
        rp.model_err(e);
        rp.lazy(bo, ref_mulmod(d, w, q), e, 3, "inverse: d w of", d, w);
        rp.expect(ao == (s >= 4 * q ? s - 4 * q : s) && bo < 4 * q, "inverse (%llu, %llu) w = %llu: got (%llu, %llu)", ULL(a), ULL(b), ULL(w), ULL(ao),
                  ULL(bo));
    }
}

}  // namespace ac
