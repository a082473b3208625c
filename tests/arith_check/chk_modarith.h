// chk_modarith.h -- the contracts of csrc/modarith.h against exact integers, for whoever evaluates the blocks (RunFn): the host
// pass in host_check.cpp, the device pass in dev_mod.hip.  Same operand sets, same reference.
#pragma once
#include "f_modarith.h"

namespace ac {

#define ULL(x) ((unsigned long long)(x))
static const u32 NU = 1u << 16;  // cases per operand family

// (a, w) pairs of a Shoup-type block: corners x {0, 1, q - 1, real twiddles}, uniform pairs, the directed family
static inline void shoup_pairs(const ModCase &mc, u64 alim, std::initializer_list<u64> acorners, u64 seed, std::vector<u64> &A,
                               std::vector<u64> &W)
{
    const u64 q = mc.m.q;
    Rng r(seed);
    std::vector<u64> ws = {0, 1, q - 1, q - 2};
    ws.insert(ws.end(), mc.tw.begin(), mc.tw.end());
    std::vector<u64> as = {0, 1, alim - 1, alim - 2};
    for (u64 a : acorners)
        if (a < alim) as.push_back(a);
    for (u64 a : as)
        for (u64 w : ws) A.push_back(a), W.push_back(w);
    for (u32 i = 0; i < NU; i++) A.push_back(r.below(alim)), W.push_back(r.below(q));
    for (u32 i = 0; i < NU / 4; i++) A.push_back(r.below(alim)), W.push_back(mc.tw.empty() ? r.below(q) : mc.tw[i % mc.tw.size()]);
    ops_directed(q, alim, NU, r, A, W);
    // (just above 2^32 one draw in a thousand qualifies: s = 1 and both a / q and frac(w 2^64 / q) within 10^-3 of 1)
    if (alim <= q) ops_directed64(q, q < (1ull << 34) ? 8 * NU : NU / 4, r, A, W);
}

// largest error of the 64-bit Shoup estimate on canonical operands: 1 needs a w mod q < a frac(w 2^64 / q) q / 2^64 < q^2 / 2^64,
// which below 2^32 leaves only a w = 0 (mod q), where nothing is lost
static inline int shoup64_canonical_need(u64 q) { return q < P32 ? 0 : 1; }

static inline bool chk_modarith(RunFn run, const ModCase &mc)
{
    const Mod &m = mc.m;
    const u64 q = m.q;
    const Uni uc = mod_uni(m);
    bool ok = true;

    if (!mc.tw.empty()) {  // the real twiddles' Shoup companions, as HostParams::init computed them
        Report rp("shoup_companions", q);
        for (size_t k = 0; k < mc.tw.size(); k++) {
            rp.cases++;
            rp.expect(mc.tw[k] < q && mc.tw_sh[k] == ref_shoup64(mc.tw[k], q), "w = %llu: companion %llu, want %llu", ULL(mc.tw[k]), ULL(mc.tw_sh[k]),
                      ULL(ref_shoup64(mc.tw[k], q)));
        }
        ok &= rp.print();
    }

    {  // barrett128, mulmod: any z < 2^128
        Rng r(0xA001 + q);
        Cases cs(2, 1);
        const u128 top = ~(u128)0;
        std::vector<u128> zs = {0, 1, q - 1, q, top, top - 1, top - top % q, top - top % q - 1};
        for (u32 i = 0; i < NU; i++) zs.push_back((((u128)r.next()) << 64) | r.next());
        for (u32 i = 0; i < NU / 2; i++) {
            const u128 k = (top / q) / 2 + r.below128((top / q) / 2);
            zs.push_back(k * q), zs.push_back(k * q - 1);
        }
        for (u128 z : zs) cs.add({(u64)(z >> 64), (u64)z});
        cs.finish();
        run(B_BARRETT128, cs, uc);
        Report rp("barrett128", q);
        for (u32 i = 0; i < cs.n; i++) {
            rp.cases++;
            const u64 want = (u64)(zs[i] % q);
            rp.model_err(model_barrett128_err(zs[i], q));
            rp.expect(cs.O(0, i) == want, "z = %llu 2^64 + %llu: got %llu, want %llu", ULL(cs.I(0, i)), ULL(cs.I(1, i)), ULL(cs.O(0, i)),
                      ULL(want));
        }
        rp.need = 1;  // the only loss is z frac(2^128 / q) / 2^128 < 1; every multiple of q attains it
        ok &= rp.print();

        Cases cm(2, 1);
        const u64 t64 = ~0ull;
        const u64 ends[] = {0, 1, q - 1, q, t64, t64 - 1};
        for (u64 a : ends)
            for (u64 b : ends) cm.add({a, b});
        for (u32 i = 0; i < NU; i++) cm.add({r.next(), r.next()});
        for (u32 i = 0; i < NU; i++) cm.add({r.below(q), r.below(q)});
        for (u32 i = 0; i < NU / 4; i++) cm.add({(1 + r.below(t64 / q)) * q, r.next()});  // products that are multiples of q
        cm.finish();
        run(B_MULMOD, cm, uc);
        Report rm("mulmod", q);
        for (u32 i = 0; i < cm.n; i++) {
            rm.cases++;
            const u64 want = ref_mulmod(cm.I(0, i), cm.I(1, i), q);
            rm.model_err(model_barrett128_err((u128)cm.I(0, i) * cm.I(1, i), q));
            rm.expect(cm.O(0, i) == want, "%llu * %llu: got %llu, want %llu", ULL(cm.I(0, i)), ULL(cm.I(1, i)), ULL(cm.O(0, i)), ULL(want));
        }
        rm.need = 1;
        ok &= rm.print();
    }

    if (mc.w60()) {  // reduce123 / reduce124: canonical result; the estimate's error from the host model
        for (int bits = 123; bits <= 124; bits++) {
            Rng r(0xA002 + q + bits);
            const std::vector<u128> zs = ops_barrett(q, bits, NU, NU, r);
            Cases cs(2, 1);
            for (u128 z : zs) cs.add({(u64)(z >> 64), (u64)z});
            cs.finish();
            run(bits == 123 ? B_REDUCE123 : B_REDUCE124, cs, uc);
            Report rp(bits == 123 ? "reduce123" : "reduce124", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                u128 rem;
                rp.model_err(bits == 123 ? model_barrett123_err(zs[i], q) : model_barrett124_err(zs[i], q, &rem));
                const u64 want = (u64)(zs[i] % q);
                rp.expect(cs.O(0, i) == want, "z = %llu 2^64 + %llu: got %llu, want %llu", ULL(cs.I(0, i)), ULL(cs.I(1, i)),
                          ULL(cs.O(0, i)), ULL(want));
            }
            rp.need = rp.max_err();  // the directed family is built to attain the largest error this modulus allows
            ok &= rp.print();
        }
    }

    {  // mul_shoup_lazy / mul_shoup: any a < 2^64;  divmod_shoup: a < q
        std::vector<u64> A, W;
        shoup_pairs(mc, ~0ull, {q - 1, q, 2 * q - 1, 2 * q, P63 - 1, P63}, 0xA003 + q, A, W);
        Cases cs(3, 1), cc(3, 1);
        for (size_t i = 0; i < A.size(); i++) cs.add({A[i], W[i], ref_shoup64(W[i], q)}), cc.add({A[i], W[i], ref_shoup64(W[i], q)});
        cs.finish(), cc.finish();
        run(B_SHOUP_LAZY, cs, uc);
        run(B_SHOUP, cc, uc);
        Report rl("mul_shoup_lazy", q), rc("mul_shoup", q);
        for (u32 i = 0; i < cs.n; i++) {
            rl.cases++, rc.cases++;
            const u64 want = ref_mulmod(A[i], W[i], q);
            const u128 e = model_shoup64_err(A[i], W[i], q);
            rl.model_err(e);
            rl.lazy(cs.O(0, i), want, e, 1, "mul_shoup_lazy", A[i], W[i]);
            rc.expect(cc.O(0, i) == want, "%llu * %llu: got %llu, want %llu", ULL(A[i]), ULL(W[i]), ULL(cc.O(0, i)), ULL(want));
        }
        rl.need = 1;
        ok &= rl.print();
        ok &= rc.print();

        std::vector<u64> A2, W2;
        shoup_pairs(mc, q, {}, 0xA004 + q, A2, W2);
        Cases cd(3, 2);
        for (size_t i = 0; i < A2.size(); i++) cd.add({A2[i], W2[i], ref_shoup64(W2[i], q)});
        cd.finish();
        run(B_DIVMOD, cd, uc);
        Report rd("divmod_shoup", q);
        for (u32 i = 0; i < cd.n; i++) {
            rd.cases++;
            const u128 p = (u128)A2[i] * W2[i];
            rd.model_err(model_shoup64_err(A2[i], W2[i], q));
            rd.expect(cd.O(0, i) == (u64)(p / q) && cd.O(1, i) == (u64)(p % q), "%llu * %llu: got (%llu, %llu), want (%llu, %llu)", ULL(A2[i]),
                      ULL(W2[i]), ULL(cd.O(0, i)), ULL(cd.O(1, i)), ULL((u64)(p / q)), ULL((u64)(p % q)));
        }
        rd.need = shoup64_canonical_need(q);
        ok &= rd.print();
    }

    {  // fixfrac: | f / 2^60 - y / q | < 2^-59  <=>  | f q - y 2^60 | < 2 q
        Rng r(0xA005 + q);
        Cases cs(1, 1);
        for (u64 y : ops_below(q, NU, r, {q / 2, q / 2 + 1, q / 3})) cs.add({y});
        cs.finish();
        run(B_FIXFRAC, cs, uc);
        Report rp("fixfrac", q);
        for (u32 i = 0; i < cs.n; i++) {
            rp.cases++;
            const u128 lhs = (u128)cs.O(0, i) * q, rhs = (u128)cs.I(0, i) * P60;
            const u128 d = lhs > rhs ? lhs - rhs : rhs - lhs;
            rp.expect(cs.O(0, i) <= P60 && d < 2 * (u128)q, "y = %llu: got %llu, | f q - y 2^60 | >= 2 q", ULL(cs.I(0, i)), ULL(cs.O(0, i)));
        }
        ok &= rp.print();
    }

    if (!mc.plaintext) {  // add128 / mac128 (modulus-free: reported under the modulus they ran beside)
        Rng r(0xA006);
        const u64 t64 = ~0ull;
        Cases ca(4, 2), cm(4, 2);
        const u64 pts[] = {0, 1, t64, t64 - 1, P63, P32, M32};
        for (u64 a : pts)
            for (u64 b : pts)
                for (u64 c : pts) ca.add({a, b % P63, c, a % P63}), cm.add({a, b % P60, c, b});
        for (u32 i = 0; i < NU; i++) ca.add({r.next(), r.next() % P63, r.next(), r.next() % P63}), cm.add({r.next(), r.next() % P60, r.next(), r.next()});
        ca.finish(), cm.finish();
        run(B_ADD128, ca, uc);
        run(B_MAC128, cm, uc);
        Report ra("add128", q), rm("mac128", q);
        for (u32 i = 0; i < ca.n; i++) {
            ra.cases++, rm.cases++;
            const u128 s = ((((u128)ca.I(1, i)) << 64) | ca.I(0, i)) + ((((u128)ca.I(3, i)) << 64) | ca.I(2, i));
            ra.expect(ca.O(0, i) == (u64)s && ca.O(1, i) == (u64)(s >> 64), "case %u: got %llu 2^64 + %llu", i, ULL(ca.O(1, i)), ULL(ca.O(0, i)));
            const u128 t = ((((u128)cm.I(1, i)) << 64) | cm.I(0, i)) + (u128)cm.I(2, i) * cm.I(3, i);
            rm.expect(cm.O(0, i) == (u64)t && cm.O(1, i) == (u64)(t >> 64), "case %u: got %llu 2^64 + %llu", i, ULL(cm.O(1, i)), ULL(cm.O(0, i)));
        }
        ok &= ra.print();
        ok &= rm.print();
    }
    return ok;
}

}  // namespace ac
