// dev_ntt.hip -- the 32-coefficient transform's helpers (csrc/ntt_bfly.h): shoup4, ct_bfly, gs_bfly, lift_digit.
#include "chk_bfly.h"
#include "ntt_bfly.h"

namespace ac {

// in: b, w, floor(w 2^63 / q)
AC_DF(F_shoup4) { AC_OUT(0) = piehip::shoup4(AC_IN(0), AC_IN(1), AC_IN(2), c.u[U_NQ]); } AC_END;
// in: a, b, w, floor(w 2^63 / q)
AC_DF(F_ct_bfly)
{
    u64 a = AC_IN(0), b = AC_IN(1);
    piehip::ct_bfly(a, b, AC_IN(2), AC_IN(3), c.u[U_NQ], 4 * c.u[0]);
    AC_OUT(0) = a, AC_OUT(1) = b;
} AC_END;
AC_DF(F_gs_bfly)
{
    u64 a = AC_IN(0), b = AC_IN(1);
    piehip::gs_bfly(a, b, AC_IN(2), AC_IN(3), c.u[U_NQ], 4 * c.u[0]);
    AC_OUT(0) = a, AC_OUT(1) = b;
} AC_END;
// in: v.  uniform: the Mod of q_j, u[U_X] = q_i, u[U_HAT] = q_i mod q_j
AC_DF(F_lift_digit) { AC_OUT(0) = piehip::lift_digit(AC_IN(0), c.u[U_X], c.u[U_HAT], uni_mod(c)); } AC_END;

bool group_ntt(const std::vector<ModCase> &mods)
{
    bool ok = true;
    for (const ModCase &mc : mods) {
        if (mc.plaintext || !mc.lt60()) continue;  // the lazy transforms: every modulus below 2^60
        const u64 q = mc.m.q;
        const Uni um = mod_uni_neg(mc.m);
        {  // shoup4: b < 2^63, result below 4q and congruent
            std::vector<u64> B, W;
            shoup_pairs(mc, P63, {q - 1, q, 4 * q - 1, 4 * q, 8 * q - 1, 8 * q}, 0xE001 + q, B, W);
            Rng r(0xE002 + q);
            ops_directed(q, q, NU, r, B, W);  // ... and the directed family with canonical operands
            size_t nd;
            const std::vector<u64> pool = uniform_ws(mc, r, 8, &nd);  // (below 2^59 few w qualify: searched for, then shared)
            for (u32 i = 0; i < NU / 2 && nd; i++) {
                u64 b;
                if (directed_a(i % 2 ? P63 : 8 * q, r, b)) B.push_back(b), W.push_back(pool[pool.size() - 1 - i % nd]);
            }
            for (size_t k = pool.size() - nd; k < pool.size(); k++)
                for (u64 lim : {q, 8 * q}) {
                    std::vector<u64> bs;
                    ops_solved63(q, lim, pool[k], 256, r, bs);
                    for (u64 b : bs) B.push_back(b), W.push_back(pool[k]);
                }
            Cases cs(3, 1);
            for (size_t i = 0; i < B.size(); i++) cs.add({B[i], W[i], (u64)(((u128)W[i] * P63) / q)});
            cs.finish();
            dev_run<F_shoup4>(cs, um);
            Report rp("shoup4", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                const u128 e = model_shoup63_err(B[i], W[i], q);
                rp.model_err(e);
                rp.lazy(cs.O(0, i), ref_mulmod(B[i], W[i], q), e, 3, "shoup4", B[i], W[i]);
            }
            rp.need = mc.w60() ? 3 : rp.max_err();
            ok &= rp.print();
        }
        for (int inv = 0; inv < 2; inv++) {
            Rng r(0xE003 + q + inv);
            Cases cs(4, 2);
            size_t nd;
            const std::vector<u64> ws = uniform_ws(mc, r, 8, &nd);
            bfly_cases(mc, inv, r, ws, nd, cs);
            if (inv)
                dev_run<F_gs_bfly>(cs, um);
            else
                dev_run<F_ct_bfly>(cs, um);
            Report rp(inv ? "gs_bfly" : "ct_bfly", q);
            for (u32 i = 0; i < cs.n; i++) bfly_check(rp, inv, q, cs.I(0, i), cs.I(1, i), cs.I(2, i), cs.O(0, i), cs.O(1, i));
            rp.need = mc.w60() ? 3 : rp.max_err();
            ok &= rp.print();
        }
    }
    // lift_digit: every ordered pair of chain moduli, both branches (q_i < 2 q_j and q_i >= 2 q_j)
    Report near("lift_digit<qi<2qj>", 0), far("lift_digit<qi>=2qj>", 0);
    for (const ModCase &mi : mods)
        for (const ModCase &mj : mods) {
            if (mi.plaintext || mj.plaintext || mi.m.q == mj.m.q) continue;
            const u64 qi = mi.m.q, qj = mj.m.q;
            Rng r(0xE004 + qi + 3 * qj);
            Cases cs(1, 1);
            for (u64 v : ops_below(qi, 2048, r, {qi / 2, qi / 2 + 1, qi / 2 - 1, qj - 1, qj, qj + 1, 2 * qj - 1, 2 * qj})) cs.add({v});
            cs.finish();
            Uni c = mod_uni_neg(mj.m);
            c.u[U_X] = qi, c.u[U_HAT] = qi % qj;
            dev_run<F_lift_digit>(cs, c);
            Report &rp = qi < 2 * qj ? near : far;
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                const u64 v = cs.I(0, i);
                const u64 want = v > qi / 2 ? (u64)(((u128)(v % qj) + qj - qi % qj) % qj) : v % qj;  // v - q_i (mod q_j) above q_i / 2
                rp.expect(cs.O(0, i) == want, "v = %llu, q_i = %llu, q_j = %llu: got %llu, want %llu", ULL(v), ULL(qi), ULL(qj), ULL(cs.O(0, i)), ULL(want));
            }
        }
    ok &= near.print();
    ok &= far.print();
    return ok;
}

}  // namespace ac
