// dev_pie.hip -- the helpers of the base conversions (csrc/pie_arith.h): sign-mask subtractions, the 63-bit Shoup blocks, the
// exact high product, the CRT lift.  Constants of the instruction blocks are wave-uniform: one launch per constant.
#include "dev.h"
#include "pie_arith.h"

namespace ac {

// in: x.  uniform: u[U_X] = 2^64 - m.  out: sel_neg(x, x - m), its mask, csub_u(x)
AC_DF(F_sel_neg)
{
    u32 mask;
    const u64 x = AC_IN(0);
    AC_OUT(0) = piehip::sel_neg(x, x + c.u[U_X], mask);
    AC_OUT(1) = mask;
    AC_OUT(2) = piehip::csub_u(x, c.u[U_X]);
} AC_END;
// in: a, w, wsh.  out: divmod_shoup_u, mul_shoup_u, mul_shoup_lazy_u
AC_DF(F_divmod_u)
{
    u64 qt, rm;
    piehip::divmod_shoup_u(AC_IN(0), AC_IN(1), AC_IN(2), c.u[0], c.u[U_NQ], qt, rm);
    AC_OUT(0) = qt, AC_OUT(1) = rm;
    AC_OUT(2) = piehip::mul_shoup_u(AC_IN(0), AC_IN(1), AC_IN(2), c.u[0], c.u[U_NQ]);
    AC_OUT(3) = piehip::mul_shoup_lazy_u(AC_IN(0), AC_IN(1), AC_IN(2), c.u[0]);
} AC_END;
AC_DF(F_reduce123_u) { AC_OUT(0) = piehip::reduce123_u(piehip::U128{AC_IN(1), AC_IN(0)}, uni_mod(c), c.u[U_NQ], c.u[U_N2Q]); } AC_END;
// in: a.  uniform: w = u[U_X], wsh = u[U_HAT].  out: shoup63_lazy, shoup63, divmod63 (quotient, remainder)
AC_DF(F_shoup63)
{
    const u64 a = AC_IN(0), w = c.u[U_X], wsh = c.u[U_HAT], nq = c.u[U_NQ];
    u64 qt, rm;
    AC_OUT(0) = piehip::shoup63_lazy(a, w, wsh, nq);
    AC_OUT(1) = piehip::shoup63(a, w, wsh, nq);
    piehip::divmod63(a, w, wsh, nq, qt, rm);
    AC_OUT(2) = qt, AC_OUT(3) = rm;
} AC_END;
// in: a.  uniform: b = u[U_X]
AC_DF(F_mulhi_sb) { AC_OUT(0) = piehip::mulhi_sb(AC_IN(0), c.u[U_X]); } AC_END;
AC_DF(F_mfixfrac)
{
    const Mod m = uni_mod(c);
    AC_OUT(0) = piehip::mfixfrac<true>(AC_IN(0), m);
    AC_OUT(1) = piehip::mfixfrac<false>(AC_IN(0), m);
} AC_END;
// in: y[NS].  uniform: c[NS] = u[U_HAT ..]
template <u32 NS, bool MAD>
struct F_dot128 {
    static __device__ __forceinline__ void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)
    {
        u64 y[NS], k[NS];
        for (u32 t = 0; t < NS; t++) y[t] = AC_IN(t), k[t] = c.u[U_HAT + t];
        const piehip::U128 v = piehip::dot128<NS, MAD>(y, k);
        AC_OUT(0) = v.lo, AC_OUT(1) = v.hi;
    }
};
// in: y[NS], v.  uniform: hat[NS] = u[U_HAT ..], prodmod = u[U_X]
template <u32 NS, bool MAD, bool LZ>
struct F_crt_out {
    static __device__ __forceinline__ void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)
    {
        u64 y[NS], hat[NS];
        for (u32 t = 0; t < NS; t++) y[t] = AC_IN(t), hat[t] = c.u[U_HAT + t];
        AC_OUT(0) = piehip::crt_out<NS, MAD, LZ>(y, hat, AC_IN(NS), c.u[U_X], uni_mod(c), c.u[U_NQ], c.u[U_N2Q]);
    }
};
// in: c0, c1, v, cc: colacc_mac_small(a, v, cc) on the accumulator {c0, c1, 0}
AC_DF(F_mac_small)
{
    piehip::ColAcc a = {AC_IN(0), AC_IN(1), 0};
    piehip::colacc_mac_small(a, (u32)AC_IN(2), AC_IN(3));
    AC_OUT(0) = a.c0, AC_OUT(1) = a.c1, AC_OUT(2) = a.c2;
} AC_END;

template <u32 NS, bool MAD>
static bool chk_dot(const ModCase &mc)
{
    const u64 q = mc.m.q, lim = MAD ? P60 : ~0ull;
    Rng r(0xD100 + q + NS);
    Report rp((std::string("dot128<") + std::to_string(NS) + (MAD ? ",mad>" : ",mul>")).c_str(), q);
    Cases cs(NS, 2);
    std::vector<u64> row(NS);
    for (u32 i = 0; i < NU / 4; i++) {
        for (u32 t = 0; t < NS; t++) row[t] = i == 0 ? lim - 1 : i == 1 ? 0 : i % 4 == 0 ? lim - 1 - r.below(4) : r.below(lim);
        cs.rows.insert(cs.rows.end(), row.begin(), row.end()), cs.n++;
    }
    cs.finish();
    DevCases d(cs);
    for (int g = 0; g < 3; g++) {
        Uni c = mod_uni_neg(mc.m);
        for (u32 t = 0; t < NS; t++) c.u[U_HAT + t] = g == 0 ? (MAD ? P60 - 1 : (NS > 1 ? ~0ull / NS : ~0ull)) : g == 1 ? q - 1 : r.below(q);
        d.run<F_dot128<NS, MAD>>(c);
        for (u32 i = 0; i < cs.n; i++) {
            rp.cases++;
            u128 want = 0;
            for (u32 t = 0; t < NS; t++) want += (u128)cs.I(t, i) * c.u[U_HAT + t];
            rp.expect(cs.O(0, i) == (u64)want && cs.O(1, i) == (u64)(want >> 64), "case %u, constants %d: differs from the exact sum", i, g);
        }
    }
    return rp.print();
}

template <u32 NS, bool MAD, bool LZ>
static bool chk_crt(const ModCase &mc)
{
    const u64 q = mc.m.q, ylim = MAD ? P60 : (1ull << 61);  // y: residues of the OTHER basis
    Rng r(0xD200 + q + NS * 4 + MAD * 2 + LZ);
    Report rp((std::string("crt_out<") + std::to_string(NS) + (MAD ? ",mad" : ",mul") + (LZ ? ",lazy>" : ">")).c_str(), q);
    Cases cs(NS + 1, 1);
    std::vector<u64> row(NS + 1);
    for (u32 i = 0; i < NU / 4; i++) {
        for (u32 t = 0; t < NS; t++) row[t] = i < 2 ? q - 1 : i == 2 ? ylim - 1 : i == 3 ? 0 : i % 4 == 0 ? ylim - 1 - r.below(4) : r.below(ylim);
        row[NS] = i < 4 ? (i == 1 ? 0 : NS) : r.below(NS + 1);
        cs.rows.insert(cs.rows.end(), row.begin(), row.end()), cs.n++;
    }
    cs.finish();
    DevCases d(cs);
    for (int g = 0; g < 3; g++) {
        Uni c = mod_uni_neg(mc.m);
        for (u32 t = 0; t < NS; t++) c.u[U_HAT + t] = g == 0 ? q - 1 : r.below(q);
        c.u[U_X] = g == 0 ? 1 : g == 1 ? q - 1 : r.below(q);  // prodmod (q - prodmod = q - 1 at g = 0)
        d.run<F_crt_out<NS, MAD, LZ>>(c);
        for (u32 i = 0; i < cs.n; i++) {
            rp.cases++;
            u128 z = (u128)cs.I(NS, i) * (q - c.u[U_X]);
            for (u32 t = 0; t < NS; t++) z += (u128)cs.I(t, i) * c.u[U_HAT + t];
            const u64 want = (u64)(z % q), got = cs.O(0, i);
            if (LZ) {
                const u128 e = model_barrett123_err(z, q);
                rp.model_err(e);
                rp.lazy(got, want, e, 2, "crt_out lazy, case", i, g);
            } else
                rp.expect(got == want, "case %u, constants %d: got %llu, want %llu", i, g, ULL(got), ULL(want));
        }
    }
    if (LZ) rp.need = rp.max_err();
    return rp.print();
}

static bool all(std::initializer_list<bool> v)
{
    bool ok = true;
    for (bool b : v) ok &= b;
    return ok;
}

bool group_pie(const std::vector<ModCase> &mods)
{
    bool ok = true;
    bool first = true;
    for (const ModCase &mc : mods) {
        const u64 q = mc.m.q;
        const Uni um = mod_uni_neg(mc.m);
        if (mc.plaintext) continue;
        {  // sel_neg / csub_u: x in [0, 2m), m = q, 2q, 4q (as far as 2m <= 2^63)
            Report rp("sel_neg/csub_u", q);
            for (u64 m = q; m <= 4 * q && m <= P63 / 2; m *= 2) {
                Rng r(0xD001 + m);
                Cases cs(1, 3);
                for (u64 x : ops_below(2 * m, NU / 2, r, {m - 1, m, m + 1, 2 * m - 1, m / 2})) cs.add({x});
                cs.finish();
                Uni c = um;
                c.u[U_X] = 0 - m;
                dev_run<F_sel_neg>(cs, c);
                for (u32 i = 0; i < cs.n; i++) {
                    rp.cases++;
                    const u64 x = cs.I(0, i), want = x < m ? x : x - m, mask = x < m ? M32 : 0;
                    rp.expect(cs.O(0, i) == want && cs.O(1, i) == mask && cs.O(2, i) == want, "x = %llu, m = %llu: got %llu, mask %llx, csub_u %llu",
                              ULL(x), ULL(m), ULL(cs.O(0, i)), ULL(cs.O(1, i)), ULL(cs.O(2, i)));
                }
            }
            ok &= rp.print();
        }
        {  // divmod_shoup_u (a < q), mul_shoup_u / mul_shoup_lazy_u
            std::vector<u64> A, W;
            shoup_pairs(mc, q, {}, 0xD002 + q, A, W);
            Cases cs(3, 4);
            for (size_t i = 0; i < A.size(); i++) cs.add({A[i], W[i], ref_shoup64(W[i], q)});
            cs.finish();
            dev_run<F_divmod_u>(cs, um);
            Report rp("divmod_shoup_u", q), rs("mul_shoup_u", q), rl("mul_shoup_lazy_u", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++, rs.cases++, rl.cases++;
                const u128 p = (u128)A[i] * W[i];
                const u128 e = model_shoup64_err(A[i], W[i], q);
                rp.model_err(e), rl.model_err(e);
                rp.expect(cs.O(0, i) == (u64)(p / q) && cs.O(1, i) == (u64)(p % q), "%llu * %llu: got (%llu, %llu), want (%llu, %llu)", ULL(A[i]),
                          ULL(W[i]), ULL(cs.O(0, i)), ULL(cs.O(1, i)), ULL((u64)(p / q)), ULL((u64)(p % q)));
                rs.expect(cs.O(2, i) == (u64)(p % q), "%llu * %llu: got %llu, want %llu", ULL(A[i]), ULL(W[i]), ULL(cs.O(2, i)), ULL((u64)(p % q)));
                rl.lazy(cs.O(3, i), (u64)(p % q), e, 1, "mul_shoup_lazy_u", A[i], W[i]);
            }
            rp.need = rl.need = shoup64_canonical_need(q);
            ok &= rp.print();
            ok &= rs.print();
            ok &= rl.print();
        }
        if (mc.w60()) {  // reduce123_u: canonical
            Rng r(0xD007 + q);
            const std::vector<u128> zs = ops_barrett(q, 123, NU, NU, r);
            Cases cs(2, 1);
            for (u128 z : zs) cs.add({(u64)(z >> 64), (u64)z});
            cs.finish();
            dev_run<F_reduce123_u>(cs, um);
            Report rp("reduce123_u", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                rp.model_err(model_barrett123_err(zs[i], q));
                const u64 want = (u64)(zs[i] % q);
                rp.expect(cs.O(0, i) == want, "z = %llu 2^64 + %llu: got %llu, want %llu", ULL(cs.I(0, i)), ULL(cs.I(1, i)), ULL(cs.O(0, i)), ULL(want));
            }
            rp.need = rp.max_err();
            ok &= rp.print();
        }
        if (mc.lt60()) {  // shoup63_lazy, shoup63: a < 2^63;  divmod63: a < q.  One launch per constant w
            Rng r(0xD003 + q);
            std::vector<u64> as = ops_below(P63, NU / 4, r, {q - 1, q, 2 * q - 1, 4 * q - 1, 4 * q, 8 * q - 1, 8 * q});
            for (u64 a : ops_below(q, NU / 4, r)) as.push_back(a);
            for (u32 i = 0; i < NU / 4; i++) {
                u64 a;
                if (directed_a(q, r, a)) as.push_back(a);
                if (directed_a(P63, r, a)) as.push_back(a);
            }
            size_t nd;
            const std::vector<u64> ws = uniform_ws(mc, r, 8, &nd);
            for (size_t k = ws.size() - nd; k < ws.size(); k++)  // operands solved for each directed constant (check.h: ops_solved63)
                ops_solved63(q, q, ws[k], 512, r, as), ops_solved63(q, 8 * q, ws[k], 256, r, as);
            Cases cs(1, 4);
            for (u64 a : as) cs.add({a});
            cs.finish();
            DevCases d(cs);
            Report rl("shoup63_lazy", q), rc("shoup63", q), rd("divmod63", q);
            for (u64 w : ws) {
                Uni c = um;
                c.u[U_X] = w, c.u[U_HAT] = ref_shoup64(w, q);
                d.run<F_shoup63>(c);
                for (u32 i = 0; i < cs.n; i++) {
                    const u64 a = cs.I(0, i);
                    const u128 p = (u128)a * w, e = model_shoup63_err(a, w, q);
                    rl.cases++, rc.cases++;
                    rl.model_err(e);
                    rl.lazy(cs.O(0, i), (u64)(p % q), e, 3, "shoup63_lazy", a, w);
                    rc.expect(cs.O(1, i) == (u64)(p % q), "%llu * %llu: got %llu, want %llu", ULL(a), ULL(w), ULL(cs.O(1, i)), ULL((u64)(p % q)));
                    if (a < q) {
                        rd.cases++;
                        rd.model_err(e);
                        rd.expect(cs.O(2, i) == (u64)(p / q) && cs.O(3, i) == (u64)(p % q), "%llu * %llu: got (%llu, %llu), want (%llu, %llu)", ULL(a),
                                  ULL(w), ULL(cs.O(2, i)), ULL(cs.O(3, i)), ULL((u64)(p / q)), ULL((u64)(p % q)));
                    }
                }
            }
            memcpy(rc.err, rl.err, sizeof rc.err);  // shoup63 is the same estimate on the same operands, reduced
            rl.need = rc.need = mc.w60() ? 3 : rl.max_err();
            rd.need = mc.w60() ? 3 : rd.max_err();
            ok &= rl.print();
            ok &= rc.print();
            ok &= rd.print();
        }
        if (first) {  // mulhi_sb: modulus-free (b wave-uniform); reported once
            first = false;
            Rng r(0xD004);
            const u64 t64 = ~0ull;
            std::vector<u64> pts = {0, 1, M32, P32, P32 + 1, t64, t64 - 1, t64 - M32, P63, P63 - 1, P32 - 2, (M32 << 32) | 1};
            Cases cs(1, 1);
            for (u64 a : pts) cs.add({a});
            for (u32 i = 0; i < NU / 4; i++) cs.add({r.next()});
            for (u32 i = 0; i < NU / 4; i++) cs.add({(r.next() & ~M32) | (M32 - r.below(4))});  // cross sums that carry
            cs.finish();
            DevCases d(cs);
            std::vector<u64> bs = pts;
            bs.push_back(mc.m.fconst), bs.push_back((mc.m.r1 << 59) | (mc.m.r0 >> 5));
            for (int i = 0; i < 4; i++) bs.push_back(r.next());
            for (int i = 0; i < 4; i++) bs.push_back((r.next() & ~M32) | (M32 - r.below(4)));
            Report rp("mulhi_sb", 0);
            for (u64 b : bs) {
                Uni c = um;
                c.u[U_X] = b;
                d.run<F_mulhi_sb>(c);
                for (u32 i = 0; i < cs.n; i++) {
                    rp.cases++;
                    const u64 want = (u64)(((u128)cs.I(0, i) * b) / (ONE << 64));
                    rp.expect(cs.O(0, i) == want, "%llu * %llu: got %llu, want %llu", ULL(cs.I(0, i)), ULL(b), ULL(cs.O(0, i)), ULL(want));
                }
            }
            ok &= rp.print();
        }
        {  // mfixfrac<true / false>: the contract of fixfrac
            Rng r(0xD005 + q);
            Cases cs(1, 2);
            for (u64 y : ops_below(q, NU, r, {q / 2, q / 2 + 1, q / 3})) cs.add({y});
            cs.finish();
            dev_run<F_mfixfrac>(cs, um);
            Report rp("mfixfrac<asm>,<c>", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                const u128 rhs = (u128)cs.I(0, i) * P60;
                bool good = cs.O(0, i) == cs.O(1, i);
                const u128 lhs = (u128)cs.O(0, i) * q;
                good &= cs.O(0, i) <= P60 && (lhs > rhs ? lhs - rhs : rhs - lhs) < 2 * (u128)q;
                rp.expect(good, "y = %llu: got %llu (asm), %llu (c)", ULL(cs.I(0, i)), ULL(cs.O(0, i)), ULL(cs.O(1, i)));
            }
            ok &= rp.print();
        }
        {  // colacc_mac_small: v < 2^30 times a residue, on columns that already hold seven terms
            Rng r(0xD006 + q);
            Cases cs(4, 3);
            for (u32 i = 0; i < NU / 4; i++)
                cs.add({i % 2 ? r.below(7 * P60) : 7 * (P60 - 1), i % 2 ? r.below(14 * P60) : 14 * (P60 - 1), i < 16 ? i % 9 : i % 4 == 0 ? (1u << 30) - 1 : r.below(1u << 30),
                        i % 3 ? r.below(q) : q - 1});
            cs.finish();
            dev_run<F_mac_small>(cs, um);
            Report rp("colacc_mac_small", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                const u128 want = (u128)cs.I(0, i) + (u128)cs.I(1, i) * (1ull << 30) + (u128)cs.I(2, i) * cs.I(3, i);
                const u128 got = (u128)cs.O(0, i) + (u128)cs.O(1, i) * (1ull << 30) + (u128)cs.O(2, i) * P60;
                rp.expect(got == want, "case %u: v = %llu, c = %llu: value differs", i, ULL(cs.I(2, i)), ULL(cs.I(3, i)));
            }
            ok &= rp.print();
        }
        // dot128 / crt_out: the multiply forms for every modulus, the column forms and the lazy ones for those of (2^59, 2^60)
        ok &= all({chk_dot<1, false>(mc), chk_dot<2, false>(mc), chk_dot<4, false>(mc), chk_dot<7, false>(mc), chk_dot<8, false>(mc)});
        ok &= all({chk_crt<1, false, false>(mc), chk_crt<2, false, false>(mc), chk_crt<4, false, false>(mc), chk_crt<7, false, false>(mc),
                   chk_crt<8, false, false>(mc)});
        if (mc.w60()) {
            ok &= all({chk_dot<1, true>(mc), chk_dot<2, true>(mc), chk_dot<4, true>(mc), chk_dot<7, true>(mc), chk_dot<8, true>(mc)});
            ok &= all({chk_crt<1, true, false>(mc), chk_crt<2, true, false>(mc), chk_crt<4, true, false>(mc), chk_crt<7, true, false>(mc),
                       chk_crt<8, true, false>(mc)});
            ok &= all({chk_crt<1, true, true>(mc), chk_crt<2, true, true>(mc), chk_crt<4, true, true>(mc), chk_crt<7, true, true>(mc)});
        }
    }
    return ok;
}

}  // namespace ac
