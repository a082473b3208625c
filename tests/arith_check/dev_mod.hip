// dev_mod.hip -- the device pass of csrc/modarith.h (the checks of chk_modarith.h), the column accumulators of csrc/madasm.h and
// the epilogue blocks of csrc/stage_a_common.h.
#include "dev.h"
#include "stage_a_common.h"

namespace ac {

using piehip::ColAcc;
using piehip::split30;

// ---- modarith.h ----------------------------------------------------------------------------------------------------------------
static void dev_modarith_run(int id, Cases &cs, const Uni &c)
{
    switch (id) {
    case B_BARRETT128: return dev_run<F_barrett128>(cs, c);
    case B_MULMOD: return dev_run<F_mulmod>(cs, c);
    case B_REDUCE123: return dev_run<F_reduce123>(cs, c);
    case B_REDUCE124: return dev_run<F_reduce124>(cs, c);
    case B_SHOUP_LAZY: return dev_run<F_shoup_lazy>(cs, c);
    case B_SHOUP: return dev_run<F_shoup>(cs, c);
    case B_DIVMOD: return dev_run<F_divmod>(cs, c);
    case B_FIXFRAC: return dev_run<F_fixfrac>(cs, c);
    case B_ADD128: return dev_run<F_add128>(cs, c);
    case B_MAC128: return dev_run<F_mac128>(cs, c);
    }
    abort();
}
bool group_modarith(const std::vector<ModCase> &mods)
{
    bool ok = true;
    for (const ModCase &mc : mods) ok &= chk_modarith(dev_modarith_run, mc);
    return ok;
}

// ---- madasm.h ------------------------------------------------------------------------------------------------------------------
// in: n1 (<= 8), n2 (<= 7), x[15], y[15]: n1 terms, colacc_carry, n2 terms.  out: the columns and colacc_value
AC_DF(F_colacc15)
{
    ColAcc a = {0, 0, 0};
    const u32 n1 = (u32)AC_IN(0), n2 = (u32)AC_IN(1);
    for (u32 t = 0; t < piehip::COLACC_MAX_TERMS; t++)
        if (t < n1) piehip::colacc_mac(a, split30(AC_IN(2 + t)), split30(AC_IN(17 + t)));
    piehip::colacc_carry(a);
    for (u32 t = 0; t < piehip::COLACC_MAX_TOTAL - piehip::COLACC_MAX_TERMS; t++)
        if (t < n2) piehip::colacc_mac(a, split30(AC_IN(10 + t)), split30(AC_IN(25 + t)));
    const piehip::U128 v = piehip::colacc_value(a);
    AC_OUT(0) = a.c0, AC_OUT(1) = a.c1, AC_OUT(2) = a.c2, AC_OUT(3) = v.lo, AC_OUT(4) = v.hi;
} AC_END;
// in: x0[8], x1[8], d[8].  out: the two accumulators of colacc_mac2, then those of two colacc_mac chains
AC_DF(F_colacc_mac2)
{
    ColAcc a = {0, 0, 0}, b = {0, 0, 0}, ra = {0, 0, 0}, rb = {0, 0, 0};
#pragma unroll
    for (u32 t = 0; t < 8; t++) {
        piehip::colacc_mac2(a, b, split30(AC_IN(t)), split30(AC_IN(8 + t)), AC_IN(16 + t));
        piehip::colacc_mac(ra, split30(AC_IN(t)), split30(AC_IN(16 + t)));
        piehip::colacc_mac(rb, split30(AC_IN(8 + t)), split30(AC_IN(16 + t)));
    }
    AC_OUT(0) = a.c0, AC_OUT(1) = a.c1, AC_OUT(2) = a.c2, AC_OUT(3) = b.c0, AC_OUT(4) = b.c1, AC_OUT(5) = b.c2;
    AC_OUT(6) = ra.c0, AC_OUT(7) = ra.c1, AC_OUT(8) = ra.c2, AC_OUT(9) = rb.c0, AC_OUT(10) = rb.c1, AC_OUT(11) = rb.c2;
} AC_END;

static u128 col_value(u64 c0, u64 c1, u64 c2) { return (u128)c0 + (u128)c1 * (1ull << 30) + (u128)c2 * P60; }

bool group_madasm(const std::vector<ModCase> &mods)
{
    bool ok = true;
    const u64 top = P60 - 1;
    for (const ModCase &mc : mods) {
        if (!mc.w60()) continue;  // operands are residues below 2^60; the moduli of the accumulating kernels
        const u64 q = mc.m.q;
        Rng r(0xB001 + q);
        {
            Cases cs(32, 5);
            std::vector<u64> row(32);
            auto add = [&](u32 n1, u32 n2, int kind) {
                row[0] = n1, row[1] = n2;
                for (int k = 2; k < 32; k++) row[k] = kind == 0 ? top : kind == 1 ? q - 1 : kind == 2 ? r.below(q) : kind == 3 ? r.below(P60) : (r.next() & 1 ? top : 0);
                cs.rows.insert(cs.rows.end(), row.begin(), row.end()), cs.n++;
            };
            for (int kind = 0; kind < 2; kind++)
                for (u32 n1 = 0; n1 <= 8; n1++)
                    for (u32 n2 = 0; n2 <= 7; n2++) add(n1, n2, kind);
            for (u32 i = 0; i < NU; i++) add(i % 4 ? 8 : (u32)r.below(9), i % 4 ? 7 : (u32)r.below(8), 2 + (int)(i % 3));
            cs.finish();
            dev_run<F_colacc15>(cs, mod_uni(mc.m));
            Report rp("colacc_mac+carry+value", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                u128 want = 0;
                for (u32 t = 0; t < cs.I(0, i); t++) want += (u128)cs.I(2 + t, i) * cs.I(17 + t, i);
                for (u32 t = 0; t < cs.I(1, i); t++) want += (u128)cs.I(10 + t, i) * cs.I(25 + t, i);
                const u128 got = (((u128)cs.O(4, i)) << 64) | cs.O(3, i);
                rp.expect(got == want && col_value(cs.O(0, i), cs.O(1, i), cs.O(2, i)) == want, "case %u (%llu + %llu terms): value differs from the exact sum",
                          i, ULL(cs.I(0, i)), ULL(cs.I(1, i)));
            }
            ok &= rp.print();
        }
        {
            Cases cs(24, 12);
            std::vector<u64> row(24);
            for (u32 i = 0; i < NU; i++) {
                for (int k = 0; k < 24; k++) row[k] = i == 0 ? top : i == 1 ? q - 1 : i % 3 == 0 ? r.below(P60) : i % 3 == 1 ? r.below(q) : (r.next() & 1 ? top : r.below(P32));
                cs.rows.insert(cs.rows.end(), row.begin(), row.end()), cs.n++;
            }
            cs.finish();
            dev_run<F_colacc_mac2>(cs, mod_uni(mc.m));
            Report rp("colacc_mac2", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                u128 wa = 0, wb = 0;
                bool same = true;
                for (u32 t = 0; t < 8; t++) wa += (u128)cs.I(t, i) * cs.I(16 + t, i), wb += (u128)cs.I(8 + t, i) * cs.I(16 + t, i);
                for (int k = 0; k < 6; k++) same &= cs.O(k, i) == cs.O(6 + k, i);
                rp.expect(same && col_value(cs.O(0, i), cs.O(1, i), cs.O(2, i)) == wa && col_value(cs.O(3, i), cs.O(4, i), cs.O(5, i)) == wb,
                          "case %u: columns %s those of colacc_mac; sums %s", i, same ? "equal" : "DIFFER from",
                          col_value(cs.O(0, i), cs.O(1, i), cs.O(2, i)) == wa && col_value(cs.O(3, i), cs.O(4, i), cs.O(5, i)) == wb ? "exact" : "WRONG");
            }
            ok &= rp.print();
        }
    }
    return ok;
}

// ---- stage_a_common.h ----------------------------------------------------------------------------------------------------------
AC_DF(F_addmod_nb) { AC_OUT(0) = piehip::addmod_nb(AC_IN(0), AC_IN(1), c.u[0]); } AC_END;
// in: c0, c1, c2.  out: colacc_reduce123_lazy, colacc_reduce<false>
AC_DF(F_colacc_reduce123)
{
    const ColAcc a = {AC_IN(0), AC_IN(1), AC_IN(2)};
    const Mod m = uni_mod(c);
    AC_OUT(0) = piehip::colacc_reduce123_lazy(a, m, c.u[U_NQ]);
    AC_OUT(1) = piehip::colacc_reduce<false>(a, m, c.u[U_NQ]);
} AC_END;
AC_DF(F_colacc_reduce124)
{
    const ColAcc a = {AC_IN(0), AC_IN(1), AC_IN(2)};
    AC_OUT(0) = piehip::colacc_reduce<true>(a, uni_mod(c), c.u[U_NQ]);
} AC_END;

bool group_stage_a(const std::vector<ModCase> &mods)
{
    bool ok = true;
    for (const ModCase &mc : mods) {
        const u64 q = mc.m.q;
        if (!mc.plaintext) {  // addmod_nb: q < 2^62, canonical inputs
            Rng r(0xC001 + q);
            Cases cs(2, 1);
            const std::vector<u64> pts = ops_below(q, 12, r, {q / 2, q / 2 + 1, (q - 1) / 2});
            for (u64 a : pts)
                for (u64 b : pts) cs.add({a, b});
            for (u32 i = 0; i < NU; i++) cs.add({r.below(q), r.below(q)});
            for (u32 i = 0; i < NU / 4; i++) {  // sums q - 1, q, q + 1
                const u64 a = r.below(q - 1) + 1;
                cs.add({a, q - 1 - a}), cs.add({a, q - a}), cs.add({a, (q - a + 1) % q});
            }
            cs.finish();
            dev_run<F_addmod_nb>(cs, mod_uni(mc.m));
            Report rp("addmod_nb", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                const u64 want = (u64)(((u128)cs.I(0, i) + cs.I(1, i)) % q);
                rp.expect(cs.O(0, i) == want, "%llu + %llu: got %llu, want %llu", ULL(cs.I(0, i)), ULL(cs.I(1, i)), ULL(cs.O(0, i)), ULL(want));
            }
            ok &= rp.print();
        }
        if (!mc.w60()) continue;
        for (int bits = 123; bits <= 124; bits++) {
            Rng r(0xC002 + q + bits);
            const std::vector<u128> zs = ops_barrett(q, bits, NU, NU, r);
            Cases cs(3, bits == 123 ? 2 : 1);
            for (size_t i = 0; i < zs.size(); i++) {
                u64 c0, c1, c2;
                columns_of(zs[i], i % 2 == 1, r, c0, c1, c2);
                cs.add({c0, c1, c2});
            }
            cs.finish();
            if (bits == 123)
                dev_run<F_colacc_reduce123>(cs, mod_uni_neg(mc.m));
            else
                dev_run<F_colacc_reduce124>(cs, mod_uni_neg(mc.m));
            Report rl("colacc_reduce123_lazy", q), rc(bits == 123 ? "colacc_reduce<false>" : "colacc_reduce<true>", q);
            for (u32 i = 0; i < cs.n; i++) {
                rl.cases++, rc.cases++;
                const u64 want = (u64)(zs[i] % q);
                u128 rem;
                const u128 e = bits == 123 ? model_barrett123_err(zs[i], q) : model_barrett124_err(zs[i], q, &rem);
                rc.model_err(e);
                if (bits == 123) {
                    rl.model_err(e);
                    rl.lazy(cs.O(0, i), want, e, 2, "colacc_reduce123_lazy", (u64)(zs[i] >> 64), (u64)zs[i]);
                }
                const u64 got = cs.O(bits == 123 ? 1 : 0, i);
                rc.expect(got == want, "z = %llu 2^64 + %llu (columns %llu, %llu, %llu): got %llu, want %llu", ULL((u64)(zs[i] >> 64)),
                          ULL((u64)zs[i]), ULL(cs.I(0, i)), ULL(cs.I(1, i)), ULL(cs.I(2, i)), ULL(got), ULL(want));
            }
            rl.need = rl.max_err(), rc.need = rc.max_err();
            if (bits == 123) ok &= rl.print();
            ok &= rc.print();
        }
    }
    return ok;
}

}  // namespace ac
