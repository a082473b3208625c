// dev_ntt16.hip -- the 16-coefficient transform's instruction blocks (csrc/ntt16_kernel.h, ntt16_bfly.inc): the eight forms of
// bfly<INV, SC, H2>, csub_neg, csub2_neg, colacc123_to_4q.
#include "chk_bfly.h"
#include "ntt16_kernel.h"

namespace ac {

namespace n16 = piehip::ntt16;

static __device__ __forceinline__ n16::ModC modc(const Uni &c)
{
    n16::ModC m;
    m.nql = (u32)c.u[U_NQ], m.nqh = (u32)(c.u[U_NQ] >> 32), m.nq4 = 0 - 4 * c.u[0], m.q4 = 4 * c.u[0];
    return m;
}
// in: a, b, w, floor(w 2^63 / q).  SC: the twiddle is wave-uniform, u[U_X] = w, u[U_HAT] = floor(w 2^63 / q)
template <bool INV, bool SC, bool H2>
struct F_bfly {
    static __device__ __forceinline__ void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)
    {
        u64 x = AC_IN(0), y = AC_IN(1);
        n16::u64x2 p;
        p.x = SC ? c.u[U_X] : AC_IN(2), p.y = SC ? c.u[U_HAT] : AC_IN(3);
        n16::bfly<INV, SC, H2>(x, y, n16::make_tw(p), modc(c));
        AC_OUT(0) = x, AC_OUT(1) = y;
    }
};
// in: x.  uniform: u[U_X] = 2^64 - m (csub_neg); 2^64 - 4q, 2^64 - 2q (csub2_neg)
AC_DF(F_csub_neg)
{
    AC_OUT(0) = n16::csub_neg(AC_IN(0), c.u[U_X]);
    AC_OUT(1) = n16::csub2_neg(AC_IN(0), 0 - 4 * c.u[0], c.u[U_N2Q]);
} AC_END;
AC_DF(F_colacc123_to_4q)
{
    const u64 mu = (c.u[2] << 59) | (c.u[1] >> 5);  // floor(2^123 / q) from r1:r0, as the kernel forms it
    AC_OUT(0) = n16::colacc123_to_4q(AC_IN(0), AC_IN(1), AC_IN(2), mu, c.u[U_NQ]);
} AC_END;

// the cases of one direction, shared by its four forms
struct Bfly16Cases {
    std::vector<u64> ws;
    Cases cs;
    Bfly16Cases(const ModCase &mc, bool inv) : cs(4, 2)
    {
        Rng r(0xF001 + mc.m.q + inv);
        size_t nd;
        ws = uniform_ws(mc, r, 8, &nd);
        bfly_cases(mc, inv, r, ws, nd, cs);
    }
};
template <bool INV, bool SC, bool H2>
static bool chk_bfly16(const ModCase &mc, Bfly16Cases &bc)
{
    const u64 q = mc.m.q;
    Cases &cs = bc.cs;
    Report rp((std::string("bfly<") + (INV ? "inv," : "fwd,") + (SC ? "sc," : "vec,") + (H2 ? "h2>" : "h1>")).c_str(), q);
    DevCases d(cs);
    Uni c = mod_uni_neg(mc.m);
    if (!SC) {
        d.run<F_bfly<INV, SC, H2>>(c);
        for (u32 i = 0; i < cs.n; i++) bfly_check(rp, INV, q, cs.I(0, i), cs.I(1, i), cs.I(2, i), cs.O(0, i), cs.O(1, i));
    } else
        for (u64 w : bc.ws) {
            c.u[U_X] = w, c.u[U_HAT] = (u64)(((u128)w * P63) / q);
            d.run<F_bfly<INV, SC, H2>>(c);
            for (u32 i = 0; i < cs.n; i++) bfly_check(rp, INV, q, cs.I(0, i), cs.I(1, i), w, cs.O(0, i), cs.O(1, i));
        }
    rp.need = mc.w60() ? 3 : rp.max_err();
    return rp.print();
}

bool group_ntt16(const std::vector<ModCase> &mods)
{
    bool ok = true;
    for (const ModCase &mc : mods) {
        if (mc.plaintext || !mc.lt60()) continue;
        const u64 q = mc.m.q;
        {
            Bfly16Cases fwd(mc, false);
            ok &= chk_bfly16<false, false, false>(mc, fwd);
            ok &= chk_bfly16<false, false, true>(mc, fwd);
            ok &= chk_bfly16<false, true, false>(mc, fwd);
            ok &= chk_bfly16<false, true, true>(mc, fwd);
        }
        {
            Bfly16Cases inv(mc, true);
            ok &= chk_bfly16<true, false, false>(mc, inv);
            ok &= chk_bfly16<true, false, true>(mc, inv);
            ok &= chk_bfly16<true, true, false>(mc, inv);
            ok &= chk_bfly16<true, true, true>(mc, inv);
        }
        {  // csub_neg: x in [0, 2m) for m = q, 2q, 4q;  csub2_neg: x in [0, 8q) -> [0, 2q).  Every multiple of q and its neighbours
            Report r1("csub_neg", q), r2("csub2_neg", q);
            for (u64 m = q; m <= 4 * q; m *= 2) {
                Rng r(0xF002 + m);
                Cases cs(1, 2);
                for (u64 k = 0; k <= 8; k++)
                    for (u64 x : {k * q - 1, k * q, k * q + 1})
                        if (x < 8 * q) cs.add({x});
                for (u32 i = 0; i < NU / 2; i++) cs.add({r.below(8 * q)});
                cs.finish();
                Uni c = mod_uni_neg(mc.m);
                c.u[U_X] = 0 - m;
                dev_run<F_csub_neg>(cs, c);
                for (u32 i = 0; i < cs.n; i++) {
                    const u64 x = cs.I(0, i);
                    if (x < 2 * m) {
                        r1.cases++;
                        r1.expect(cs.O(0, i) == (x < m ? x : x - m), "x = %llu, m = %llu: got %llu", ULL(x), ULL(m), ULL(cs.O(0, i)));
                    }
                    if (m == q) {
                        r2.cases++;
                        r2.expect(cs.O(1, i) == x % (2 * q), "x = %llu: got %llu, want %llu", ULL(x), ULL(cs.O(1, i)), ULL(x % (2 * q)));
                    }
                }
            }
            ok &= r1.print();
            ok &= r2.print();
        }
        if (mc.w60()) {  // colacc123_to_4q: a column accumulator below 2^123 to [0, 4q)
            Rng r(0xF003 + q);
            const std::vector<u128> zs = ops_barrett(q, 123, NU, NU, r);
            Cases cs(3, 1);
            for (size_t i = 0; i < zs.size(); i++) {
                u64 c0, c1, c2;
                columns_of(zs[i], i % 2 == 1, r, c0, c1, c2);
                cs.add({c0, c1, c2});
            }
            cs.finish();
            dev_run<F_colacc123_to_4q>(cs, mod_uni_neg(mc.m));
            Report rp("colacc123_to_4q", q);
            for (u32 i = 0; i < cs.n; i++) {
                rp.cases++;
                const u128 e = model_barrett123_err(zs[i], q);
                rp.model_err(e);
                rp.lazy(cs.O(0, i), (u64)(zs[i] % q), e, 2, "colacc123_to_4q", (u64)(zs[i] >> 64), (u64)zs[i]);
            }
            rp.need = rp.max_err();
            ok &= rp.print();
        }
    }
    return ok;
}

}  // namespace ac
