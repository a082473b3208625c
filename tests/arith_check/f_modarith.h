// f_modarith.h -- one evaluator per function of csrc/modarith.h, compiled for the host (host_check.cpp) and for the device
// (dev_mod.hip).  Word k of case i is at [k n + i]; the modulus and its constants are wave-uniform (c).
#pragma once
#include "check.h"
#include "modarith.h"

namespace ac {

enum {
    B_BARRETT128, B_MULMOD, B_REDUCE123, B_REDUCE124, B_SHOUP_LAZY, B_SHOUP, B_DIVMOD, B_FIXFRAC, B_ADD128, B_MAC128, B_MODARITH_END
};

#define AC_IN(k) in[(size_t)(k) * n + i]
#define AC_OUT(k) out[(size_t)(k) * n + i]
#define AC_F(name) \
    struct name {  \
        static PH_HD void go(const u64 *in, u64 *out, u32 n, u32 i, const Uni &c)
#define AC_END }

AC_F(F_barrett128) { AC_OUT(0) = piehip::barrett128(AC_IN(0), AC_IN(1), uni_mod(c)); } AC_END;
AC_F(F_mulmod) { AC_OUT(0) = piehip::mulmod(AC_IN(0), AC_IN(1), uni_mod(c)); } AC_END;
AC_F(F_reduce123) { AC_OUT(0) = piehip::reduce123(piehip::U128{AC_IN(1), AC_IN(0)}, uni_mod(c)); } AC_END;
AC_F(F_reduce124) { AC_OUT(0) = piehip::reduce124(piehip::U128{AC_IN(1), AC_IN(0)}, uni_mod(c)); } AC_END;
AC_F(F_shoup_lazy) { AC_OUT(0) = piehip::mul_shoup_lazy(AC_IN(0), AC_IN(1), AC_IN(2), c.u[0]); } AC_END;
AC_F(F_shoup) { AC_OUT(0) = piehip::mul_shoup(AC_IN(0), AC_IN(1), AC_IN(2), c.u[0]); } AC_END;
AC_F(F_divmod)
{
    u64 qt, rm;
    piehip::divmod_shoup(AC_IN(0), AC_IN(1), AC_IN(2), c.u[0], qt, rm);
    AC_OUT(0) = qt, AC_OUT(1) = rm;
} AC_END;
AC_F(F_fixfrac) { AC_OUT(0) = piehip::fixfrac(AC_IN(0), uni_mod(c)); } AC_END;
AC_F(F_add128)
{
    piehip::U128 a = {AC_IN(0), AC_IN(1)};
    piehip::add128(a, piehip::U128{AC_IN(2), AC_IN(3)});
    AC_OUT(0) = a.lo, AC_OUT(1) = a.hi;
} AC_END;
AC_F(F_mac128)
{
    piehip::U128 a = {AC_IN(0), AC_IN(1)};
    piehip::mac128(a, AC_IN(2), AC_IN(3));
    AC_OUT(0) = a.lo, AC_OUT(1) = a.hi;
} AC_END;

}  // namespace ac
