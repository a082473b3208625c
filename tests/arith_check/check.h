// check.h -- host side of the arithmetic-block harness: exact references in unsigned __int128 (+ - * / % only), the host models
// of the quotient estimates as the comments of csrc/ state them, operand sets with fixed seeds and the report lines.
// modarith.h is included for the types Mod / U128 alone: nothing here calls its functions.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "params.hpp"

namespace ac {

using piehip::Mod;
using piehip::u32;
using piehip::u64;
typedef unsigned __int128 u128;

static const u128 ONE = 1;
static const u64 P31 = 1ull << 31, P32 = 1ull << 32, P59 = 1ull << 59, P60 = 1ull << 60, P63 = 1ull << 63;
static const u64 M32 = 0xffffffffull;

// wave-uniform operands of a block: kernel arguments on the device (scalar registers, as in the product)
struct Uni {
    u64 u[16];
};
PH_HD Mod uni_mod(const Uni &c)  // u[0..4] = q, r0, r1, fconst, fshift
{
    Mod m;
    m.q = c.u[0], m.r0 = c.u[1], m.r1 = c.u[2], m.n_inv = 0, m.n_inv_sh = 0, m.fconst = c.u[3], m.fshift = (u32)c.u[4], m.pad = 0;
    return m;
}
static inline Uni mod_uni(const Mod &m)
{
    Uni c;
    memset(&c, 0, sizeof c);
    c.u[0] = m.q, c.u[1] = m.r0, c.u[2] = m.r1, c.u[3] = m.fconst, c.u[4] = m.fshift;
    return c;
}

// one modulus under test: Mod and twiddles as HostParams::init computed them
struct ModCase {
    Mod m;
    std::vector<u64> tw, tw_sh;  // a few real twiddles {w, floor(w 2^64 / q)} (empty for the plaintext modulus)
    bool plaintext;
    bool w60() const { return m.q > P59 && m.q < P60; }  // the width of the one-word Barrett and the column accumulators
    bool lt60() const { return m.q < P60; }              // the width of the 63-bit Shoup blocks
};

struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed) {}
    u64 next()
    {
        u64 z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    u64 below(u64 lim) { return (u64)(((u128)next() * lim) >> 64); }            // lim >= 1
    u128 below128(u128 lim) { return ((((u128)next()) << 64) | next()) % lim; }  // lim >= 1
};

// block -> cases: `nin` input words and `nout` output words per case, word k of case i at [k n + i]
struct Cases {
    u32 n = 0;
    int nin = 0, nout = 0;
    std::vector<u64> in, out;
    Cases(int nin_, int nout_) : nin(nin_), nout(nout_) {}
    void add(std::initializer_list<u64> v)
    {
        if ((int)v.size() != nin) abort();
        rows.insert(rows.end(), v);
        n++;
    }
    void finish()  // rows -> columns
    {
        in.assign((size_t)nin * n, 0);
        out.assign((size_t)nout * n, 0);
        for (u32 i = 0; i < n; i++)
            for (int k = 0; k < nin; k++) in[(size_t)k * n + i] = rows[(size_t)i * nin + k];
    }
    u64 I(int k, u32 i) const { return in[(size_t)k * n + i]; }
    u64 O(int k, u32 i) const { return out[(size_t)k * n + i]; }
    std::vector<u64> rows;
};
// evaluates block `id` on every case (a loop on the host, one launch on the device)
typedef void (*RunFn)(int id, Cases &cs, const Uni &c);

struct Report {
    std::string block;
    u64 q;
    u64 cases = 0, fails = 0;
    int need = -1;        // estimate errors 0..need must each have MIN_COVER cases; -1: no coverage condition
    long err[8] = {0};    // histogram of the host model's estimate error
    bool has_k = false;   // lazy form: the multiple of q in the output, from the block (kdev) and from the model (kmod)
    long kdev[8] = {0}, kmod[8] = {0};
    u64 kdiff = 0;        // cases whose multiple differs from the model's
    Report(const char *b, u64 q_) : block(b), q(q_) {}
    void vfail(const char *fmt, va_list ap)
    {
        if (fails++ >= 5) return;
        char buf[512];
        vsnprintf(buf, sizeof buf, fmt, ap);
        first.push_back(buf);
    }
    void fail(const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vfail(fmt, ap);
        va_end(ap);
    }
    void expect(bool ok, const char *fmt, ...)
    {
        if (ok) return;
        va_list ap;
        va_start(ap, fmt);
        vfail(fmt, ap);
        va_end(ap);
    }
    void model_err(u128 e) { err[e < 7 ? (int)e : 7]++; }
    int max_err() const
    {
        int m = 0;
        for (int e = 0; e < 8; e++)
            if (err[e]) m = e;
        return m;
    }
    // lazy output `got` against the canonical value `want` and the model's multiple `km`; `kmax`: the contract's largest multiple
    void lazy(u64 got, u64 want, u128 km, u32 kmax, const char *what, u64 a, u64 b)
    {
        has_k = true;
        const u64 d = got - want;
        const u64 k = d / q;
        if (got < want || d % q != 0 || k > kmax) {
            fail("%s(%llu, %llu): got %llu, want %llu + k q with k <= %u", what, (unsigned long long)a, (unsigned long long)b,
                 (unsigned long long)got, (unsigned long long)want, kmax);
            return;
        }
        kdev[k < 7 ? k : 7]++;
        kmod[km < 7 ? (int)km : 7]++;
        if (k != (u64)km) {
            kdiff++;
            fail("%s(%llu, %llu): multiple of q is %llu, the estimate of the comment gives %llu", what, (unsigned long long)a,
                 (unsigned long long)b, (unsigned long long)k, (unsigned long long)(u64)km);
        }
    }
    static const long MIN_COVER = 64;
    bool covered() const
    {
        for (int e = 0; e <= need; e++)
            if (err[e] < MIN_COVER) return false;
        return true;
    }
    // prints the line; returns whether the block held its contract and the operand set met its coverage condition
    bool print() const
    {
        printf("arith %s q=%llu cases=%llu fail=%llu", block.c_str(), (unsigned long long)q, (unsigned long long)cases,
               (unsigned long long)fails);
        long any = 0;
        for (int e = 0; e < 8; e++) any += err[e];
        if (any) printf(" err=[%ld,%ld,%ld,%ld,%ld]", err[0], err[1], err[2], err[3], err[4] + err[5] + err[6] + err[7]);
        if (need >= 0) printf(" need=%d cover=%s", need, covered() ? "ok" : "LOW");
        if (has_k) {
            printf(" kdev=[%ld,%ld,%ld,%ld,%ld,%ld,%ld]", kdev[0], kdev[1], kdev[2], kdev[3], kdev[4], kdev[5], kdev[6] + kdev[7]);
            printf(" kmod=[%ld,%ld,%ld,%ld,%ld,%ld,%ld]", kmod[0], kmod[1], kmod[2], kmod[3], kmod[4], kmod[5], kmod[6] + kmod[7]);
            printf(" kdiff=%llu", (unsigned long long)kdiff);
        }
        printf("\n");
        for (const std::string &s : first) printf("  FAIL %s q=%llu: %s\n", block.c_str(), (unsigned long long)q, s.c_str());
        fflush(stdout);
        return fails == 0 && (need < 0 || covered());
    }
    std::vector<std::string> first;
};

// ---- exact references ------------------------------------------------------------------------------------------------------
static inline u64 ref_mulmod(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static inline u64 ref_shoup64(u64 w, u64 q) { return (u64)(((u128)w * (ONE << 64)) / q); }  // the operand floor(w 2^64 / q)

// ---- host models of the quotient estimates, as the comments state them -------------------------------------------------------
// "qe = 2 bh sh + (bh sl + bl sh) >> 31" with ws = floor(w 2^63 / q): how far below floor(b w / q) it lies
static inline u128 model_shoup63_err(u64 b, u64 w, u64 q)
{
    const u64 ws = (u64)(((u128)w * P63) / q);
    const u64 bl = b % P32, bh = b / P32, sl = ws % P32, sh = ws / P32;
    const u128 qe = 2 * (u128)bh * sh + ((u128)bh * sl + (u128)bl * sh) / P31;
    return (u128)b * w / q - qe;
}
// barrett128: qhat = floor(z R / 2^128) with R = r1:r0 = floor(2^128 / q), which the code forms exactly from the four 64-bit
// partial products: how far below floor(z / q) it lies
static inline u128 model_barrett128_err(u128 z, u64 q)
{
    const u128 W = ONE << 64, R = (~(u128)0) / q;  // q is odd and > 1: floor((2^128 - 1) / q) = floor(2^128 / q)
    const u128 z1 = z / W, z0 = z % W, r1 = R / W, r0 = R % W;
    const u128 m10 = z1 * r0, m01 = z0 * r1;
    const u128 carry = (m10 % W + m01 % W + (z0 * r0) / W) / W;
    const u128 qhat = z1 * r1 + m10 / W + m01 / W + carry;
    return z / q - qhat;
}
// "floor(floor(z / 2^59) mu / 2^64)" with mu = floor(2^123 / q): how far below floor(z / q) it lies
static inline u128 model_barrett123_err(u128 z, u64 q)
{
    const u128 mu = (ONE << 123) / q;
    const u128 qhat = ((z / P59) * mu) / (ONE << 64);  // z < 2^123, mu < 2^64: the product fits
    return z / q - qhat;
}
// "t = floor(floor(z / 2^60) mu / 2^64)": how far below floor(z / 2q) it lies; the remainder z - 2 t q
static inline u128 model_barrett124_err(u128 z, u64 q, u128 *rem)
{
    const u128 mu = (ONE << 123) / q;
    const u128 t = ((z / P60) * mu) / (ONE << 64);
    *rem = z - 2 * t * q;
    return z / (2 * (u128)q) - t;
}
// 64-bit Shoup: floor(a wsh / 2^64) with wsh = floor(w 2^64 / q): how far below floor(a w / q)
static inline u128 model_shoup64_err(u64 a, u64 w, u64 q)
{
    const u128 qe = ((u128)a * ref_shoup64(w, q)) / (ONE << 64);
    return (u128)a * w / q - qe;
}

// ---- operand sets ------------------------------------------------------------------------------------------------------------
// uniform below `lim` with the corners 0, 1, lim - 1, lim - 2 and the given extra points (those below lim) in front
static inline std::vector<u64> ops_below(u64 lim, u32 n, Rng &r, std::initializer_list<u64> extra = {})
{
    std::vector<u64> v = {0, 1, lim - 1, lim - 2};
    for (u64 e : extra)
        if (e < lim) v.push_back(e);
    while (v.size() < n) v.push_back(r.below(lim));
    return v;
}
// the directed family: a below `lim` and w < q with the low 32-bit words of a and of floor(w 2^63 / q) within 2^8 of 2^32 - 1.
// Appends the accepted (a, w) pairs of `draws` draws.
static inline bool directed_w(u64 q, Rng &r, u64 &w)
{
    const u64 ws_t = (r.below(P31) * P32) + (M32 - r.below(256));
    const u64 wc = (u64)(((u128)ws_t * q + P63 - 1) / P63);  // the smallest w whose constant is >= the target
    if (wc >= q) return false;
    const u64 ws = (u64)(((u128)wc * P63) / q);
    if (M32 - ws % P32 >= 256) return false;
    w = wc;
    return true;
}
static inline bool directed_a(u64 lim, Rng &r, u64 &a)
{
    a = r.below((lim - 1) / P32 + 1) * P32 + (M32 - r.below(256));
    return a < lim;
}
static inline void ops_directed(u64 q, u64 lim, u32 draws, Rng &r, std::vector<u64> &a, std::vector<u64> &w)
{
    for (u32 i = 0; i < draws; i++) {
        u64 av, wc;
        if (directed_w(q, r, wc) && directed_a(lim, r, av)) a.push_back(av), w.push_back(wc);
    }
}
// ... and below `lim` << 2^63, where the 63-bit estimate is 3 short only if besides the two low words the dropped fraction
// frac((bh sl + bl sh) / 2^31) is within about lim / 2^63 of 1: for the constant w, low words bl as above and the high word bh
// SOLVED from bh sl + bl sh = 2^31 - 1 - delta (mod 2^31), kept when b = bh 2^32 + bl is below lim (one try in 2^63 / lim).
// Appends up to `want` such b; nothing where lim < 2^43 (expected yield below one per 2^20 tries) or the low word of the constant is even.
static inline void ops_solved63(u64 q, u64 lim, u64 w, u32 want, Rng &r, std::vector<u64> &b)
{
    const u64 ws = (u64)(((u128)w * P63) / q), sl = ws % P32, sh = ws / P32;
    if (sl % 2 == 0 || lim < (1ull << 43)) return;
    u64 inv = sl;  // sl^-1 mod 2^31 (Newton; sl sl = 1 mod 8)
    for (int k = 0; k < 5; k++) inv = (inv * (2 - sl * inv)) % P31;
    const u64 nhi = (lim - 1) / P32 + 1, dmax = lim / P32 / 2 + 4;
    const u64 tries = ((u128)want * 4 * P31) / nhi < (1ull << 24) ? (u64)(((u128)want * 4 * P31) / nhi) : (1ull << 24);
    for (u64 t = 0, got = 0; t < tries && got < want; t++) {
        const u64 bl = M32 - r.below(256), target = P31 - 1 - r.below(dmax < P31 ? dmax : P31);
        const u64 bh = (((target + P31 - (bl * sh) % P31) % P31) * inv) % P31;
        if (bh >= nhi || bh * P32 + bl >= lim) continue;
        b.push_back(bh * P32 + bl), got++;
    }
}
// the 64-bit Shoup estimate floor(a wsh / 2^64) of a canonical a is 1 short iff a w mod q < a frac(w 2^64 / q) q / 2^64 (< q^2 /
// 2^64): pairs with a just below q and a w = s (mod q) for s from 1 to about q^2 / 2^64.  (For q < 2^32 no pair qualifies.)
static inline void ops_directed64(u64 q, u32 draws, Rng &r, std::vector<u64> &a, std::vector<u64> &w)
{
    const u64 smax = (u64)(((u128)q * q) / (ONE << 64));
    for (u32 i = 0; i < draws; i++) {
        const u64 av = q - 1 - r.below(q / 8192 + 1);
        const u64 s = 1 + r.below(smax ? smax : 1);
        a.push_back(av), w.push_back(ref_mulmod(s % q, piehip::invmod(av, q), q));
    }
}
// Barrett operands below 2^bits (bits = 123 or 124): uniform, uniform sums of a few products, the range ends, multiples of q and
// one below near the top, the low `bits - 64` bits all ones; and the directed family: low bits all ones AND z mod q (mod 2q for 124)
// small, at every high word that allows it -- the operands at which both rounding losses of the estimate are largest.
static inline std::vector<u128> ops_barrett(u64 q, int bits, u32 n_uniform, u32 n_directed, Rng &r, u64 s0 = 0)
{
    const u128 lim = ONE << bits;
    const u64 lowones = (1ull << (bits - 64)) - 1;  // 59 or 60 low bits
    const u128 lowp = (u128)lowones + 1;
    std::vector<u128> v = {0, 1, q - 1, q, lim - 1, lim - 2, lim - 1 - (lim - 1) % q, lim - 2 - (lim - 1) % q};
    for (u32 i = 0; i < n_uniform / 4; i++) v.push_back(r.below128(lim));
    for (u32 i = 0; i < n_uniform / 4; i++) {  // sums of 1 .. 7 (15) products of canonical residues
        u128 z = 0;
        const u32 terms = 1 + (u32)r.below(bits == 123 ? 7 : 15);
        for (u32 t = 0; t < terms; t++) z += (u128)r.below(q) * r.below(q);
        v.push_back(z);
    }
    for (u32 i = 0; i < n_uniform / 4; i++) {  // multiples of q in the top half of the range, and one below
        const u128 k = (lim / 2) / q + r.below128((lim / 2) / q);
        v.push_back(k * q), v.push_back(k * q - 1);
    }
    for (u32 i = 0; i < n_uniform / 4; i++) v.push_back((r.below128(lim) / lowp) * lowp + lowones);
    // directed: zh 2^k + (2^k - 1) = s (mod q)  <=>  zh = (s + 1) 2^-k - 1 (mod q)
    const u64 inv = piehip::invmod((u64)(lowp % q), q);
    u32 made = 0;
    for (u64 s = s0 + (bits == 124 ? 1 - s0 % 2 : 0); made < n_directed; s += (bits == 124 ? 2 : 1)) {
        const u64 zh0 = (u64)(((u128)ref_mulmod((s + 1) % q, inv, q) + q - 1) % q);
        for (u128 zh = zh0; zh < (ONE << 64) && made < n_directed; zh += q) {
            const u128 z = zh * lowp + lowones;
            if (bits == 124 && z % (2 * (u128)q) != s) continue;  // z = s + q (mod 2q): not the small remainder
            v.push_back(z), made++;
        }
    }
    return v;
}

}  // namespace ac
