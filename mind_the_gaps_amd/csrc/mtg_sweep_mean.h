// mtg_sweep_mean.h -- the profile means as `Mean` types of mtg_sweep (mtg_sweep.h): per-lane constants from the
// row's coefficient column (mtg_mean.h says what they are) and the value at a sample's ABSOLUTE time, built from the
// pieces of mtg_math.h -- the (cos, sin) and exp2 tables in LDS and their short polynomials -- so that a step stays one
// basic block and no OCML sin / exp (30-65 instructions and two dozen 64-bit constants each) enters the loop.
#ifndef MTG_SWEEP_MEAN_H
#define MTG_SWEEP_MEAN_H

#include "mtg_mean.h"
#include "mtg_sweep.h"

static_assert(MTG_EXP_BITS >= 11 && MTG_TRIG_BITS >= 11, "the profile means use the short polynomials of the 2^11-entry tables");

// (sin, cos) of w t at the absolute time t.  The product is taken exactly, w t = p + pe (one fma), and p reduced by
// k = rint(p N / 2 pi) table steps with 2 pi / N in two parts: k C1 - p is exact in the first fma (C1 has 53 bits, the
// difference is below 2^-9 and a multiple of ulp(C1) for every k < 2^47), the second brings in C2 = 2 pi / N - C1, then
// the low part of the product.  The reduced phase is good to ~1e-16 rad for phases below ~1e9 rad, against the
// ulp(w t) / 2 -- 7e-12 rad at 1e5 rad -- of the phase formed plainly, which is what numpy's evaluation of the
// reference's formula carries.  The table index is masked: whatever w t is (NaN, inf), the load stays inside the table.
template <class Tab>
__device__ __forceinline__ void mtg_abs_sincos(double w, double t, double *sn, double *cs, const Tab *tab)
{
#pragma clang fp contract(off)
    const double magic = 0x1.8p+56;                                                 // 1.5 * 2^(52+4)
    const double p = w * t;
    const double pe = __builtin_fma(w, t, -p);
    const double wk = __builtin_fma(p, 0x1.45f306dc9c883p+1 * MTG_TRIG_N, magic);   // p 16 N / 2 pi
    const double md16 = wk - magic;                                                 // 16 k
    const double r1 = __builtin_fma(md16, -(0x1.921fb54442d18p-2 / MTG_TRIG_N), p);            // C1 / 16
    const double r = __builtin_fma(md16, -(0x1.1a62633145c07p-56 / MTG_TRIG_N), r1) + pe;      // C2 / 16
    const int m16 = __double2loint(wk) << 4;                                        // low mantissa dword of wk = k
    const double2 cj = *(const double2 *)((const char *)tab->cis + (m16 & ((MTG_TRIG_N - 1) * 16)));
    double s, c;
    mtg_sincos_small(r, &s, &c);
    *sn = __builtin_fma(cj.x, s, cj.y * c);
    *cs = __builtin_fma(-cj.y, s, cj.x * c);
}

// exp(d^2 q) for q = qh + ql <= 0 in units of ln2 / (8 N_exp) (mtg_mean_derive): mtg_exp_cdx's reduction and polynomial
// with the square taken exactly, d^2 = d2 + e2, and the low parts of both factors in the remainder -- the exponent's only
// error is the rounding of d itself.  Far below the underflow point the result is 0 (the remainder of a product beyond
// 2^56 table steps means nothing); the table index is masked.
template <class Tab>
__device__ __forceinline__ double mtg_exp_sq(double d, double qh, double ql, const Tab *tab)
{
#pragma clang fp contract(off)
    const double magic = 0x1.8p+55;                                                 // 1.5 * 2^(52+3)
    const double d2 = d * d;
    const double e2 = __builtin_fma(d, d, -d2);
    const double w = __builtin_fma(d2, qh, magic);
    const double q8 = w - magic;                                                    // 8 rint(y N / ln2)
    const int i8 = (int)q8;                                                         // saturates
    const double t = *(const double *)((const char *)tab->exp2_frac + (i8 & ((MTG_EXP_N - 1) * 8)));
    const double f = __builtin_fma(d2, qh, -q8) + __builtin_fma(e2, qh, d2 * ql);
    double p = __builtin_fma(f, MTG_EXP_C1 * MTG_EXP_C1 * MTG_EXP_C1 / 6.0, MTG_EXP_C1 * MTG_EXP_C1 / 2.0);
    p = __builtin_fma(p, f, MTG_EXP_C1) * f;
    const double v = __builtin_ldexp(__builtin_fma(t, p, t), i8 >> (3 + MTG_EXP_BITS));
    return d2 * qh < -0x1.2p+24 ? 0.0 : v;                                          // exp(-798) = 0 in double
}

template <int KIND> struct MtgMeanProfile;

// constant + amplitude sin(frequency t + phase)
template <> struct MtgMeanProfile<MTG_MEAN_SINE> {
    static constexpr bool always = true, trig = true;
    static constexpr int nconst = 4;
    double c0, w, ac, as;
    __device__ __forceinline__ void load(const MtgSolveArgs &a, const double *cf, int64_t cs)
    {
        c0 = cf[a.lay.mean(1) * cs];
        w = cf[a.lay.mean_extra(0) * cs]; ac = cf[a.lay.mean_extra(1) * cs]; as = cf[a.lay.mean_extra(2) * cs];
    }
    template <class Tab>
    __device__ __forceinline__ double value(double tc, const Tab *tab) const
    {
        double s, c;
        mtg_abs_sincos(w, tc, &s, &c, tab);
        return fma(ac, s, fma(as, c, c0));
    }
};

// constant + amplitude0 sin(frequency t + phase0) + amplitude1 sin(2 frequency t + phase1)
template <> struct MtgMeanProfile<MTG_MEAN_TWOSINE> {
    static constexpr bool always = true, trig = true;
    static constexpr int nconst = 6;
    double c0, w, a0c, a0s, a1c, a1s;
    __device__ __forceinline__ void load(const MtgSolveArgs &a, const double *cf, int64_t cs)
    {
        c0 = cf[a.lay.mean(1) * cs];
        w = cf[a.lay.mean_extra(0) * cs];
        a0c = cf[a.lay.mean_extra(1) * cs]; a0s = cf[a.lay.mean_extra(2) * cs];
        a1c = cf[a.lay.mean_extra(3) * cs]; a1s = cf[a.lay.mean_extra(4) * cs];
    }
    template <class Tab>
    __device__ __forceinline__ double value(double tc, const Tab *tab) const
    {
#pragma clang fp contract(off)
        double s, c;
        mtg_abs_sincos(w, tc, &s, &c, tab);
        const double s2 = (s + s) * c, c2 = (c - s) * (c + s);
        return fma(a0c, s, fma(a0s, c, fma(a1c, s2, fma(a1s, c2, c0))));
    }
};

// amplitude / (2 pi sigma) exp(-(t - mean)^2 / (2 sigma^2)) + constant
template <> struct MtgMeanProfile<MTG_MEAN_GAUSSIAN> {
    static constexpr bool always = true, trig = false;
    static constexpr int nconst = 5;
    double c0, mu, norm, qh, ql;
    __device__ __forceinline__ void load(const MtgSolveArgs &a, const double *cf, int64_t cs)
    {
        c0 = cf[a.lay.mean(1) * cs];
        mu = cf[a.lay.mean_extra(0) * cs]; norm = cf[a.lay.mean_extra(1) * cs];
        qh = cf[a.lay.mean_extra(2) * cs]; ql = cf[a.lay.mean_extra(3) * cs];
    }
    template <class Tab>
    __device__ __forceinline__ double value(double tc, const Tab *tab) const
    {
        return fma(norm, mtg_exp_sq(tc - mu, qh, ql, tab), c0);
    }
};

#endif  // MTG_SWEEP_MEAN_H
