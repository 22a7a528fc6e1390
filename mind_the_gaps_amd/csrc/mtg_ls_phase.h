// mtg_ls_phase.h -- the (cos, sin) pair of one (frequency, sample) of the Lomb-Scargle kernels, with the phase formed in
// cycles: shared by mtg_lomb_scargle.hip (one sinusoid) and mtg_lomb_scargle_multi.hip (its harmonics follow from the
// pair by angle addition), so that both see the same pair bit for bit.
#ifndef MTG_LS_PHASE_H
#define MTG_LS_PHASE_H

#include "mtg_device.h"
#include "mtg_math.h"

#ifndef MTG_LS_CHUNK
#define MTG_LS_CHUNK 256
#endif
#define MTG_LS_THREADS 256

struct MtgLsTab {
    double2 cis[MTG_TRIG_N];   // (cos, sin)(2 pi j / N): the table of mtg_math.h
};

// (sin, cos) of 2 pi f te with the phase formed in cycles.  The product is taken exactly, f te = p + pe (one fma); the
// integer part of p is dropped before anything is rounded (p - rint(p) is exact), the fraction q in [-1/2, 1/2] is
// split into m = rint(q N) table steps and a remainder (exact again: both are multiples of ulp(p) below 2^-1), the low
// part of the product joins the remainder, and only then comes the factor 2 pi -- on |x| <= pi / N, where its rounding
// is 1e-19 rad.  What is left is the rounding of te itself.  The table index is masked as in mtg_abs_sincos
// (mtg_sweep_mean.h): whatever f te is, the load stays inside the table.
template <class Tab>
__device__ __forceinline__ void mtg_cycles_sincos(double f, double te, double *sn, double *cs, const Tab *tab)
{
#pragma clang fp contract(off)
    const double magic = 0x1.8p+56;                                                 // 1.5 * 2^(52+4)
    const double p = f * te;
    const double pe = __builtin_fma(f, te, -p);
    const double q = p - __builtin_rint(p);
    const double wk = __builtin_fma(q, 16.0 * MTG_TRIG_N, magic);                   // q 16 N
    const double md16 = wk - magic;                                                 // 16 m
    const double rc = __builtin_fma(md16, -(1.0 / (16.0 * MTG_TRIG_N)), q) + pe;    // cycles, |rc| <= 1 / 2N
    const double r = rc * 0x1.921fb54442d18p+2;                                     // 2 pi
    const int m16 = __double2loint(wk) << 4;                                        // low mantissa dword of wk = m
    const double2 cj = *(const double2 *)((const char *)tab->cis + (m16 & ((MTG_TRIG_N - 1) * 16)));
    double s, c;
    mtg_sincos_small(r, &s, &c);
    *sn = __builtin_fma(cj.x, s, cj.y * c);
    *cs = __builtin_fma(-cj.y, s, cj.x * c);
}

// the table, filled by the whole workgroup (the caller's next barrier publishes it)
__device__ __forceinline__ void mtg_ls_fill_tab(MtgLsTab *tab)
{
    for (int j = threadIdx.x; j < MTG_TRIG_N; j += blockDim.x) {
        double s, c;
        sincospi((double)j * (2.0 / MTG_TRIG_N), &s, &c);
        tab->cis[j] = make_double2(c, s);
    }
}

#endif
