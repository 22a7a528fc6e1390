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

// The phase bin floor(nbins frac(f te)) of the epoch-folding kernels (mtg_epoch_fold.hip), nbins in 2 .. 32, with the
// product taken exactly as above: f te = p + pe, q = p - rint(p) in [-1/2, 1/2] (exact), so that frac(f te) = q + pe
// mod 1.  nbins q = hi + lo is an exact pair again.  The integer part is split off as above, by the NEAREST integer:
// n = rint(hi) and g = hi - n in [-1/2, 1/2] are exact whatever the sign and size of hi (hi - floor(hi) is not: just below
// an integer, or just below zero, it rounds up to 1), so that nbins frac = n + g + d with d = lo + nbins pe (one fma: one
// rounding, the sign is that of the exact value) and |g + d| < 1: the bin is n where g + d >= 0 and n - 1 where it is
// negative -- a sample on or next to a bin edge, the case the rounded product gets wrong, is decided by the sign of what
// is left there.  A negative bin wraps by nbins.
// Exact for |f te| < 2^47 (beyond, pe no longer is a small correction) as long as g + d does not round to 0 from a
// non-zero value, which takes g + lo + nbins pe to cancel to 53 digits with g != 0 and nbins no power of two.
__device__ __forceinline__ int mtg_cycles_bin(double f, double te, int nbins)
{
#pragma clang fp contract(off)
    const double nb = (double)nbins;
    const double p = f * te;
    const double pe = __builtin_fma(f, te, -p);
    const double q = p - __builtin_rint(p);
    const double hi = nb * q;
    const double lo = __builtin_fma(nb, q, -hi);
    const double n = __builtin_rint(hi);
    const double s = (hi - n) + __builtin_fma(nb, pe, lo);
    int b = (int)n - (s < 0.0 ? 1 : 0);
    if (b < 0) b += nbins;
    return b < 0 ? 0 : b < nbins ? b : nbins - 1;   // (a finite product is inside already: whatever f te is, the index stays in the bins)
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
