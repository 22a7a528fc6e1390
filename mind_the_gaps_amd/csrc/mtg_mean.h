// mtg_mean.h -- the profile means (MTG_MEAN_SINE, MTG_MEAN_TWOSINE, MTG_MEAN_GAUSSIAN of include/mtg.h): how many
// parameters and coefficient slots each takes, and the per-row constants the sweep wants, derived once per row from the
// parameters -- on the device by mtg_prepare_from (mtg_prepare.h), on the host by mtg_loglike_coeffs' staging.
//
// Slots: mean(0) holds 0 and mean(1) the profile's constant level, so that everything that reads the two affine slots
// (mtg_apply_inverse's factorisation) sees a constant mean; the further constants sit in mean_extra(i) (mtg_device.h):
//   sine      w, A cos p, A sin p                      A sin(w t + p) = (A cos p) sin(w t) + (A sin p) cos(w t)
//   two sines w, A0 cos p0, A0 sin p0, A1 cos p1, A1 sin p1          (sin, cos)(2 w t) from the double-angle formulas
//   Gaussian  mu, amplitude / (2 pi sigma), q_hi, q_lo  with q = -1 / (2 sigma^2) in units of ln2 / (8 N_exp), the table
//             exp's own (mtg_math.h), as a double-double: the exponent (t - mu)^2 q then carries the rounding of t - mu only
#pragma once
#include "mtg_device.h"
#include "mtg_math.h"

#include <math.h>

__host__ __device__ constexpr int mtg_mean_nparams_of(int kind)
{
    return kind == MTG_MEAN_CONSTANT ? 1 : kind == MTG_MEAN_LINEAR ? 2 : kind == MTG_MEAN_SINE ? 4 :
           kind == MTG_MEAN_TWOSINE ? 6 : kind == MTG_MEAN_GAUSSIAN ? 4 : -1;
}
__host__ __device__ constexpr bool mtg_mean_is_profile(int kind)
{
    return kind == MTG_MEAN_SINE || kind == MTG_MEAN_TWOSINE || kind == MTG_MEAN_GAUSSIAN;
}
__host__ __device__ constexpr int mtg_mean_extra_slots(int kind)
{
    return kind == MTG_MEAN_SINE ? 3 : kind == MTG_MEAN_TWOSINE ? 5 : kind == MTG_MEAN_GAUSSIAN ? 4 : 0;
}
static inline const char *mtg_mean_name(int kind)
{
    return kind == MTG_MEAN_SINE ? "MTG_MEAN_SINE" : kind == MTG_MEAN_TWOSINE ? "MTG_MEAN_TWOSINE" :
           kind == MTG_MEAN_GAUSSIAN ? "MTG_MEAN_GAUSSIAN" : kind == MTG_MEAN_LINEAR ? "MTG_MEAN_LINEAR" : "MTG_MEAN_CONSTANT";
}

// low part of 8 N_exp / ln2 (MTG_EXP_CSCALE is the double nearest to it)
#define MTG_EXP_CSCALE_LO (0x1.777d0ffda0d24p-53 * MTG_EXP_N)

// The level and the mtg_mean_extra_slots(kind) constants of one row, by value: no address of a local leaves the caller
struct MtgMeanConsts {
    double level, ex0, ex1, ex2, ex3, ex4;
    __host__ __device__ double ex(int i) const { return i == 0 ? ex0 : i == 1 ? ex1 : i == 2 ? ex2 : i == 3 ? ex3 : ex4; }
};

// p0 .. p5: the kind's parameters in the reference's order (those it does not have: anything)
__host__ __device__ inline MtgMeanConsts mtg_mean_derive(int kind, double p0, double p1, double p2, double p3, double p4, double p5)
{
    MtgMeanConsts r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (kind == MTG_MEAN_SINE) {            // constant, amplitude, frequency, phase
        r.level = p0;
        r.ex0 = p2;
        r.ex1 = p1 * cos(p3);
        r.ex2 = p1 * sin(p3);
    } else if (kind == MTG_MEAN_TWOSINE) {  // constant, amplitude0, phase0, amplitude1, phase1, frequency
        r.level = p0;
        r.ex0 = p5;
        r.ex1 = p1 * cos(p2);
        r.ex2 = p1 * sin(p2);
        r.ex3 = p3 * cos(p4);
        r.ex4 = p3 * sin(p4);
    } else {                                // MTG_MEAN_GAUSSIAN: mean, sigma, amplitude, constant
        const double sg = p1;
        r.level = p3;
        r.ex0 = p0;
        r.ex1 = p2 / (2.0 * 3.14159265358979323846 * sg);   // the reference's normalisation 2 pi sigma, kept as is
        // q = -(K + K_lo) / (2 sigma^2), sigma^2 = s2 + e exactly
        const double s2 = sg * sg, e = fma(sg, sg, -s2), D = 2.0 * s2, De = 2.0 * e;
        const double qh = -MTG_EXP_CSCALE / D;
        const double ql = (fma(-qh, D, -MTG_EXP_CSCALE) - MTG_EXP_CSCALE_LO - qh * De) / D;
        r.ex2 = qh;
        r.ex3 = ql - ql == 0.0 ? ql : 0.0;  // (sigma = 0 or huge: the high part and the normalisation speak for the row)
    }
    return r;
}
