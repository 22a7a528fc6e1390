// mtg_sweep_step.h -- the pieces of the serial sweep that its kernels share as functions: the one-lane-per-evaluation
// sweep (mtg_sweep.h), its two-wave pipeline (mtg_sweep_pipe.h) and the white kernel (mtg_kernels.hip) read their
// samples through mtg_ld128 and turn their sums into lnL and a status in mtg_finish_lnl.
#ifndef MTG_SWEEP_STEP_H
#define MTG_SWEEP_STEP_H

#include "mtg_device.h"
#include "mtg_math.h"

#include <math.h>

#define MTG_LN_2PI 1.8378770664093454835606594728112

// 16 bytes through a buffer descriptor: resource in SGPRs, voff per lane, soff on the scalar unit -- no VALU
// instruction is spent on addressing, and the hardware range check makes a load past the end a harmless zero
__device__ __forceinline__ double2 mtg_ld128(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// lnL and status from the sums of a whole light curve: dot = r^T K^-1 r, ln det K = ln dprod + dexp ln 2
__device__ __forceinline__ void mtg_finish_lnl(int64_t N, double dot, double dprod, int dexp, int dmin_hi, double *ll,
                                               int *status)
{
#pragma clang fp contract(off)
    const double logdet = fma((double)dexp, 0.69314718055994530942, log(dprod));
    double v = -0.5 * fma((double)N, MTG_LN_2PI, dot + logdet);
    int st = MTG_ST_OK;
    if (dmin_hi <= 0) { st = MTG_ST_NOTPD; v = -INFINITY; }
    else if (!isfinite(v)) { st = MTG_ST_NONFINITE; v = -INFINITY; }
    *ll = v;
    *status = st;
}

#endif  // MTG_SWEEP_STEP_H
