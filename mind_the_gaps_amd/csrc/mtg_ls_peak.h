// mtg_ls_peak.h -- the largest of value(k), k in [0, n), over a workgroup of T lanes and the first k that attains it:
// NaN is passed over, ties go to the lower index.  The rows of mtg_lomb_scargle_peak_kernel (the powers) and of
// mtg_ls_envelope_ratio_peak_kernel (power / scale) are reduced by it.
#ifndef MTG_LS_PEAK_H
#define MTG_LS_PEAK_H

#include "mtg_device.h"

// -> *peak and *at in every lane (nothing but NaN: *at = -1, and *peak means nothing)
template <int T, class Value>
__device__ __forceinline__ void ls_block_peak(int64_t n, Value value, double *peak, int64_t *at)
{
    __shared__ double bv[T];
    __shared__ int64_t bi[T];
    const int tid = threadIdx.x;
    double v = 0.0;
    int64_t vi = -1;
    for (int64_t k = tid; k < n; k += T) {
        const double x = value(k);
        if (x == x && (vi < 0 || x > v)) { v = x; vi = k; }
    }
    bv[tid] = v; bi[tid] = vi;
    __syncthreads();
    for (int h = T / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double x = bv[tid + h];
            const int64_t xi = bi[tid + h];
            if (xi >= 0 && (bi[tid] < 0 || x > bv[tid] || (x == bv[tid] && xi < bi[tid]))) { bv[tid] = x; bi[tid] = xi; }
        }
        __syncthreads();
    }
    *peak = bv[0];
    *at = bi[0];
}

#endif
