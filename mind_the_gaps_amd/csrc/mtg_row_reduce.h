// mtg_row_reduce.h -- the rows' partials of one (light curve, bin) added in an order fixed by the number of rows alone:
// what the reductions of the lag-bin sweep (mtg_lag.hip) and of the two-series sweep (mtg_cross.hip) share.  Lane q of
// MTG_LAG_LANES takes the rows q, q + 256, ... ascending from zero, then a binary tree over the lanes.  No atomics; the
// same sequence of additions whatever the launch looks like.
#ifndef MTG_ROW_REDUCE_H
#define MTG_ROW_REDUCE_H

#include "mtg_device.h"
#include "mtg_lag_plan.h"

// sum of v over the workgroup in a fixed order (a binary tree over the lanes): `red` holds MTG_LAG_LANES entries
template <class V>
__device__ __forceinline__ V lag_block_sum(V v, V *red)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = MTG_LAG_LANES / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// term(n) of the rows q, q + 256, ... ascending per lane, then the tree
template <class V, class F>
__device__ __forceinline__ V lag_row_sum_of(int64_t N, V *red, F term)
{
#pragma clang fp contract(off)
    V s = 0;
    for (int64_t n = threadIdx.x; n < N; n += MTG_LAG_LANES) s = s + term(n);
    return lag_block_sum(s, red);
}

// ... of the stored partials rows[0 .. N)
template <class V>
__device__ __forceinline__ V lag_row_sum(const V *rows, int64_t N, V *red)
{
    return lag_row_sum_of(N, red, [rows](int64_t n) { return rows[n]; });
}

#endif
