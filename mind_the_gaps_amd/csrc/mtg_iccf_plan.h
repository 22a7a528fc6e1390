// mtg_iccf_plan.h -- light curves per lane, instantiation, grid and slab of the interpolated cross-correlation
// (mtg_iccf.hip, mtg_iccf of include/mtg.h); pure functions of the sizes: no HIP, testable on the host alone,
// tests/iccf_plan_driver.cpp.  The scheme is mtg_cross_plan.h's.
//
// A lane owns a lag and, on shared resident sampling, a tile of R light curves; a workgroup MTG_ICCF_LANES lags.  It keeps
// the six running sums of the half it is walking in registers: three per light curve (the sums that hold the resident
// residual) and, when the companion is one row for every light curve, the other two and the count once per tile; with a
// companion row per light curve all five are per light curve.  R = 4 at most: 20 doubles of sums and 4 of finished
// half-A values, of the 128 that two waves per SIMD leave a lane; at R = 8 the rows' pointers and means no longer fit
// the scalar registers (profiles/iccf_resources.txt: no scratch, no spills, four waves per SIMD or more).
// Nothing is staged: the bracket nodes are plain cached gathers, the sample of a step is the same for the whole wave.
// No LDS, no workspace beyond the outputs.
//
// Slab.  The device copies of the [L][K] outputs (the values, which the peaks are reduced from, and whichever counts are
// asked for) stay within MTG_ICCF_OUT_BYTES = 256 MiB unless one tile alone needs more; the limit is an argument so that
// a test can cut a small set in two.  An output entry does not depend on any of this.
#ifndef MTG_ICCF_PLAN_H
#define MTG_ICCF_PLAN_H

#include <stdint.h>

enum { MTG_ICCF_LANES = 256, MTG_ICCF_TILE = 4, MTG_ICCF_PLAN_MAX_LAGS = 65536 };
#define MTG_ICCF_OUT_BYTES ((int64_t)1 << 28)
#define MTG_ICCF_MAX_M ((int64_t)1 << 28)

struct MtgIccfPlan {
    int tile;              // light curves per lane: 1 or MTG_ICCF_TILE
    int per;               // the companion: 0 one row for every light curve, 1 a row per light curve
    int all;               // 0: the kernel that walks half A alone (the companion interpolated); 1: the one that walks both
    int arrays;            // [slab][K] arrays of 8-byte entries on the device: 1 .. 3
    int64_t lag_blocks;    // workgroups along the lags
    int64_t slab;          // light curves per slab: whole tiles, at most L
    int64_t out_bytes;     // of one slab's arrays
    int lds_bytes;         // of one workgroup: none
};

// K in 1 .. 65536, L >= 1, arrays in 1 .. 3, out_limit >= 1 (the caller's checks); half_a_only: the mode forms r_A alone
static inline MtgIccfPlan mtg_iccf_plan(int64_t K, int64_t L, int shared_sampling, int companion_per_lc, int half_a_only, int arrays,
                                        int64_t out_limit = MTG_ICCF_OUT_BYTES)
{
    MtgIccfPlan p;
    p.tile = !shared_sampling || L == 1 ? 1 : MTG_ICCF_TILE;
    p.per = companion_per_lc ? 1 : 0;
    p.all = half_a_only ? 0 : 1;
    p.arrays = arrays;
    p.lag_blocks = (K + MTG_ICCF_LANES - 1) / MTG_ICCF_LANES;
    int64_t rows = out_limit / ((int64_t)arrays * K * 8 * p.tile) * p.tile;
    if (rows < p.tile) rows = p.tile;
    p.slab = rows > L ? L : rows;
    p.out_bytes = (int64_t)arrays * p.slab * K * 8;
    p.lds_bytes = 0;
    return p;
}

// workgroups of a launch over `rows` light curves (0: more than a grid holds)
static inline int64_t mtg_iccf_blocks(const MtgIccfPlan &p, int64_t rows)
{
    const int64_t tiles = (rows + p.tile - 1) / p.tile;
    return p.lag_blocks > 0x7fffffff / tiles ? 0 : p.lag_blocks * tiles;
}

#endif
