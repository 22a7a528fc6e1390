// mtg_cross_plan.h -- light curves per lane, instantiation, workspace and slab of the two-series lag-bin sweep
// (mtg_cross.hip, mtg_cross_sums of include/mtg.h); pure functions of the sizes: no HIP, testable on the host alone,
// tests/cross_plan_driver.cpp.  The scheme is mtg_lag_plan.h's.
//
// A lane owns a resident row i and, on shared resident sampling, a tile of R light curves.  It keeps the running sums of
// its CURRENT bin in registers -- (r_i, cf, cf2) per light curve in the light variant, and the companion's (sb, sbb) with
// everything: per light curve when the companion is per light curve, once when it is shared -- and the tile's count and
// lag once.  R = 8 in every instantiation: at most 40 doubles of the 128 that two waves per SIMD leave a lane
// (profiles/cross_resources.txt: no scratch).  sa and saa need no accumulator and no workspace: a row's partial is
// fl(r_i c) and fl(fl(r_i^2) c) with c its pair count in the bin, which the reduction forms from the count it reads anyway.
//
// Workspace: [sum][light curve of the slab][bin][row] for cf, cf2 (and sb, sbb with everything), then
// [tile of the slab][bin][row] for lag and count, every entry written exactly once -- zeros for the bins a row never
// enters.  At most MTG_CROSS_WS_BYTES = 1 GiB per slab unless one tile alone needs more; the limit is an argument so that a
// test can cut a small set into slabs.  An output entry does not depend on any of this.
// LDS of one workgroup: the chunk's companion times (2 KiB), the edges (1 KiB + 8) and the chunk's companion residuals,
// 8 bytes per column when the companion is shared and 8 R when it is per light curve: at most 19.5 KiB, static.
#ifndef MTG_CROSS_PLAN_H
#define MTG_CROSS_PLAN_H

#include <stdint.h>

#include "mtg_lag_plan.h"

enum { MTG_CROSS_CHUNK = MTG_LAG_CHUNK, MTG_CROSS_LANES = MTG_LAG_LANES, MTG_CROSS_TILE = MTG_LAG_TILE };
#define MTG_CROSS_WS_BYTES MTG_LAG_WS_BYTES
#define MTG_CROSS_MAX_M ((int64_t)1 << 28)

// which sums a call asks for, as bits; the kernel is compiled for the first four alone and for everything
enum {
    MTG_CROSS_COUNT = 1, MTG_CROSS_LAG = 2, MTG_CROSS_CF = 4, MTG_CROSS_CF2 = 8,
    MTG_CROSS_SA = 16, MTG_CROSS_SB = 32, MTG_CROSS_SAA = 64, MTG_CROSS_SBB = 128,
    MTG_CROSS_LIGHT = MTG_CROSS_COUNT | MTG_CROSS_LAG | MTG_CROSS_CF | MTG_CROSS_CF2
};

struct MtgCrossPlan : MtgLagPlan {   // all = 0: the kernel that forms count, lag, cf, cf2; 1: the one that forms sb and sbb too
    int per;               // the companion: 0 one row for every light curve, 1 a row per light curve
    int64_t chunks;        // chunks of companion columns
};

static constexpr int mtg_cross_lds_bytes(int tile, int per)
{
    return 8 * MTG_CROSS_CHUNK + 8 * (MTG_LAG_PLAN_MAX_BINS + 2) + 8 * (per ? tile : 1) * MTG_CROSS_CHUNK;
}

// N >= 1, 1 <= M < 2^28, nbins in 1 .. 128, L >= 1, `what` a non-empty set of MTG_CROSS_* bits, ws_limit >= 1 (the
// caller's checks)
static inline MtgCrossPlan mtg_cross_plan(int64_t N, int64_t M, int nbins, int64_t L, int shared_sampling, int companion_per_lc, int what,
                                          int64_t ws_limit = MTG_CROSS_WS_BYTES)
{
    const int all = (what & ~MTG_CROSS_LIGHT) ? 1 : 0;
    MtgCrossPlan p;
    static_cast<MtgLagPlan &>(p) = mtg_lag_sweep_plan(N, nbins, L, shared_sampling, all, all ? 4 : 2, 2, ws_limit);
    p.per = companion_per_lc ? 1 : 0;
    p.chunks = (M + MTG_CROSS_CHUNK - 1) / MTG_CROSS_CHUNK;
    p.lds_bytes = mtg_cross_lds_bytes(p.tile, p.per);
    return p;
}

// (tests/cross_plan_driver.cpp's name for it)
static inline int64_t mtg_cross_blocks(const MtgCrossPlan &p, int64_t rows) { return mtg_lag_blocks(p, rows); }

#endif
