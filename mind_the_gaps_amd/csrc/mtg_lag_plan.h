// mtg_lag_plan.h -- light curves per lane, workspace and slab of the lag-bin sweep (mtg_lag.hip, mtg_lag_sums of
// include/mtg.h); pure functions of the sizes: no HIP, testable on the host alone, tests/lag_plan_driver.cpp.
//
// A lane owns a row i of the pair matrix and, on shared sampling, a tile of R light curves.  It keeps the running sums
// of its CURRENT bin in registers -- (y_i, sf) per light curve with the structure function alone, (y_i, r_i, sigma_i^2,
// sf, cf, cf2, noise) with everything, and the tile's count and lag once -- and touches memory only when its bin
// changes: R = 8 either way, 16 or 56 doubles of the 128 two waves per SIMD leave a lane
// (profiles/lag_resources.txt: no scratch).
//
// Where a row's partial for a bin goes: a global workspace, [light curve of the slab][bin][row] per sum asked for and
// [tile of the slab][bin][row] for count and lag (they depend on the sampling alone), every entry written exactly once --
// zeros for the bins a row never enters -- and reduced over the rows by a second kernel in an order fixed by N.  The
// other candidate, partials in LDS as [bin][lane] reduced per row block, was not built: at 8 bytes per (sum, light
// curve, bin, lane) one light curve's structure function at 128 bins and 256 lanes already takes 256 KiB, more than the
// 160 KiB of a CU, and every sum of a tile of 8 takes 40 times that; it would force one-wave workgroups of one light curve
// at the bin counts the entry allows, and give up sharing tau and the bin decision across a tile.
//
// Slab.  The workspace is MTG_LAG_WS_BYTES = 1 GiB at most -- unless one tile alone needs more: larger than the
// 256 MiB of the periodogram entries, because a slab has to fill the device with (row block, tile) workgroups and a light
// curve of N = 10^4 at 50 bins takes 4 MB per sum.  An output entry does not depend on any of this.
// LDS of one workgroup: the chunk's times (2 KiB), the edges (1 KiB + 8) and the chunk's columns, 8 R bytes per sample
// with the structure function alone and 24 R with everything: at most 51 KiB, static.
#ifndef MTG_LAG_PLAN_H
#define MTG_LAG_PLAN_H

#include <stdint.h>

enum { MTG_LAG_CHUNK = 256, MTG_LAG_LANES = 256, MTG_LAG_TILE = 8, MTG_LAG_PLAN_MAX_BINS = 128 };
#define MTG_LAG_WS_BYTES ((int64_t)1 << 30)

// which sums a call asks for, as bits; the kernel is compiled for MTG_LAG_SF alone and for everything
enum { MTG_LAG_COUNT = 1, MTG_LAG_LAG = 2, MTG_LAG_SF = 4, MTG_LAG_CF = 8, MTG_LAG_CF2 = 16, MTG_LAG_NOISE = 32 };

// what both pair sweeps plan (mtg_lag.hip, mtg_cross.hip): mtg_cross_plan.h extends it
struct MtgLagPlan {
    int tile;              // light curves per lane: 1, 4 or MTG_LAG_TILE
    int all;               // 0: the lighter kernel of the entry; 1: the one that forms every sum
    int per_lc;            // workspace arrays with an entry per light curve
    int per_tile;          // ... and per tile: 0 or 2 (lag, count)
    int64_t row_blocks;    // workgroups along the rows
    int64_t slab;          // light curves per slab: whole tiles, at most L
    int64_t ws_bytes;      // of one slab
    int lds_bytes;         // of one workgroup
};

static constexpr int mtg_lag_lds_bytes(int tile, int all)
{
    return 8 * MTG_LAG_CHUNK + 8 * (MTG_LAG_PLAN_MAX_BINS + 2) + (all ? 24 : 8) * tile * MTG_LAG_CHUNK;
}

// bytes of workspace of `rows` light curves in tiles of `tile`
static inline int64_t mtg_lag_ws_bytes(int64_t N, int nbins, int tile, int per_lc, int per_tile, int64_t rows)
{
    return ((int64_t)per_lc * rows + (int64_t)per_tile * ((rows + tile - 1) / tile)) * nbins * N * 8;
}

// The tile and the slab of a sweep over N rows that keeps per_lc + per_tile arrays, in at most ws_limit bytes of workspace
// unless one tile alone needs more (lds_bytes is the caller's).
static inline MtgLagPlan mtg_lag_sweep_plan(int64_t N, int nbins, int64_t L, int shared_sampling, int all, int per_lc, int per_tile,
                                            int64_t ws_limit)
{
    MtgLagPlan p;
    p.tile = !shared_sampling || L == 1 ? 1 : L <= 4 ? 4 : MTG_LAG_TILE;
    p.all = all;
    p.per_lc = per_lc;
    p.per_tile = per_tile;
    p.row_blocks = (N + MTG_LAG_LANES - 1) / MTG_LAG_LANES;
    int64_t rows = ws_limit / mtg_lag_ws_bytes(N, nbins, p.tile, p.per_lc, p.per_tile, p.tile) * p.tile;
    if (rows < p.tile) rows = p.tile;
    p.slab = rows > L ? L : rows;
    p.ws_bytes = mtg_lag_ws_bytes(N, nbins, p.tile, p.per_lc, p.per_tile, p.slab);
    p.lds_bytes = 0;
    return p;
}

// nbins in 1 .. 128, N >= 2, L >= 1, `what` a non-empty set of MTG_LAG_* bits (the caller's checks)
static inline MtgLagPlan mtg_lag_plan(int64_t N, int nbins, int64_t L, int shared_sampling, int what)
{
    const int all = (what & ~MTG_LAG_SF) ? 1 : 0;
    MtgLagPlan p = mtg_lag_sweep_plan(N, nbins, L, shared_sampling, all, all ? 4 : 1, all ? 2 : 0, MTG_LAG_WS_BYTES);
    p.lds_bytes = mtg_lag_lds_bytes(p.tile, p.all);
    return p;
}

// workgroups of a launch over `rows` light curves (0: more than a grid holds)
static inline int64_t mtg_lag_blocks(const MtgLagPlan &p, int64_t rows)
{
    const int64_t tiles = (rows + p.tile - 1) / p.tile;
    return p.row_blocks > 0x7fffffff / tiles ? 0 : p.row_blocks * tiles;
}

// Whether the slab [l0, l0 + Ls) of a set of L light curves of N samples can be launched with this plan: the sizes in
// range, the plan the one its planner makes for them, the workspace within the plan's.  -> its workgroups, 0 if not.
static inline int64_t mtg_lag_launch_blocks(const MtgLagPlan &p, int64_t N, int64_t t_stride, int64_t L, int nbins, int64_t l0, int64_t Ls)
{
    if (nbins < 1 || nbins > MTG_LAG_PLAN_MAX_BINS || N < 1 || Ls < 1 || l0 < 0 || l0 + Ls > L || Ls > 0x7fffffff / nbins ||
        p.tile < 1 || (p.tile != 1 && t_stride != 0) ||
        p.row_blocks != (N + MTG_LAG_LANES - 1) / MTG_LAG_LANES ||
        mtg_lag_ws_bytes(N, nbins, p.tile, p.per_lc, p.per_tile, Ls) > p.ws_bytes)
        return 0;
    return mtg_lag_blocks(p, Ls);
}

#endif
