// mtg_wwz_plan.h -- light curves per lane, lanes per workgroup, slab and grid of the weighted wavelet Z-transform
// (mtg_wwz.hip); pure functions of the sizes: no HIP, testable on the host alone, tests/wwz_plan_driver.cpp.
//
// A lane owns a frequency of one window centre tau and keeps, each twice (running total and the chunk's partial sum),
//   weighted     ten sums per light curve (sum w, sum w^2, C, S, CC, CS and X, XX, XC, XS): 2 x 10 R doubles, R = 4 (80);
//   unweighted   the six weight and trigonometric sums once per tile and four data sums per light curve:
//                2 x (4 R + 6) doubles, R = 8 (76)
// of the 128 doubles two waves per SIMD leave a lane; the phase, the exponential and the chunk's operands take the rest
// (profiles/wwz_resources.txt: no scratch).  The unweighted chunk is staged as pairs of light curves: R even or 1.
// LDS: the 32 KiB (cos, sin) table, 2 KiB of elapsed times, 2 KiB of te^2 - te_*^2 and 4 KiB per weighted light curve or
// unweighted pair: 52 KiB with the reduction's words, two workgroups on a CU's 160 KiB.
//
// Grid: frequency blocks fastest, then the centres, then the tiles of light curves, in one dimension.  The maps of a slab
// of light curves at a time keep the workspace at 2 x 256 MiB (values and N_eff) whatever L T F is -- unless one tile's
// maps alone are larger.  An entry of the output does not depend on any of this.
#ifndef MTG_WWZ_PLAN_H
#define MTG_WWZ_PLAN_H

#include <stdint.h>

enum { MTG_WWZ_CHUNK = 256, MTG_WWZ_MAX_LANES = 256, MTG_WWZ_TILE_WEIGHTED = 4, MTG_WWZ_TILE_UNWEIGHTED = 8 };
#define MTG_WWZ_SLAB_ENTRIES ((int64_t)1 << 25)

struct MtgWwzPlan {
    int tile;         // light curves per lane: 1, or the full tile of the weighting
    int lanes;        // 64, 128 or 256
    int64_t nfb;      // workgroups along the frequencies
    int64_t slab;     // light curves per slab: whole tiles, at most L
    int lds_bytes;    // of one workgroup
};

static constexpr int mtg_wwz_full_tile(int weighted) { return weighted ? MTG_WWZ_TILE_WEIGHTED : MTG_WWZ_TILE_UNWEIGHTED; }

// bytes of LDS of one workgroup: table, elapsed times, exponents' te part, columns, the chunk range's words
static constexpr int mtg_wwz_lds_bytes(int tile, int weighted)
{
    return 32768 + 2 * 8 * MTG_WWZ_CHUNK + 16 * MTG_WWZ_CHUNK * (weighted ? tile : (tile + 1) / 2) + 8 * MTG_WWZ_MAX_LANES + 8;
}

// F, T, L >= 1 with T F < 2^63 (the caller's checks)
static inline MtgWwzPlan mtg_wwz_plan(int64_t F, int64_t T, int64_t L, int shared_sampling, int weighted)
{
    MtgWwzPlan p;
    p.tile = shared_sampling && L > 1 ? mtg_wwz_full_tile(weighted) : 1;
    p.lanes = F <= 64 ? 64 : F <= 128 ? 128 : MTG_WWZ_MAX_LANES;
    p.nfb = (F + p.lanes - 1) / p.lanes;
    int64_t rows = MTG_WWZ_SLAB_ENTRIES / F / T;
    rows = rows / p.tile * p.tile;
    if (rows < p.tile) rows = p.tile;
    p.slab = rows > L ? L : rows;
    p.lds_bytes = mtg_wwz_lds_bytes(p.tile, weighted);
    return p;
}

// workgroups of a launch over `rows` light curves (0: more than a grid holds)
static inline int64_t mtg_wwz_blocks(const MtgWwzPlan &p, int64_t T, int64_t rows)
{
    const int64_t tiles = (rows + p.tile - 1) / p.tile;
    if (p.nfb > 0x7fffffff / T || p.nfb * T > 0x7fffffff / tiles) return 0;
    return p.nfb * T * tiles;
}

#endif
