// mtg_ls_plan.h -- light curves per lane of the Lomb-Scargle tile sweep (mtg_ls_tile.h), for one term
// (mtg_lomb_scargle.hip) and K = 2 .. 5 harmonics (mtg_lomb_scargle_multi.hip); pure functions of the sizes: no HIP,
// testable on the host alone, tests/ls_multi_plan_driver.cpp.
//
// A lane keeps, for K harmonics, the 4 K trigonometric sums C_m, S_m (m = 1 .. 2 K) and 2 K data sums per light curve,
// each twice (running total and the chunk's partial sum): 2 x 6 K R doubles when every light curve has weights of its
// own, 2 x (2 K R + 4 K) when the weights are 1 / N and the trigonometric sums are the tile's.  Two waves per SIMD
// leave a lane 256 registers = 128 doubles; what the phase, the harmonic recurrence and the chunk's operands need on
// top is ~ 30, so that the sums may take 96.  The unweighted chunk is staged as pairs of light curves: R even there.
//   weighted    K = 2: 24 R, R = 4 (96)   K = 3: 36 R, R = 2 (72)   K = 4: 48 R, R = 2 (96)   K = 5: 60 R, R = 1 (60)
//   unweighted  K = 2: 8 R + 16, R = 10 (96)   K = 3: 12 R + 24, R = 6 (96)   K = 4: 16 R + 32, R = 4 (96)
//               K = 5: 20 R + 40, R = 2 (80)
// One term carries four trigonometric sums (C, S, sum w c^2, sum w c s) and two data sums: 2 x 6 R weighted, R = 8 (96),
// 2 x (2 R + 4) unweighted, R = 16 (72), and a tile of 4 for sets of up to four light curves.
// profiles/lomb_scargle_resources.txt and profiles/lomb_scargle_multi_resources.txt are the compiler's reports of every
// instantiation (no scratch).
#ifndef MTG_LS_PLAN_H
#define MTG_LS_PLAN_H

#include <stdint.h>

// the full tile of (K, weighted), K in 1 .. 5 (0 otherwise)
static constexpr int mtg_ls_full_tile(int nterms, int weighted)
{
    switch (nterms) {
    case 1: return weighted ? 8 : 16;
    case 2: return weighted ? 4 : 10;
    case 3: return weighted ? 2 : 6;
    case 4: return weighted ? 2 : 4;
    case 5: return weighted ? 1 : 2;
    default: return 0;
    }
}

// light curves per lane for a set of L: 1 where every light curve has a sampling of its own or there is only one, the
// full tile otherwise -- with one term, 4 for L <= 4.  A power does not depend on the tile.  0: no kernel for nterms.
static inline int mtg_ls_tile(int nterms, int64_t L, int shared_sampling, int weighted)
{
    const int full = mtg_ls_full_tile(nterms, weighted);
    if (full == 0) return 0;
    if (!shared_sampling || L <= 1) return 1;
    if (nterms == 1 && L <= 4) return 4;
    return full;
}

// The powers of a slab of light curves at a time (mtg_lomb_scargle, mtg_epoch_fold): at most MTG_LS_SLAB_ENTRIES of them,
// 256 MiB of workspace whatever L F is.  -> light curves per slab: whole tiles (a light curve's power does not depend on
// its tile: this only fills the lanes), at least one tile, at most L.
static constexpr int64_t MTG_LS_SLAB_ENTRIES = (int64_t)1 << 25;

static inline int64_t mtg_ls_slab(int64_t F, int tile, int64_t L)
{
    int64_t slab = MTG_LS_SLAB_ENTRIES / F / tile * tile;
    if (slab < tile) slab = tile;
    return slab < L ? slab : L;
}

#endif
