// mtg_ls_multi_plan.h -- light curves per lane of the multi-harmonic Lomb-Scargle kernel (mtg_lomb_scargle_multi.hip;
// pure functions of the sizes: no HIP, testable on the host alone, tests/ls_multi_plan_driver.cpp).
//
// A lane keeps, for K harmonics, the 4 K trigonometric sums C_m, S_m (m = 1 .. 2 K) and 2 K data sums per light curve,
// each twice (running total and the chunk's partial sum): 2 x 6 K R doubles when every light curve has weights of its
// own, 2 x (2 K R + 4 K) when the weights are 1 / N and the trigonometric sums are the tile's.  Two waves per SIMD
// leave a lane 256 registers = 128 doubles; what the phase, the harmonic recurrence and the chunk's operands need on
// top is ~ 30, so that the sums may take 96 (the K = 1 kernel's R = 8 weighted is 96 too).  The unweighted chunk is
// staged as pairs of light curves: R even there.
//   weighted    K = 2: 24 R, R = 4 (96)   K = 3: 36 R, R = 2 (72)   K = 4: 48 R, R = 2 (96)   K = 5: 60 R, R = 1 (60)
//   unweighted  K = 2: 8 R + 16, R = 10 (96)   K = 3: 12 R + 24, R = 6 (96)   K = 4: 16 R + 32, R = 4 (96)
//               K = 5: 20 R + 40, R = 2 (80)
// profiles/lomb_scargle_multi_resources.txt is the compiler's report of every instantiation (no scratch).
#ifndef MTG_LS_MULTI_PLAN_H
#define MTG_LS_MULTI_PLAN_H

#include <stdint.h>

// the full tile of (K, weighted), K in 2 .. 5 (0 otherwise)
static constexpr int mtg_ls_multi_full_tile(int nterms, int weighted)
{
    switch (nterms) {
    case 2: return weighted ? 4 : 10;
    case 3: return weighted ? 2 : 6;
    case 4: return weighted ? 2 : 4;
    case 5: return weighted ? 1 : 2;
    default: return 0;
    }
}

// light curves per lane for a set of L: 1 where every light curve has a sampling of its own or there is only one, the
// full tile otherwise.  A power does not depend on the tile.
static inline int mtg_ls_multi_tile(int nterms, int64_t L, int shared_sampling, int weighted)
{
    if (!shared_sampling || L <= 1) return 1;
    return mtg_ls_multi_full_tile(nterms, weighted);
}

#endif
