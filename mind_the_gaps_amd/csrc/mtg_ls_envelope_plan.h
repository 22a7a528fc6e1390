// mtg_ls_envelope_plan.h -- how mtg_lomb_scargle_envelope cuts its work (pure functions of the sizes: no HIP, testable on
// the host alone, tests/ls_envelope_plan_driver.cpp).
//
// The entry walks the F frequencies in slabs of Fs columns; a slab holds the power of ALL L light curves at its
// frequencies, [L][Fs] doubles, and the Q order statistics asked for, [Q][Fs].  Up to MTG_LSE_LDS_KEYS light curves a
// column is sorted in LDS (a workgroup carries mtg_lse_columns(L) columns, each padded to a power of two); beyond that
// the slab is transposed into 64-bit keys and sorted by segments, which takes two more arrays of the slab's size.
#ifndef MTG_LS_ENVELOPE_PLAN_H
#define MTG_LS_ENVELOPE_PLAN_H

#include <stdint.h>

// device workspace of a call that scales with L Fs, whatever L F is (the rule of mtg_lomb_scargle's 256 MiB; smaller, so
// that the test that crosses it stays small)
#define MTG_LSE_BUDGET ((int64_t)64 << 20)
// keys of one workgroup in LDS: 128 KiB of the CU's 160
#define MTG_LSE_LDS_KEYS 16384
// columns a workgroup carries at most: 32 x 8 bytes = one 256-byte run per row of the slab
#define MTG_LSE_MAX_COLS 32
#define MTG_LSE_THREADS 512

// the smallest power of two >= L (L >= 1)
static inline int64_t mtg_lse_pow2(int64_t L)
{
    int64_t p = 1;
    while (p < L) p <<= 1;
    return p;
}

// 1: columns of L light curves are sorted in LDS; 0: by segments in global memory
static inline int mtg_lse_in_lds(int64_t L) { return L >= 1 && L <= MTG_LSE_LDS_KEYS; }

// columns per workgroup on the LDS path: the power of two that fills MTG_LSE_LDS_KEYS keys with padded columns, at most
// MTG_LSE_MAX_COLS (0 on the other path)
static inline int mtg_lse_columns(int64_t L)
{
    if (!mtg_lse_in_lds(L)) return 0;
    const int64_t c = MTG_LSE_LDS_KEYS / mtg_lse_pow2(L);
    return (int)(c > MTG_LSE_MAX_COLS ? MTG_LSE_MAX_COLS : c);
}

// bytes of workspace a column of the slab costs: its powers, its Q order statistics and, beyond LDS, the two key arrays
static inline int64_t mtg_lse_column_bytes(int64_t L, int64_t Q) { return 8 * ((mtg_lse_in_lds(L) ? 1 : 3) * L + Q); }

// columns per slab: as many as the budget holds, at least 1 (a single column of more than the budget is the one case
// that exceeds it), at most F
static inline int64_t mtg_lse_slab_width(int64_t L, int64_t F, int64_t Q, int64_t budget)
{
    int64_t w = budget / mtg_lse_column_bytes(L, Q);
    if (w > F) w = F;
    return w < 1 ? 1 : w;
}

static inline int64_t mtg_lse_workspace_bytes(int64_t L, int64_t Q, int64_t Fs) { return Fs * mtg_lse_column_bytes(L, Q); }

#endif
