// The cutting rules of mtg_lomb_scargle_envelope (mind_the_gaps_amd/csrc/mtg_ls_envelope_plan.h) on the host: reads
// "L F Q budget" lines, prints "in_lds columns pow2 width workspace" (tests/test_lomb_scargle_envelope_cpu.py).  A first
// line "constants" prints MTG_LSE_BUDGET, MTG_LSE_LDS_KEYS, MTG_LSE_MAX_COLS and MTG_LSE_THREADS.
#include "mtg_ls_envelope_plan.h"

#include <stdio.h>
#include <string.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "constants", 9)) {
            printf("%lld %d %d %d\n", (long long)MTG_LSE_BUDGET, MTG_LSE_LDS_KEYS, MTG_LSE_MAX_COLS, MTG_LSE_THREADS);
            continue;
        }
        long long L, F, Q, budget;
        if (sscanf(line, "%lld %lld %lld %lld", &L, &F, &Q, &budget) != 4) return 1;
        const long long w = mtg_lse_slab_width(L, F, Q, budget);
        printf("%d %d %lld %lld %lld\n", mtg_lse_in_lds(L), mtg_lse_columns(L), (long long)mtg_lse_pow2(L), w,
               (long long)mtg_lse_workspace_bytes(L, Q, w));
    }
    return 0;
}
