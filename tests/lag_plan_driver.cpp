// The planner of the lag-bin sweep (mind_the_gaps_amd/csrc/mtg_lag_plan.h) on the host: reads "N nbins L shared what rows"
// lines, prints "tile all per_lc per_tile row_blocks slab ws_bytes lds_bytes blocks" (tests/test_lag_cpu.py).
#include "mtg_lag_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int nbins, shared, what;
        long long N, L, rows;
        if (sscanf(line, "%lld %d %lld %d %d %lld", &N, &nbins, &L, &shared, &what, &rows) != 6) return 1;
        const MtgLagPlan p = mtg_lag_plan(N, nbins, L, shared, what);
        printf("%d %d %d %d %lld %lld %lld %d %lld\n", p.tile, p.all, p.per_lc, p.per_tile, (long long)p.row_blocks, (long long)p.slab,
               (long long)p.ws_bytes, p.lds_bytes, (long long)mtg_lag_blocks(p, rows));
    }
    return 0;
}
