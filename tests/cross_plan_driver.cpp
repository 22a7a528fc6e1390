// The planner of the two-series lag-bin sweep (mind_the_gaps_amd/csrc/mtg_cross_plan.h) on the host: reads
// "N M nbins L shared per what rows ws_limit" lines (ws_limit 0: the default), prints
// "tile per all per_lc per_tile row_blocks chunks slab ws_bytes lds_bytes blocks" (tests/test_cross_cpu.py).
#include "mtg_cross_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int nbins, shared, per, what;
        long long N, M, L, rows, limit;
        if (sscanf(line, "%lld %lld %d %lld %d %d %d %lld %lld", &N, &M, &nbins, &L, &shared, &per, &what, &rows, &limit) != 9) return 1;
        const MtgCrossPlan p = limit ? mtg_cross_plan(N, M, nbins, L, shared, per, what, limit) : mtg_cross_plan(N, M, nbins, L, shared, per, what);
        printf("%d %d %d %d %d %lld %lld %lld %lld %d %lld\n", p.tile, p.per, p.all, p.per_lc, p.per_tile, (long long)p.row_blocks,
               (long long)p.chunks, (long long)p.slab, (long long)p.ws_bytes, p.lds_bytes, (long long)mtg_cross_blocks(p, rows));
    }
    return 0;
}
