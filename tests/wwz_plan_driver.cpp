// The planner of the weighted wavelet Z-transform (mind_the_gaps_amd/csrc/mtg_wwz_plan.h) on the host: reads
// "F T L shared weighted rows" lines, prints "tile lanes nfb slab lds_bytes blocks" (tests/test_wwz_cpu.py).
#include "mtg_wwz_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int shared, weighted;
        long long F, T, L, rows;
        if (sscanf(line, "%lld %lld %lld %d %d %lld", &F, &T, &L, &shared, &weighted, &rows) != 6) return 1;
        const MtgWwzPlan p = mtg_wwz_plan(F, T, L, shared, weighted);
        printf("%d %d %lld %lld %d %lld\n", p.tile, p.lanes, (long long)p.nfb, (long long)p.slab, p.lds_bytes, (long long)mtg_wwz_blocks(p, T, rows));
    }
    return 0;
}
