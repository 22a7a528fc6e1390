// The planner of the epoch-folding sweep (mind_the_gaps_amd/csrc/mtg_ef_plan.h) on the host: reads
// "nbins F L shared weighted" lines, prints "tile lanes acc_bytes lds_bytes" (tests/test_epoch_fold_cpu.py).
#include "mtg_ef_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int nbins, shared, weighted;
        long long F, L;
        if (sscanf(line, "%d %lld %lld %d %d", &nbins, &F, &L, &shared, &weighted) != 5) return 1;
        const MtgEfPlan p = mtg_ef_plan(nbins, F, L, shared, weighted);
        printf("%d %d %d %d\n", p.tile, p.lanes, p.acc_bytes, p.lds_bytes);
    }
    return 0;
}
