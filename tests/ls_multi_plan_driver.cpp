// The tile planner of the Lomb-Scargle kernels (mind_the_gaps_amd/csrc/mtg_ls_plan.h) on the host: reads
// "nterms L shared weighted" lines, prints the light curves per lane; reads "slab F tile L" lines, prints the light curves
// per slab (tests/test_lomb_scargle_multi_cpu.py).
#include "mtg_ls_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int nterms, shared, weighted, tile;
        long long L, F;
        if (sscanf(line, "slab %lld %d %lld", &F, &tile, &L) == 3) {
            printf("%lld\n", (long long)mtg_ls_slab(F, tile, L));
            continue;
        }
        if (sscanf(line, "%d %lld %d %d", &nterms, &L, &shared, &weighted) != 4) return 1;
        printf("%d\n", mtg_ls_tile(nterms, L, shared, weighted));
    }
    return 0;
}
