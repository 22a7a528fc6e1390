// The tile planner of the Lomb-Scargle kernels (mind_the_gaps_amd/csrc/mtg_ls_plan.h) on the host: reads
// "nterms L shared weighted" lines, prints the light curves per lane (tests/test_lomb_scargle_multi_cpu.py).
#include "mtg_ls_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int nterms, shared, weighted;
        long long L;
        if (sscanf(line, "%d %lld %d %d", &nterms, &L, &shared, &weighted) != 4) return 1;
        printf("%d\n", mtg_ls_tile(nterms, L, shared, weighted));
    }
    return 0;
}
