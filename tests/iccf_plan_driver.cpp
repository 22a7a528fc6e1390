// The planner of the interpolated cross-correlation (mind_the_gaps_amd/csrc/mtg_iccf_plan.h) on the host: reads
// "K L shared per half_a_only arrays rows out_limit" lines (out_limit 0: the default), prints
// "tile per all arrays lag_blocks slab out_bytes lds_bytes blocks" (tests/test_iccf_cpu.py).
#include "mtg_iccf_plan.h"

#include <stdio.h>

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int shared, per, half, arrays;
        long long K, L, rows, limit;
        if (sscanf(line, "%lld %lld %d %d %d %d %lld %lld", &K, &L, &shared, &per, &half, &arrays, &rows, &limit) != 8) return 1;
        const MtgIccfPlan p = limit ? mtg_iccf_plan(K, L, shared, per, half, arrays, limit) : mtg_iccf_plan(K, L, shared, per, half, arrays);
        printf("%d %d %d %d %lld %lld %lld %d %lld\n", p.tile, p.per, p.all, p.arrays, (long long)p.lag_blocks, (long long)p.slab,
               (long long)p.out_bytes, p.lds_bytes, (long long)mtg_iccf_blocks(p, rows));
    }
    return 0;
}
