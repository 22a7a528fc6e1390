// Runs the solve planner (mind_the_gaps_amd/csrc/mtg_solve_plan.h) over a small grid of (N, B, structures, tp_mode,
// pipe_mode) for tests/test_mean_profile_cpu.py: one line per point with MtgPlanIn::profile_mean clear -- which must be
// the plan the header gave before the field existed (tests/golden/mean_plan_parent.txt, written by this program
// compiled with -DMTG_PLAN_PARENT against that header) -- and one with it set.  The catalogue is the library's ranges.
#include "mtg_solve_plan.h"

#include <iostream>

namespace {

bool sweep(int nr, int nc, int) { return nr + 2 * nc <= MTG_MAX_J; }
int uses_b0(int nr, int nc, int b0) { return b0 && nc > 0 && nr < 5 && nc < 4 && nr + 2 * nc <= 6; }
bool tp(int nr, int nc) { return (nr + nc > 0 && nr + 2 * nc <= 6) || (nr + 2 * nc == 10 && nr % 2 == 0); }
bool tp_wide(int nr, int nc) { return nr + nc > 0 && nr + 2 * nc <= 5; }
bool tp_fused(int, int nc0, int, int) { return nc0 >= 1 && nc0 <= 3; }
bool pipe(int nr0, int nc0, int nsig, int) { return nr0 <= 4 && nc0 >= 1 && nc0 <= 3 && nsig <= 3; }
bool multi(int nr0, int nc0, int nsig, int) { return nr0 <= 4 && nc0 >= 1 && nc0 <= 3 && nsig >= 2 && nsig <= 3; }
const MtgCatalogue g_cat = {sweep, uses_b0, tp, tp_wide, tp_fused, pipe, multi};
const char *const g_family[] = {"tp_big", "tp_fused", "pipe", "multi", "structures"};
const char *const g_kernel[] = {"none", "sweep", "tp", "tp_wide"};

void show(const char *tag, const MtgPlanIn &in)
{
    const MtgSolvePlan p = mtg_plan_solve(in, g_cat);
    std::cout << tag << " N=" << in.N << " B=" << in.B << " nr0=" << in.nr0 << " nc0=" << in.nc0 << " nsig=" << in.nsig << " b0="
              << in.last_b0 << " tp=" << in.tp_mode << " pipe=" << in.pipe_mode << " : family=" << g_family[p.family]
              << " sort=" << p.sort << " fan_out=" << p.fan_out << " C=" << p.tp_chunks << " lanes=" << p.fused_lanes << " kernels=";
    for (int k = 0; k < in.nsig; ++k) std::cout << (k ? "," : "") << g_kernel[p.kernel[k]] << ":" << p.side[k];
    std::cout << " name=" << p.name << "\n";
}

}  // namespace

int main()
{
    const int shapes[][4] = {{0, 0, 1, 0}, {1, 0, 1, 0}, {0, 1, 2, 0}, {1, 2, 2, 1}, {2, 2, 1, 0}, {0, 5, 6, 0}};   // nr0, nc0, nsig, b0
    for (const auto &sh : shapes)
        for (const int64_t N : {65, 4097})
            for (const int64_t B : {1, 67, 5000, 100000})
                for (int tp = 0; tp <= 3; ++tp)
                    for (int pm = 0; pm <= 2; ++pm) {
                        MtgPlanIn in;
                        in.N = N; in.B = in.Bw = B; in.L = 2;
                        in.nr0 = sh[0]; in.nc0 = sh[1]; in.nsig = sh[2]; in.last_b0 = sh[3];
                        in.tp_mode = tp; in.pipe_mode = pm; in.may_sort = true; in.cus = 256;
                        show("plain", in);
#ifndef MTG_PLAN_PARENT
                        in.profile_mean = true;
                        show("profile", in);
#endif
                    }
    return 0;
}
