// Runs the solve planner (mind_the_gaps_amd/csrc/mtg_solve_plan.h) on the host for tests/test_solve_plan_cpu.py: one
// case per line of standard input as key=value tokens, one line of the plan's decisions per case.  The catalogue is a
// stub with the compiled ranges of the library; `no=<shape>` takes one kind of kernel out of it.  `run=1` asks for the
// sampler's run plan instead, `sched=1` for that plan's whole schedule, from the priming launch to the last solve,
// `slab=1` for the rows per slab of mtg_predict_at (N, the rank nr0 + 2 nc0, M, B) and of mtg_gp_draw (N, B).
#include "mtg_solve_plan.h"

#include <iostream>
#include <sstream>
#include <string>

namespace {

std::string g_missing;   // the kernels a case takes out of the catalogue
bool missing(const char *what) { return g_missing.find(what) != std::string::npos; }

bool sweep(int nr, int nc, int) { return nr + 2 * nc <= MTG_MAX_J && !(missing("sweep1") && nc == 1); }
int uses_b0(int nr, int nc, int b0) { return b0 && nc > 0 && nr < 5 && nc < 4 && nr + 2 * nc <= 6; }
bool tp(int nr, int nc) { return !missing("tp") && ((nr + nc > 0 && nr + 2 * nc <= 6) || (nr + 2 * nc == 10 && nr % 2 == 0)); }
bool tp_wide(int nr, int nc) { return !missing("wide") && nr + nc > 0 && nr + 2 * nc <= 5; }
bool tp_fused(int, int nc0, int, int lanes) { return nc0 >= 1 && nc0 <= 3 && !missing(("fused" + std::to_string(lanes)).c_str()); }
bool pipe(int nr0, int nc0, int nsig, int) { return !missing("pipe") && nr0 <= 4 && nc0 >= 1 && nc0 <= 3 && nsig <= 3; }
bool multi(int nr0, int nc0, int nsig, int) { return !missing("multi") && nr0 <= 4 && nc0 >= 1 && nc0 <= 3 && nsig >= 2 && nsig <= 3; }
const MtgCatalogue g_cat = {sweep, uses_b0, tp, tp_wide, tp_fused, pipe, multi};

const char *const g_family[] = {"tp_big", "tp_fused", "pipe", "multi", "structures"};
const char *const g_kernel[] = {"none", "sweep", "tp", "tp_wide"};

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        MtgPlanIn in;
        bool spec = false, run = false, sched = false, slab = false;
        long long E = 1, W = 8, steps = 3, spec_mode = 1, shard = 0, lo = 0, hi = 0, iter0 = 0, M = 1;
        g_missing.clear();
        std::istringstream tokens(line);
        std::string tok;
        while (tokens >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "no") { g_missing = v; continue; }
            const long long x = std::stoll(v);
            if (k == "N") in.N = x;
            else if (k == "B") in.B = x;
            else if (k == "Bw") in.Bw = x;
            else if (k == "L") in.L = x;
            else if (k == "nr0") in.nr0 = (int)x;
            else if (k == "nc0") in.nc0 = (int)x;
            else if (k == "nsig") in.nsig = (int)x;
            else if (k == "b0") in.last_b0 = (int)x;
            else if (k == "tp") in.tp_mode = (int)x;
            else if (k == "pipe") in.pipe_mode = (int)x;
            else if (k == "sort") in.sort_mode = (int)x;
            else if (k == "may_sort") in.may_sort = x != 0;
            else if (k == "grouped") in.lc_grouped_hint = x != 0;
            else if (k == "no_prior") in.no_prior_batch = x != 0;
            else if (k == "free_b") in.free_b = x != 0;
            else if (k == "in_window") in.in_window = x != 0;
            else if (k == "cus") in.cus = (int)x;
            else if (k == "multi_knob") in.sweep_multi = x != 0;
            else if (k == "fan_out_knob") in.sweep_fan_out = x != 0;
            else if (k == "gsize") in.tp_gsize = (int)x;
            else if (k == "chunk_target") in.tp_chunk_target = x;
            else if (k == "spec") spec = x != 0;
            else if (k == "run") run = x != 0;
            else if (k == "sched") sched = x != 0;
            else if (k == "slab") slab = x != 0;
            else if (k == "M") M = x;
            else if (k == "E") E = x;
            else if (k == "W") W = x;
            else if (k == "steps") steps = x;
            else if (k == "spec_mode") spec_mode = x;
            else if (k == "shard") shard = x;
            else if (k == "lo") lo = x;
            else if (k == "hi") hi = x;
            else if (k == "iter0") iter0 = x;
            else { std::cerr << "unknown key " << k << "\n"; return 2; }
        }
        if (in.Bw == 0) in.Bw = in.B;
        if (spec) {
            std::cout << "spec=" << mtg_plan_speculate(in.tp_mode, in.nr0 + 2 * in.nc0, in.N, in.B) << "\n";
            continue;
        }
        if (slab) {
            std::cout << "predict_at=" << mtg_plan_predict_at_slab(in.N, in.nr0 + 2 * in.nc0, M, in.B)
                      << " draw=" << mtg_plan_draw_slab(in.N, in.B) << "\n";
            continue;
        }
        if (run || sched) {
            const MtgEnsembleRunPlan r = mtg_plan_ensemble_run(E, (int)W, steps, in.tp_mode, (int)spec_mode, in.nr0 + 2 * in.nc0, in.N,
                                                               (int)shard, lo, hi);
            if (run)
                std::cout << "speculative=" << r.speculative << " up_front=" << r.splits_up_front << " rows=" << r.rows_per_solve
                          << " solves=" << r.solves << " live=" << r.live_rows << " perm_bytes=" << r.perm_bytes;
            for (int64_t k = -1; sched && r.solves > 0 && k < r.solves; ++k) {   // (no solve: no priming launch either)
                const MtgEnsembleStep st = mtg_ensemble_step(r, k, steps, (uint32_t)iter0);
                std::cout << (k >= 0 ? " | " : "") << k << " " << st.bank_used << " " << st.bank_next << " " << st.do_accept << " "
                          << st.half << " " << st.iteration << " " << st.do_propose << " " << st.next_half << " "
                          << st.next_iteration << " " << st.chain_row << " " << st.perm << " " << st.perm_next;
            }
            std::cout << "\n";
            continue;
        }
        const MtgSolvePlan p = mtg_plan_solve(in, g_cat);
        std::cout << "family=" << g_family[p.family] << " sort=" << p.sort << " fan_out=" << p.fan_out << " C=" << p.tp_chunks
                  << " g=" << p.tp_gsize << " lanes=" << p.fused_lanes << " kernels=";
        for (int k = 0; k < in.nsig; ++k) std::cout << (k ? "," : "") << g_kernel[p.kernel[k]] << ":" << p.side[k];
        std::cout << " name=" << p.name << "\n";
    }
    return 0;
}
