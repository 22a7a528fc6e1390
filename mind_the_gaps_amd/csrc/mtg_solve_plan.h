// mtg_solve_plan.h -- which kernels solve a batch of prepared evaluations, decided from shapes alone: mtg_capi.hip's
// solve_prepared builds an MtgPlanIn, asks mtg_plan_solve and launches the plan.  Plain C++17 without HIP, so that the
// measured crossovers can be read in one place and run on the host (tests/solve_plan_driver.cpp).  The sampler's run plan
// and the rows per slab of mtg_predict_at and mtg_gp_draw are decided here in the same way.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mtg.h"

// ---------------------------------------------------------------------------------------------------------------
// The rank-10 time-parallel path's integer plan (mtg_tp_big.h; element and state layouts: mtg_tp_scan.h)
#define MTG_TPB_ELEM(J) (3 * (J) * (J) + 2 * (J))
#define MTG_TPB_STATE(J) ((J) * (J) + (J))
#define MTG_TPB_MAX_LEVELS 8

// Workspace of the big-J path, in doubles from a.tp_ws: element and state arrays per scan level,
// per-chunk partial sums of the final filter pass, per-evaluation head (sample 0).
#define MTG_TPB_TOP 4        /* elements per evaluation at the top level */
struct MtgTpBigPlan {
    int C;                         // chunks per evaluation (a power of two >= 64)
    int g;                         // elements per scan group (4 or 16), fewer where a level has less than 4 g
    int nlev;                      // scan levels; level 0 = the chunks, level nlev - 1 has MTG_TPB_TOP elements
    int n[MTG_TPB_MAX_LEVELS];     // elements per evaluation at each level
    int gl[MTG_TPB_MAX_LEVELS];    // group size that takes level l to level l + 1
    int64_t elem_off[MTG_TPB_MAX_LEVELS], state_off[MTG_TPB_MAX_LEVELS];
    int64_t rec_off[MTG_TPB_MAX_LEVELS];   // likelihood records of the levels >= 1 (level 0: the parts array)
    int64_t part_off, head_off, redo_off, total;
};

static inline MtgTpBigPlan mtg_tp_big_plan(int J, int64_t B, int C, int g)
{
    MtgTpBigPlan p;
    p.C = C;
    p.g = g;
    p.nlev = 0;
    int64_t off = 0;
    for (int n = C;;) {
        const int l = p.nlev++;
        p.n[l] = n;
        p.elem_off[l] = off; off += B * n * MTG_TPB_ELEM(J);
        p.state_off[l] = off; off += B * n * MTG_TPB_STATE(J);
        p.rec_off[l] = off; off += l > 0 ? B * n * 4 : 0;
        p.gl[l] = 0;
        if (n <= MTG_TPB_TOP || p.nlev == MTG_TPB_MAX_LEVELS) break;
        p.gl[l] = g < n / MTG_TPB_TOP ? g : n / MTG_TPB_TOP;   // (C is a power of two >= 64: ends on exactly four)
        n /= p.gl[l];
    }
    p.part_off = off; off += B * C * 4;
    p.head_off = off; off += B * 4;
    // evaluations sent back through the filter pass (mtg_tp_big.h): int list + counter
    p.redo_off = off; off += (B + 16) / 2 + 1;
    p.total = off;
    return p;
}

// chunks per evaluation: enough (chunk, evaluation) pairs to fill the GPU ONCE -- the composition kernel gives 64
// chunks to a workgroup of two waves, one per SIMD, two workgroups to a CU: 512 x 64 = 32 768 chunks in flight --, at
// least 64, at most 4096, and no chunk shorter than ~24 samples.  (Round 2 asked for 65 536: two rounds of
// workgroups with chunks half as long take the composition exactly as long, and leave the scan twice the elements.)
// target_knob: MTG_TP_CHUNK_TARGET of an MTG_MEASURE build, >= 64 replaces the target (the chunk count decides a
// result's bits); 0 otherwise.
static inline int mtg_tp_big_chunks(int64_t N, int64_t B, int64_t target_knob)
{
    // chunks over the whole batch: two waves per SIMD in the composition (32 768), one for the smallest batches, whose up-sweep
    // is then half as long (scripts/c5_chunk_target.sh, N = 2e5, ms per half-step at 32 768 / 16 384: 8 rows 0.311 / 0.265,
    // 16 rows 0.385 / 0.349, 32 rows 0.540 / 0.534, 64 rows 0.843 / 0.876, 256 rows 2.66 / 2.87)
    int64_t target = B <= 16 ? 16384 : 32768;
    if (target_knob >= 64) target = target_knob;
    int C = 64;
    while (C < 4096 && (int64_t)C * B < target && (int64_t)C * 2 * 24 <= N) C *= 2;
    return C;
}

// elements per scan group.  A group is one wave's chain of g - 1 dependent combinations (6.5 us each when the wave
// has a SIMD to itself, ~1 us of LDS traffic per CU when the GPU is full): the number of combinations of the whole
// scan is the number of elements whatever g is, so the short chains of g = 4 cost nothing but a launch per level
// (~5 us) and cut the depth from 15 to 3 combinations per level.
static inline int mtg_tp_big_gsize(int64_t B, int C)
{
    (void)B; (void)C;
    return 4;
}

// ---------------------------------------------------------------------------------------------------------------
// The solve plan

#define MTG_PIPE_ROWS_PER_CU 128   // the pipelined sweep (mtg_kernels_pipe.hip): one workgroup of 128 rows per CU
#define MTG_PLAN_MAX_SIG (MTG_MAX_J / 2 + 1)

// What the planner sees of a batch, its context and its model.
struct MtgPlanIn {
    int64_t N = 0, B = 0, L = 0;
    int64_t Bw = 0;                 // rows that do work: a walker-sharded half-step skips the other ranks' rows
    int nr0 = 0, nc0 = 0, nsig = 1, last_b0 = 0;     // the model's structures (MtgModel; nsig = SHO terms + 1)
    int tp_mode = 2, pipe_mode = 2, sort_mode = 2;  // mtg_set_time_parallel / mtg_set_pipeline / mtg_set_sort
    bool may_sort = false;          // the caller's order is arbitrary and comes with a light-curve index ...
    bool lc_grouped_hint = false;   // ... which the host saw grouped by light curve already
    bool no_prior_batch = false;    // the batch was expanded without the prior
    bool free_b = false;            // a term with a free b (ComplexTerm with four parameters, BendingPowerlaw)
    bool in_window = true;          // the resident set within one buffer descriptor's reach (yv_bytes <= window_bytes)
    int cus = 0;                    // compute units of the device
    bool profile_mean = false;      // the model's mean is a profile (MTG_MEAN_SINE, _TWOSINE, _GAUSSIAN): the one-lane sweep only
    // MTG_MEASURE knobs, read from the environment by the caller (shipped builds: these values)
    bool sweep_multi = true;        // MTG_SWEEP_MULTI=0: one launch per structure even where the one-launch kernel exists
    bool sweep_fan_out = true;      // MTG_SWEEP_FANOUT=0: the serial sweep's structures one after the other
    int tp_gsize = 0;               // MTG_TP_GSIZE: 4, 8 or 16 replaces the rank-10 scan group size
    int64_t tp_chunk_target = 0;    // MTG_TP_CHUNK_TARGET (mtg_tp_big_chunks)
};

// Which shapes have a compiled kernel (mtg_capi.hip asks the mtg_find_* tables of mtg_device.h).
struct MtgCatalogue {
    bool (*sweep)(int nr, int nc, int last_b0);
    int (*sweep_uses_b0)(int nr, int nc, int last_b0);   // mtg_solver_uses_b0
    bool (*tp)(int nr, int nc);
    bool (*tp_wide)(int nr, int nc);
    bool (*tp_fused)(int nr0, int nc0, int nsig, int lanes);
    bool (*pipe)(int nr0, int nc0, int nsig, int last_b0);
    bool (*multi)(int nr0, int nc0, int nsig, int last_b0);
};

enum MtgSolveFamily {
    MTG_SOLVE_TP_BIG,      // rank 10: every structure in one sequence of launches (mtg_tp_big.h)
    MTG_SOLVE_TP_FUSED,    // every structure in one time-parallel launch
    MTG_SOLVE_PIPE,        // the pipelined sweep, alone or in a launch shared with a paired context
    MTG_SOLVE_MULTI,       // every structure of the sorted order in one sweep launch (mtg_kernels_multi.hip)
    MTG_SOLVE_STRUCTURES,  // a launch per structure
};
enum MtgStructKernel { MTG_STRUCT_NONE, MTG_STRUCT_SWEEP, MTG_STRUCT_TP, MTG_STRUCT_TP_WIDE };

struct MtgSolvePlan {
    MtgSolveFamily family = MTG_SOLVE_STRUCTURES;
    bool sort = false;                  // sort the evaluations by (structure, light curve) first (mtg_sort.hip)
    bool fan_out = false;               // MTG_SOLVE_STRUCTURES: the structures k > 0 on side streams
    int fused_lanes = 0;                // MTG_SOLVE_TP_FUSED: 64, 128 or 256 lanes per evaluation
    int tp_chunks = 0, tp_gsize = 0;    // MTG_SOLVE_TP_BIG: chunks per evaluation, scan group size ...
    size_t tp_ws_bytes = 0;             // ... and workspace
    MtgStructKernel kernel[MTG_PLAN_MAX_SIG] = {};   // MTG_SOLVE_STRUCTURES: structure k's kernel (NONE: not launched)
    int side[MTG_PLAN_MAX_SIG] = {};    // ... and its stream: -1 the caller's, i >= 0 side stream i
    char name[96] = "";                 // what mtg_last_solver reports
};

// mtg_last_solver's text for the kernel of structure (nr, nc), `what` appended
static inline void mtg_struct_kernel_name(char *buf, size_t n, MtgStructKernel kind, int nr, int nc, int uses_b0,
                                          const char *what)
{
    if (kind == MTG_STRUCT_TP || kind == MTG_STRUCT_TP_WIDE)
        snprintf(buf, n, "mtg_tp_kernel<%d,%d,%d>%s", nr, nc, kind == MTG_STRUCT_TP ? 64 : 256, what);
    else if (nr + nc == 0) snprintf(buf, n, "mtg_white_kernel%s", what);
    else snprintf(buf, n, "mtg_solve_kernel<%d,%d,%d>%s", nr, nc, uses_b0, what);
}

// the same for the sweep with a profile mean (mtg_kernels_mean.hip)
static inline void mtg_mean_kernel_name(char *buf, size_t n, int nr, int nc, int uses_b0, const char *what)
{
    if (nr + nc == 0) snprintf(buf, n, "mtg_white_mean_kernel%s", what);
    else snprintf(buf, n, "mtg_solve_mean_kernel<%d,%d,%d>%s", nr, nc, uses_b0, what);
}

static inline MtgSolvePlan mtg_plan_solve(const MtgPlanIn &in, const MtgCatalogue &cat)
{
    MtgSolvePlan p;
    const int J = in.nr0 + 2 * in.nc0, nsig = in.nsig, b0 = in.last_b0 ? 1 : 0;
    // A small batch of long light curves leaves a one-lane-per-evaluation launch idle for N serial
    // steps: give every evaluation a whole wave (or four) instead (mtg_timeparallel.hip); the rank-10
    // structures get as many chunks per evaluation as fill the GPU (mtg_tp_big.h).
    // Measured crossovers: J <= 6 (one workgroup per evaluation) pays up to several thousand evaluations -- the serial
    // sweep runs one wave per 64 evaluations, latency bound, on a fraction of the SIMDs until ~10^5 of them; the J = 10
    // path costs ~3 x the serial sweep's work per sample, spread over every SIMD instead of B / 64 of
    // them, against ~1.05 us x N for the serial sweep whatever B <= 65 536 is.
    bool pays;
    // (scripts/crossover_probe.py, serial sweep / time-parallel in ms: N = 1e4, J = 5: 3.4 / 0.35 at 1024 evaluations,
    // 3.4 / 1.0 at 4096, 3.4 / 1.8 at 8192, equal at 16 384; N = 1e3, J = 5: 0.36 / 0.29 at 4096, 0.36 / 0.51 at 8192)
    // (round 4, against the pipelined sweep that now takes over beyond: scripts/pipe_probe.py, N = 1e4, time-parallel / pipeline
    // in ms: J = 3: 0.82 / 1.37 at 8192 rows, 1.20 / 1.39 at 12 288, 1.51 / 1.40 at 16 000; J = 5: 1.85 / 2.40 at 8192, 2.73 / 2.46 at 12 288)
    if (J <= 6) pays = in.N >= 256 && in.Bw <= (in.N >= 4096 ? (J <= 3 ? 12288 : 8192) : 4096);
    else pays = in.N >= 1024 && in.Bw <= 8192;
    // A term with a free b (ComplexTerm with four parameters, BendingPowerlaw) has a power spectrum that goes negative
    // where b d > a c -- which is exactly what those terms' own log_prior forbids, so a batch expanded WITH the prior never
    // solves such a row.  Without it (the optimiser's -lnL, gpmodelling.py:155-169) it may, and there the state-space form
    // the time-parallel kernels work in has an indefinite stationary covariance: their filter pass was found 1e-7 off on
    // such a row (tests/test_fuzz_gpu.py at MTG_FUZZ_OFFSET=112000, case 70; scripts/fuzz_case.py) where celerite's own
    // recursion -- the sweep -- is exact to rounding.  Those batches keep the sweep.
    const bool tp_allowed = !(in.free_b && in.no_prior_batch);
    bool small_ok = tp_allowed && (in.tp_mode == 1 || in.tp_mode == 3 || (in.tp_mode == 2 && pays));
    // mode 3 promises bits that do not depend on the batch; the rank-10 path sizes its chunks and scan groups by the
    // batch (mtg_tp_big_chunks), so under mode 3 such a model keeps the serial sweep
    if (in.tp_mode == 3 && J > 6) small_ok = false;
    if (J == 0) small_ok = false;  // a white kernel: nothing to parallelise over time (mtg_white_kernel)
    // A profile mean is known to the one-lane sweep of mtg_kernels_mean.hip alone: a launch per structure whatever
    // tp_mode and pipe_mode say -- no time-parallel kernel, no pipeline (hence no pairing), no multi launch -- so that
    // a row's bits never depend on the batch; sorting, the window logic and the fan-out work as for the plain sweep.
    if (in.profile_mean) small_ok = false;
    if (small_ok && J > 6) {
        for (int k = 0; k < nsig; ++k)
            if (!cat.tp(in.nr0 + 2 * k, in.nc0 - k)) small_ok = false;
        const int C = mtg_tp_big_chunks(in.N, in.Bw, in.tp_chunk_target);
        int g = mtg_tp_big_gsize(in.Bw, C);
        if (in.tp_gsize == 4 || in.tp_gsize == 8 || in.tp_gsize == 16) g = in.tp_gsize;
        const size_t need = (size_t)mtg_tp_big_plan(J, in.B, C, g).total * sizeof(double);
        if (in.B > 65535 || need > ((size_t)16 << 30)) small_ok = false;  // grid / workspace limits: the serial sweep
        if (small_ok) {
            p.family = MTG_SOLVE_TP_BIG;
            p.tp_chunks = C;
            p.tp_gsize = g;
            p.tp_ws_bytes = need;
            snprintf(p.name, sizeof p.name, "mtg_tpb_compose4q_kernel (+ mtg_tpb_reduce_kernel<10>, C = %d)", C);
            return p;
        }
    }
    // four waves per evaluation: while every evaluation's workgroup is resident at once (rank <= 3: two per CU, their
    // elements take 68 KB of LDS; above: one)
    // (scripts/spec_probe.py, J = 3, N = 1e4: 384 rows 70.9 us against 96.0 us with one wave each, 512 rows 77.4 / 97.2)
    // (mode 3: the one-wave kernel whatever the batch, so that a row's bits do not depend on how many rows travel with it)
    const bool wide = in.tp_mode != 3 && in.Bw <= (J <= 3 ? 512 : 256) && in.N >= 4096;
    // two waves per evaluation between 257 and 512 rows of rank 4 or 5: half a CU's LDS each, all resident at once
    // (scripts/spec_probe.py, J = 5, N = 1e4, 384 rows: see DESIGN.md)
    const bool mid = in.tp_mode != 3 && !wide && in.Bw <= 512 && in.N >= 4096 && (J == 4 || J == 5);
    if (small_ok && nsig > 1) {  // every signature in one launch: the widest form that applies and is compiled
        const int widest_first[3] = {wide ? 256 : 0, mid ? 128 : 0, 64};
        for (const int lanes : widest_first) {
            if (!lanes || !cat.tp_fused(in.nr0, in.nc0, nsig, lanes)) continue;
            p.family = MTG_SOLVE_TP_FUSED;
            p.fused_lanes = lanes;
            snprintf(p.name, sizeof p.name, "mtg_tp_fused_kernel<%d,%d,%d,%d>", in.nr0, in.nc0, nsig, lanes);
            return p;
        }
    }
    // Between the time-parallel kernels' range and ~one wave per SIMD the serial sweep is one lone wave per 64 rows on
    // a fraction of the SIMDs, N dependent steps of ~166 instructions: the pipelined form puts the generators of those
    // rows on a second wave (mtg_kernels_pipe.hip) -- one workgroup of 128 rows per CU, all resident at once.
    const bool pipe = !small_ok && !in.profile_mean && in.pipe_mode != 0 && in.N >= 64 && in.in_window &&
                      (in.pipe_mode == 1 || (in.N >= 256 && in.B <= (int64_t)MTG_PIPE_ROWS_PER_CU * in.cus)) &&
                      cat.pipe(in.nr0, in.nc0, nsig, in.last_b0);
    // The serial sweep reads each lane's own light curve: sort the evaluations by (structure, light curve) unless the
    // caller's order is known to be grouped (mtg_sort.hip).  One light curve, or no index at all: nothing to sort.
    // More than one structure: the per-structure lists are appended to with one atomic per wave, so their order -- which
    // rows share a wave -- changes from run to run, and a row's last bits may depend on its wave (a lane with a huge
    // d dx sends the whole wave through the libm sincos).  A seeded chain has to be reproducible: the stable sort gives
    // the lanes of every structure the caller's order, whatever the arrival order of the waves was.
    const bool for_order = in.may_sort && in.L > 1 && (in.sort_mode == 1 || (in.sort_mode == 2 && !in.lc_grouped_hint));
    const bool for_determinism = nsig > 1 && in.sort_mode != 0;
    p.sort = (for_order || for_determinism) && !small_ok && in.B > 64 && (uint64_t)in.L * (uint64_t)nsig < 0x7fffffffull;
    if (pipe && (nsig == 1 || p.sort)) {
        p.family = MTG_SOLVE_PIPE;   // (a launch shared with the partner is named by mtg_plan_name_paired)
        snprintf(p.name, sizeof p.name, "mtg_pipe_kernel<%d,%d,%d,%d>", in.nr0, in.nc0, nsig, b0);
        return p;
    }
    if (p.sort && nsig > 1 && !in.profile_mean && in.in_window && in.sweep_multi && cat.multi(in.nr0, in.nc0, nsig, in.last_b0)) {
        p.family = MTG_SOLVE_MULTI;
        snprintf(p.name, sizeof p.name, "mtg_solve_kernel_multi<%d,%d,%d,%d>", in.nr0, in.nc0, nsig, b0);
        return p;
    }
    // A time-parallel launch is latency bound: a structure holding three evaluations takes as long
    // as one holding 250 (J = 10: ~10 ms each), and one after the other on the same stream they
    // add up.  The structures work on disjoint evaluations, so each gets its own stream: forked
    // after the expansion, joined before whatever follows on `s`.
    // The serial sweep is latency bound in the same way -- N dependent steps, ~0.4 us each, whatever the number of
    // rows -- and a sampler's half-step of 256 000 walkers with a handful of them over-damped paid 14.9 ms for
    // the first structure and 3.2-4.3 ms more for those few (profiles/r03_c3_halfstep_trace.txt).  On their own
    // stream they take wave slots as the big launch frees them and finish under it.
    p.fan_out = (small_ok || in.sweep_fan_out) && nsig > 1 && nsig - 1 <= MTG_MAX_J / 2;
    for (int k = 0; k < nsig; ++k) {
        const int nr = in.nr0 + 2 * k, nc = in.nc0 - k;
        p.side[k] = p.fan_out && k > 0 ? k - 1 : -1;
        if (!cat.sweep(nr, nc, in.last_b0)) continue;   // not launched, not joined
        if (!small_ok || !cat.tp(nr, nc)) p.kernel[k] = MTG_STRUCT_SWEEP;
        else p.kernel[k] = wide && cat.tp_wide(nr, nc) ? MTG_STRUCT_TP_WIDE : MTG_STRUCT_TP;
        if (k == 0 && in.profile_mean) mtg_mean_kernel_name(p.name, sizeof p.name, nr, nc, cat.sweep_uses_b0(nr, nc, in.last_b0), "");
        else if (k == 0) mtg_struct_kernel_name(p.name, sizeof p.name, p.kernel[0], nr, nc, cat.sweep_uses_b0(nr, nc, in.last_b0), "");
    }
    return p;
}

// the pipelined family's name once pair_launch put the rows into a launch shared with the partner context's
static inline void mtg_plan_name_paired(MtgSolvePlan &p, const MtgPlanIn &in)
{
    snprintf(p.name, sizeof p.name, "mtg_pipe_pair_kernel (this model: <%d,%d,%d,%d>)", in.nr0, in.nc0, in.nsig, in.last_b0 ? 1 : 0);
}

// mtg_ensemble_run: both half-steps of an iteration in one batch of rows3 = 3 E W / 2 rows?  A small ensemble leaves
// most of the GPU idle and its solve takes as long for 3 H rows as for H (mtg_sampler.hip: speculative iteration).
// Where: the time-parallel kernels with every row on a workgroup of its own in one occupancy round -- 256 workgroups
// of four waves for long light curves (one per CU: their elements fill the LDS; two per CU up to rank 3, and for ranks
// 4 and 5 with two waves each), 1024 single-wave ones for short.  Same chain either way where both forms run the same
// kernel.
static inline bool mtg_plan_speculate(int tp_mode, int Jmodel, int64_t N, int64_t rows3)
{
    return tp_mode != 0 && Jmodel <= 6 && N >= 256 && rows3 <= (N >= 4096 ? (Jmodel <= 5 ? 512 : 256) : 1024);
}

// ---------------------------------------------------------------------------------------------------------------
// Rows per slab of the host-pointer entries that keep a whole row of device memory per evaluation (mtg_capi.hip)

// device workspace of one slab of mtg_predict_at: rows whose stored generators (3 J + 3 doubles per sample) stay below this
#define MTG_PAT_SLAB_BYTES ((size_t)1 << 30)
// device memory of one slab of mtg_gp_draw: rows (a multiple of 64) whose draws stay below this, and as much again for
// the caller's normals
#define MTG_DRAW_SLAB_BYTES ((size_t)1 << 28)

// mtg_predict_at: the stored generators within MTG_PAT_SLAB_BYTES, and the grid of the second stage -- rows x
// ceil(M / 64) blocks -- within 2^30 blocks; at least one row, at most B.  0: M alone has more than 2^30 blocks
// more_row_bytes: what a caller keeps per row of the slab beside the generators (mtg_gp_cond_draw: its normals, y - y~,
// f*, mu and the draws, which grow with M), counted within the same budget
static inline int64_t mtg_plan_predict_at_slab(int64_t N, int J, int64_t M, int64_t B, size_t more_row_bytes = 0)
{
    const size_t row_bytes = (size_t)N * (3 * J + 3) * 8 + more_row_bytes;
    int64_t Bs = (int64_t)(MTG_PAT_SLAB_BYTES / row_bytes);
    const int64_t mblocks = (M + 63) / 64;
    if (mblocks > ((int64_t)1 << 30)) return 0;
    if (Bs > ((int64_t)1 << 30) / mblocks) Bs = ((int64_t)1 << 30) / mblocks;
    if (Bs < 1) Bs = 1;
    if (Bs > B) Bs = B;
    return Bs;
}

// mtg_gp_draw: a multiple of 64 rows (a workgroup's tile) within MTG_DRAW_SLAB_BYTES, at least 64; or all B rows
static inline int64_t mtg_plan_draw_slab(int64_t N, int64_t B)
{
    int64_t Bs = (int64_t)(MTG_DRAW_SLAB_BYTES / ((size_t)N * 8)) / 64 * 64;
    if (Bs < 64) Bs = 64;
    if (Bs > B) Bs = B;
    return Bs;
}

// mtg_whiten: as mtg_plan_draw_slab -- whole workgroups of 64 rows whose residuals [rows][N] stay within `budget` bytes,
// at least 64, or all B rows -- and at most 65472 rows, the y extent of the autocorrelation's grid in whole workgroups.
// The budget is MTG_DRAW_SLAB_BYTES or the context's window (mtg_set_window_bytes), whichever is smaller: one slab of
// residuals stays within the reach of one buffer descriptor, as a resident light curve does.  sorted: the rows are sorted
// for the KS distances, and the segmented sort counts a slab's items in 32 bits: then rows N < 2^31 comes first, down to
// one row (a slab need not be whole workgroups: a row does not depend on its neighbours).
#define MTG_WHITEN_SLAB_MAX_ROWS 65472
// slab buffers above this are given back at the end of a call (mtg_capi.hip)
#define MTG_WHITEN_KEEP_BYTES ((size_t)64 << 20)
static inline int64_t mtg_plan_whiten_slab(int64_t N, int64_t B, uint64_t window_bytes, bool sorted = false)
{
    const uint64_t budget = window_bytes < (uint64_t)MTG_DRAW_SLAB_BYTES ? window_bytes : (uint64_t)MTG_DRAW_SLAB_BYTES;
    int64_t Bs = (int64_t)(budget / ((uint64_t)N * 8)) / 64 * 64;
    if (Bs < 64) Bs = 64;
    if (Bs > MTG_WHITEN_SLAB_MAX_ROWS) Bs = MTG_WHITEN_SLAB_MAX_ROWS;
    if (sorted && Bs > (int64_t)0x7fffffff / N) Bs = (int64_t)0x7fffffff / N;
    if (Bs < 1) Bs = 1;
    if (Bs > B) Bs = B;
    return Bs;
}

// ---------------------------------------------------------------------------------------------------------------
// The run plan of the device-resident sampler (mtg_capi.hip: mtg_ensemble_run)

// The red/blue splits of a whole speculative run are made by ONE launch before it (mtg_launch_split_all) while they are
// small: the sampler kernel of an iteration is one workgroup's chain of latencies and ranking W keys is 2-5 us of it.
#define MTG_SPLITS_MAX_BYTES ((size_t)64 << 20)   // [steps][E][W] int32
#define MTG_SPLITS_MAX_STEPS 65535                // the launch's grid: one row of workgroups per step

struct MtgEnsembleRunPlan {
    bool speculative = false;       // both half-steps of an iteration in one solve (where: mtg_plan_speculate)
    bool splits_up_front = false;   // speculative: every split of the run made before it, perm_bytes of them
    int64_t rows_per_solve = 0;     // E W/2 for a half-step, 3 E W/2 for a speculative iteration
    int64_t solves = 0;             // 2 steps half-steps, or steps iterations
    int64_t live_rows = 0;          // rows of a solve this rank evaluates, for the solver's kernel choice (0: all)
    size_t perm_bytes = 0;
};

// spec_mode: mtg_set_speculation (0 never, 1 where it pays, 2 = 1 with the splits inside the sampler's launches);
// shard_kind != 0: every half-step's rows [shard_lo, shard_hi) only (an empty share still counts as one live row:
// 0 means all).  Walker-sharded runs do not speculate.
static inline MtgEnsembleRunPlan mtg_plan_ensemble_run(int64_t E, int W, int64_t steps, int tp_mode, int spec_mode, int Jmodel,
                                                       int64_t N, int shard_kind, int64_t shard_lo, int64_t shard_hi)
{
    MtgEnsembleRunPlan p;
    const int64_t EH = E * (W / 2);
    const bool sharded = shard_kind != 0;
    p.speculative = steps > 0 && spec_mode != 0 && !sharded && mtg_plan_speculate(tp_mode, Jmodel, N, 3 * EH);
    p.rows_per_solve = p.speculative ? 3 * EH : EH;
    p.solves = p.speculative ? steps : 2 * steps;
    p.live_rows = sharded ? (shard_hi > shard_lo ? shard_hi - shard_lo : 1) : 0;
    if (p.speculative) {
        const size_t bytes = (size_t)steps * (size_t)(E * W) * sizeof(int32_t);
        p.splits_up_front = bytes <= MTG_SPLITS_MAX_BYTES && steps <= MTG_SPLITS_MAX_STEPS && spec_mode != 2;
        if (p.splits_up_front) p.perm_bytes = bytes;
    }
    return p;
}

// What the sampler launch after solve k of a run does (k = -1: the priming launch before the first solve).  Solve k
// reads the structure lists of bank k & 1; the launch accepts (iteration, half), clears that bank's counters and
// proposes (next_iteration, next_half) into the other bank.  A speculative solve is a whole iteration: half = 0.
struct MtgEnsembleStep {
    int bank_used = -1, bank_next = 0;   // -1: no solve came before, nothing to accept or clear
    int do_accept = 0, half = 0;
    uint32_t iteration = 0;
    int do_propose = 1, next_half = 0;
    uint32_t next_iteration = 0;
    int64_t chain_row = -1;              // the step of this run whose chain row the launch writes; -1: none
    // slices [E][W] of the up-front splits: the accepted iteration's and the proposed one's (-1: the split made inside
    // the launch, in the ensembles' own buffer)
    int64_t perm = -1, perm_next = -1;
};

static inline MtgEnsembleStep mtg_ensemble_step(const MtgEnsembleRunPlan &plan, int64_t k, int64_t steps, uint32_t iteration0)
{
    MtgEnsembleStep st;
    st.next_iteration = iteration0;
    if (k >= 0) {
        const int per = plan.speculative ? 1 : 2;   // solves per iteration
        const int64_t it = k / per;
        const bool closes = k % per == per - 1;      // the iteration is complete after this accept
        st.bank_used = (int)(k & 1);
        st.bank_next = st.bank_used ^ 1;
        st.do_accept = 1;
        st.half = (int)(k % per);
        st.iteration = iteration0 + (uint32_t)it;
        st.do_propose = k + 1 < plan.solves ? 1 : 0;
        st.next_half = closes ? 0 : 1;
        st.next_iteration = closes ? st.iteration + 1 : st.iteration;
        st.chain_row = closes ? it : -1;
    }
    if (plan.splits_up_front) {
        st.perm = k;   // (one solve per iteration)
        st.perm_next = k + 1 < steps ? k + 1 : -1;
    }
    return st;
}
