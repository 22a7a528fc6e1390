// mtg_kernels_mean.hip -- the one-lane-per-evaluation sweep of mtg_kernels.hip with a profile mean (MTG_MEAN_SINE,
// MTG_MEAN_TWOSINE, MTG_MEAN_GAUSSIAN) subtracted inside the step: mtg_sweep itself, instantiated with a `Mean` type of
// mtg_sweep_mean.h, for every structure (NR, NC, NB0) mtg_kernels.hip compiles, and the white kernel's form of it.
// Compiled once per mean kind (-DMTG_MEAN_UNIT=<kind>: one object each, so that the three build side by side);
// the object of MTG_MEAN_SINE also holds mtg_find_mean_solver, which picks among the three tables.
//
// These are the only kernels that know the profile means: the planner (mtg_solve_plan.h) sends a model that has one
// to the per-structure sweep whatever the batch is, so a row's bits do not depend on what travels with it.
#include "mtg_device.h"
#include "mtg_sweep_mean.h"

#ifndef MTG_MEAN_UNIT
#error "compile with -DMTG_MEAN_UNIT=<MTG_MEAN_SINE | MTG_MEAN_TWOSINE | MTG_MEAN_GAUSSIAN>"
#endif

typedef MtgMeanProfile<MTG_MEAN_UNIT> MtgUnitMean;

// The per-lane constants of the mean (nconst doubles) come on top of the recurrence's state.  The lowest ranks give up
// one wave of the five mtg_waves_for asks for (their tables cap a CU at three workgroups -- three waves per SIMD --
// anyway).  At rank 6 the 256 registers of two waves per SIMD are the limit: three complex terms alone take 238 of
// them without a profile mean, and the two sines' six constants push structures with a complex term over it.  Those
// get one wave's 512 registers; which instantiations spilled at two waves, and what every one takes now, is in
// profiles/mean_probe.txt.
__host__ __device__ constexpr int mtg_mean_waves_for(int NR, int NC, int nconst)
{
    return NR + 2 * NC <= 2 ? 4 : NR + 2 * NC == 6 && (NC == 3 || (NC > 0 && nconst >= 6)) ? 1 : mtg_waves_for(NR + 2 * NC);
}

// Which row is whose, as in mtg_solve_kernel / mtg_white_kernel (mtg_kernels.hip, whose code is not touched): rows,
// lists, the solo launch of the left-overs (one evaluation per wave, on lane 0) and the prior's verdict.
__device__ __forceinline__ bool mtg_mean_block_idle(const MtgSolveArgs &a)
{
    const int64_t count = a.count_ptr ? (int64_t)*a.count_ptr : a.B;
    return (int64_t)blockIdx.x * (a.solo ? MTG_BLOCK / 64 : MTG_BLOCK) >= count;   // e.g. an empty signature list
}
__device__ __forceinline__ bool mtg_mean_lane_row(const MtgSolveArgs &a, int64_t *row)
{
    const int64_t count = a.count_ptr ? (int64_t)*a.count_ptr : a.B;
    const int per_block = a.solo ? MTG_BLOCK / 64 : MTG_BLOCK;
    if (a.solo && (threadIdx.x & 63) != 0) return false;
    const int64_t gid = (int64_t)blockIdx.x * per_block + (a.solo ? threadIdx.x >> 6 : threadIdx.x);
    if (gid >= count) return false;
    int64_t first = 0;  // sorted order: this structure's segment of the sorted batch
    if (a.seg_counts)
        for (int i = 0; i < a.seg_k; ++i) first += a.seg_counts[i];
    const int64_t e = a.list ? (int64_t)a.list[first + gid] : gid;
    *row = e;
    return a.status[e] == MTG_ST_OK;  // else the prior's verdict stands
}

// (Mean is a template parameter of the kernels so that the three objects' kernels are three sets of symbols)
template <int NR, int NC, int NB0, class Mean>
__global__ void __launch_bounds__(MTG_BLOCK, mtg_mean_waves_for(NR, NC, Mean::nconst)) mtg_solve_mean_kernel(MtgSolveArgs a)
{
    if (mtg_mean_block_idle(a)) return;
    __shared__ MtgMathTablesT<(NC > 0 || Mean::trig)> tab;
    mtg_fill_tables(&tab, threadIdx.x, MTG_BLOCK);
    __syncthreads();
    int64_t e;
    if (!mtg_mean_lane_row(a, &e)) return;
    mtg_solve_row<NR, NC, NB0, MtgMathTablesT<(NC > 0 || Mean::trig)>, Mean>(a, e, &tab);
}

namespace {

template <int NR, int NC, int NB0 = 0>
void mtg_launch_solve_mean(const MtgSolveArgs &a, int64_t nlanes, hipStream_t stream)
{
    const int64_t blocks = (nlanes + MTG_BLOCK - 1) / MTG_BLOCK;
    if (blocks <= 0) return;
    hipLaunchKernelGGL((mtg_solve_mean_kernel<NR, NC, NB0, MtgUnitMean>), dim3((unsigned)blocks), dim3(MTG_BLOCK), 0, stream, a);
}

}  // namespace

// A white kernel (JitterTerm alone) under a profile mean: mtg_white_kernel's rows, lists and verdicts, the mean from the
// same `Mean` type as the sweep's.
template <class Mean>
__global__ void __launch_bounds__(MTG_BLOCK) mtg_white_mean_kernel(MtgSolveArgs a)
{
    if (mtg_mean_block_idle(a)) return;
    __shared__ MtgMathTablesT<Mean::trig> tab;
    mtg_fill_tables(&tab, threadIdx.x, MTG_BLOCK);
    __syncthreads();
    int64_t e;
    if (!mtg_mean_lane_row(a, &e)) return;
    const double *cf = a.coef + e;
    const double jit = cf[a.lay.jit() * a.cstride];
    Mean mean;
    mean.load(a, cf, a.cstride);
    const uint64_t lc = a.lc_index ? (uint64_t)(uint32_t)a.lc_index[e] : 0u;
    if ((lc + 1u) * (uint64_t)a.N * 16u > a.yv_bytes) {  // a device-side lc_index outside the resident set
        a.out[e] = -INFINITY;
        a.status[e] = MTG_ST_NONFINITE;
        return;
    }
    const double2 *yv = a.yv + lc * (uint64_t)a.N;
    const double2 *dxt = a.dxt + (a.t_stride ? lc * (uint64_t)a.N : 0u);
    double dot = 0.0, dprod = 1.0;
    int dexp = 0, dmin_hi = 0x7fffffff;
    for (int64_t n = 0; n < a.N; ++n) {
        const double2 s = yv[n];
        const double D = s.y + jit, z = s.x - mean.value(dxt[n].y, &tab);
        dmin_hi = min(dmin_hi, __double2hiint(D));
        dot = fma(z, z / D, dot);
        dprod *= D;
        dexp += __builtin_amdgcn_frexp_exp(dprod);
        dprod = __builtin_amdgcn_frexp_mant(dprod);
    }
    double ll;
    int st;
    mtg_finish_lnl(a.N, dot, dprod, dexp, dmin_hi, &ll, &st);
    a.out[e] = ll;
    a.status[e] = st;
}

namespace {

void mtg_launch_white_mean(const MtgSolveArgs &a, int64_t nlanes, hipStream_t stream)
{
    const int64_t blocks = (nlanes + MTG_BLOCK - 1) / MTG_BLOCK;
    if (blocks <= 0) return;
    hipLaunchKernelGGL(mtg_white_mean_kernel<MtgUnitMean>, dim3((unsigned)blocks), dim3(MTG_BLOCK), 0, stream, a);
}

// The structures of mtg_kernels.hip's tables: NR real + NC complex terms, J = NR + 2 NC <= MTG_MAX_J ...
#define MTG_MAX_NR 10
#define MTG_MAX_NC 5
template <int NR, int NC, bool OK = (NR + NC > 0 && NR + 2 * NC <= MTG_MAX_J)>
struct MtgMeanSel { static constexpr mtg_solve_launcher fn = mtg_launch_solve_mean<NR, NC>; };
template <int NR, int NC>
struct MtgMeanSel<NR, NC, false> { static constexpr mtg_solve_launcher fn = nullptr; };
#define MTG_MEAN_ROW(nr)                                                                                  \
    { MtgMeanSel<(nr), 0>::fn, MtgMeanSel<(nr), 1>::fn, MtgMeanSel<(nr), 2>::fn, MtgMeanSel<(nr), 3>::fn, \
      MtgMeanSel<(nr), 4>::fn, MtgMeanSel<(nr), 5>::fn }
const mtg_solve_launcher mtg_mean_solver_table[MTG_MAX_NR + 1][MTG_MAX_NC + 1] = {
    MTG_MEAN_ROW(0), MTG_MEAN_ROW(1), MTG_MEAN_ROW(2), MTG_MEAN_ROW(3), MTG_MEAN_ROW(4), MTG_MEAN_ROW(5),
    MTG_MEAN_ROW(6), MTG_MEAN_ROW(7), MTG_MEAN_ROW(8), MTG_MEAN_ROW(9), MTG_MEAN_ROW(10)};

// ... and with the LAST complex term known to have b = 0, for the small ranks (J <= 6)
template <int NR, int NC, bool OK = (NC > 0 && NR + 2 * NC <= 6)>
struct MtgMeanSelB0 { static constexpr mtg_solve_launcher fn = mtg_launch_solve_mean<NR, NC, 1>; };
template <int NR, int NC>
struct MtgMeanSelB0<NR, NC, false> { static constexpr mtg_solve_launcher fn = nullptr; };
#define MTG_MEAN_ROW_B0(nr) { nullptr, MtgMeanSelB0<(nr), 1>::fn, MtgMeanSelB0<(nr), 2>::fn, MtgMeanSelB0<(nr), 3>::fn }
const mtg_solve_launcher mtg_mean_solver_table_b0[5][4] = {MTG_MEAN_ROW_B0(0), MTG_MEAN_ROW_B0(1), MTG_MEAN_ROW_B0(2),
                                                                 MTG_MEAN_ROW_B0(3), MTG_MEAN_ROW_B0(4)};

}  // namespace

// this unit's table; the b = 0 specialisation exactly where mtg_find_solver picks it (mtg_solver_uses_b0)
#define MTG_MEAN_PASTE2(a, b) a##b
#define MTG_MEAN_PASTE(a, b) MTG_MEAN_PASTE2(a, b)
mtg_solve_launcher MTG_MEAN_PASTE(mtg_find_mean_solver_, MTG_MEAN_UNIT)(int nr, int nc, int last_b0)
{
    if (nr < 0 || nc < 0 || nr > MTG_MAX_NR || nc > MTG_MAX_NC) return nullptr;
    if (last_b0 && nr < 5 && nc < 4 && mtg_mean_solver_table_b0[nr][nc]) return mtg_mean_solver_table_b0[nr][nc];
    if (nr + nc == 0) return mtg_launch_white_mean;
    return mtg_mean_solver_table[nr][nc];
}

#if MTG_MEAN_UNIT == MTG_MEAN_SINE
mtg_solve_launcher mtg_find_mean_solver_3(int nr, int nc, int last_b0);
mtg_solve_launcher mtg_find_mean_solver_4(int nr, int nc, int last_b0);
static_assert(MTG_MEAN_SINE == 2 && MTG_MEAN_TWOSINE == 3 && MTG_MEAN_GAUSSIAN == 4, "the units' tables are named by kind");

mtg_solve_launcher mtg_find_mean_solver(int mean_kind, int nr, int nc, int last_b0)
{
    switch (mean_kind) {
    case MTG_MEAN_SINE: return mtg_find_mean_solver_2(nr, nc, last_b0);
    case MTG_MEAN_TWOSINE: return mtg_find_mean_solver_3(nr, nc, last_b0);
    case MTG_MEAN_GAUSSIAN: return mtg_find_mean_solver_4(nr, nc, last_b0);
    default: return nullptr;
    }
}
#endif
