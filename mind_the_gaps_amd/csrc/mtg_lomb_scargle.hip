// mtg_lomb_scargle.hip -- the generalised (floating-mean) Lomb-Scargle periodogram of every resident light curve at a
// list of frequencies (mtg_lomb_scargle of include/mtg.h): astropy's LombScargle(fit_mean=True, center_data=True,
// nterms=1).power.
//
// With weights w_n (sigma_n^-2 / sum sigma^-2, or 1 / N), ybar = sum w y, r = y - ybar, YY = sum w r^2 and
// c_n, s_n = cos, sin(2 pi f (t_n - t_0)):
//   C = sum w c, S = sum w s, YC = sum w r c, YS = sum w r s,
//   CC = sum w c^2 - C^2, SS = sum w s^2 - S^2, CS = sum w c s - C S,
//   p = (SS YC^2 + CC YS^2 - 2 CS YC YS) / (CC SS - CS^2)
// the tau-free form of Zechmeister & Kuerster (2009): algebraically astropy's YC_tau^2 / CC_tau + YS_tau^2 / SS_tau and
// invariant under a shift of the times, which is why the elapsed time t - t_0 serves and the y_offset of the resident
// set does not matter.  sum w s^2 is (sum w) - sum w c^2 with sum w = 1.
//
// Work: one (cos, sin) pair per (frequency, sample) and 2 FMAs per (frequency, sample, light curve) -- 6 when the
// weights differ from one light curve to the next.  The sweep over tiles of light curves, chunks of samples and
// frequencies, its LDS budget and its order of summation are mtg_ls_tile.h's; LsOneTerm below is this unit's model.
// Registers: the running totals and the chunk's partial sums, 2 x 6 R doubles weighted, 2 x (2 R + 4) unweighted, under
// the 256 VGPRs two waves per SIMD leave each lane (profiles/lomb_scargle_resources.txt; no scratch).
#include "mtg_ls_tile.h"
#include "mtg_ls_peak.h"

namespace {

// sum of v over the workgroup in a fixed order (thread-strided partial sums, then a binary tree): `red` holds
// MTG_LS_THREADS doubles
__device__ __forceinline__ double ls_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = MTG_LS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// Per light curve: sw = sum sigma^-2 (weighted) or N, ybar = sum w y, YY = sum w (y - ybar)^2 with w = sigma^-2 / sw
// or 1 / N -- stats[l] = (ybar, YY, sw, 0).  One workgroup per light curve, sums in an order that depends on N alone.
__global__ void __launch_bounds__(MTG_LS_THREADS)
mtg_lomb_scargle_stats_kernel(const double2 *__restrict__ yv, int64_t N, int weighted, double4 *__restrict__ stats)
{
#pragma clang fp contract(off)
    __shared__ double red[MTG_LS_THREADS];
    const int64_t l = blockIdx.x;
    const double2 *row = yv + l * N;
    const int tid = threadIdx.x;
    double sw = (double)N;
    if (weighted) {
        double a = 0.0;
        for (int64_t n = tid; n < N; n += MTG_LS_THREADS) a += 1.0 / row[n].y;
        sw = ls_block_sum(a, red);
    }
    double a = 0.0;
    for (int64_t n = tid; n < N; n += MTG_LS_THREADS) {
        const double2 v = row[n];
        const double w = weighted ? (1.0 / v.y) / sw : 1.0 / sw;
        a = __builtin_fma(w, v.x, a);
    }
    const double ybar = ls_block_sum(a, red);
    a = 0.0;
    for (int64_t n = tid; n < N; n += MTG_LS_THREADS) {
        const double2 v = row[n];
        const double w = weighted ? (1.0 / v.y) / sw : 1.0 / sw;
        const double r = v.x - ybar;
        a = __builtin_fma(w * r, r, a);
    }
    const double yy = ls_block_sum(a, red);
    if (tid == 0) stats[l] = make_double4(ybar, yy, sw, 0.0);
}

// the trig part of a lane's sums: C, S, sum w c^2, sum w c s
struct LsTrig {
    double c, s, cc, cs;
    __device__ __forceinline__ void zero() { c = s = cc = cs = 0.0; }
    __device__ __forceinline__ void add(double w, double co, double si)
    {
        const double wc = w * co;
        c = __builtin_fma(w, co, c);
        s = __builtin_fma(w, si, s);
        cc = __builtin_fma(wc, co, cc);
        cs = __builtin_fma(wc, si, cs);
    }
    __device__ __forceinline__ void fold(const LsTrig &o) { c += o.c; s += o.s; cc += o.cc; cs += o.cs; }
};

// a light curve's sums YC = sum w r c, YS = sum w r s
struct LsPair {
    double yc, ys;
    __device__ __forceinline__ void zero() { yc = ys = 0.0; }
    __device__ __forceinline__ void fold(const LsPair &o) { yc += o.yc; ys += o.ys; }
};

// one sinusoid with a floating mean: the closed form of the file header
struct LsOneTerm {
    typedef LsTrig Trig;
    typedef LsPair Data;
    template <int NT, int R>
    static __device__ __forceinline__ void accumulate(double co, double si, const double (&wt)[NT], const double (&wr)[R], LsTrig (&pt)[NT],
                                                      LsPair (&py)[R])
    {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (j < NT) pt[j].add(wt[j], co, si);
            py[j].yc = __builtin_fma(wr[j], co, py[j].yc);
            py[j].ys = __builtin_fma(wr[j], si, py[j].ys);
        }
    }
    struct Solve {
        double CC, SS, CS, det;
        __device__ __forceinline__ void prepare(const LsTrig &g)
        {
#pragma clang fp contract(off)
            CC = g.cc - g.c * g.c; SS = (1.0 - g.cc) - g.s * g.s; CS = g.cs - g.c * g.s;
            det = CC * SS - CS * CS;
        }
        __device__ __forceinline__ bool solve(const LsPair &y, double *p) const
        {
#pragma clang fp contract(off)
            const double YC = y.yc, YS = y.ys;
            const double num = (SS * YC) * YC + (CC * YS) * YS - 2.0 * ((CS * YC) * YS);
            if (!(det > 0.0)) return false;
            *p = num / det;
            return true;
        }
    };
};

// R light curves per lane; WEIGHTED: weights from the light curve's own sigma (its trig sums are its own), else 1 / N
// (the trig sums are the tile's)
template <int R, bool WEIGHTED>
__global__ void __launch_bounds__(MTG_LS_THREADS, 2)
mtg_lomb_scargle_kernel(const MtgLsArgs a)
{
    ls_tile_sweep<LsOneTerm, R, WEIGHTED>(a);
}

// the largest entry of every row of power[Ls][F] and the first index that attains it; NaN entries are passed over (a
// row of nothing else: NaN and -1).  One workgroup per row.
__global__ void __launch_bounds__(MTG_LS_THREADS)
mtg_lomb_scargle_peak_kernel(const double *__restrict__ power, int64_t F, double *__restrict__ peak, int64_t *__restrict__ index)
{
    const double *row = power + (int64_t)blockIdx.x * F;
    double v;
    int64_t at;
    ls_block_peak<MTG_LS_THREADS>(F, [row](int64_t k) { return row[k]; }, &v, &at);
    if (threadIdx.x == 0) {
        if (peak) peak[blockIdx.x] = at < 0 ? __builtin_nan("") : v;
        if (index) index[blockIdx.x] = at;
    }
}

template <int R, bool WEIGHTED>
void ls_launch(const MtgLsLaunch &g, hipStream_t s)
{
    hipLaunchKernelGGL((mtg_lomb_scargle_kernel<R, WEIGHTED>), dim3((unsigned)g.blocks), dim3(g.threads), 0, s, g.a);
}

}  // namespace

// the peaks of the slab's rows, where asked for
void mtg_launch_lomb_scargle_peaks(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, hipStream_t s)
{
    if (q.peak_power || q.peak_index)
        hipLaunchKernelGGL(mtg_lomb_scargle_peak_kernel, dim3((unsigned)Ls), dim3(MTG_LS_THREADS), 0, s, q.power, q.F,
                           q.peak_power ? q.peak_power + l0 : nullptr, q.peak_index ? q.peak_index + l0 : nullptr);
}

void mtg_launch_lomb_scargle_stats(const MtgLombScargleArgs &q, hipStream_t s)
{
    hipLaunchKernelGGL(mtg_lomb_scargle_stats_kernel, dim3((unsigned)q.L), dim3(MTG_LS_THREADS), 0, s, q.yv, q.N, q.weighted,
                       reinterpret_cast<double4 *>(q.stats));
}

int mtg_launch_lomb_scargle(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, hipStream_t s)
{
    if (q.nterms > 1) {   // the powers with harmonics come from mtg_lomb_scargle_multi.hip; the peaks are reduced here
        if (!mtg_launch_lomb_scargle_multi_powers(q, l0, Ls, s)) return 0;
    } else {
        constexpr int RW = mtg_ls_full_tile(1, 1), RU = mtg_ls_full_tile(1, 0);
        const int R = mtg_ls_tile(1, q.L, q.t_stride == 0, q.weighted);
        MtgLsLaunch g;
        if (!mtg_ls_plan_launch(q, R, l0, Ls, &g)) return 0;
        if (q.weighted) {
            if (R == 1) ls_launch<1, true>(g, s);
            else if (R == 4) ls_launch<4, true>(g, s);
            else ls_launch<RW, true>(g, s);
        } else {
            if (R == 1) ls_launch<1, false>(g, s);
            else if (R == 4) ls_launch<4, false>(g, s);
            else ls_launch<RU, false>(g, s);
        }
    }
    mtg_launch_lomb_scargle_peaks(q, l0, Ls, s);
    return 1;
}
