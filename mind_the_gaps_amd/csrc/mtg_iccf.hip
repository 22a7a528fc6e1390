// mtg_iccf.hip -- the interpolated cross-correlation function (Gaskell & Peterson 1987; White & Peterson 1994) of every
// resident light curve and a companion series on its own sampling, on a grid of lags (mtg_iccf of include/mtg.h, where the
// definition and its operation order stand).
//
// One lane owns a lag, a workgroup MTG_ICCF_LANES lags and, on shared resident sampling, a tile of R light curves
// (mtg_iccf_plan.h).  A half is one walk: the lane takes the samples of the WALKED series in ascending order, shifts each
// by its lag, x = fl(time + shift), and interpolates the OTHER series at x.
//   half A   walks the resident samples, shift = tau, interpolates the companion's residuals;
//   half B   walks the companion's samples, shift = -tau (fl(t2 - tau) == fl(t2 + (-tau))), interpolates the resident ones.
// For a fixed lane x does not decrease along the walk, so the samples with x inside the other series' span are one
// contiguous run [i0, i1): both ends are found by a binary search on the rounded x itself, the predicate the walk then
// repeats, and the bracket p -- the largest index with node time <= x -- only moves up: O(N + M) per lane and half.
// The walk's trip count is the wave's: from the smallest i0 to the largest i1 of its 64 lanes, so that the walked sample
// of a step is the same for the whole wave and is read once on the scalar path; a lane outside its own run idles.  The
// launcher hands the lanes their lags in ascending order (args.order), so a wave's runs nearly coincide and its brackets
// at one step are neighbours.  The bracket's node times and values are plain cached gathers: nothing is staged.
//
// What a tile shares: the walk, x, the bracket, the weight and the count always; the interpolated value too where the
// interpolated series is one row for the tile (half A with one companion for all light curves), and with it its two sums.
// Every light curve's sums are the same sequence of operations in every instantiation: an entry does not depend on R,
// PER, the lag's place in the grid or the slab.  The finished r goes straight to the slab's [Ls][K] values; a second
// kernel, one lane per light curve, forms peak, peak_index and centroid from a row with k ascending.  No atomics, no
// LDS, no scratch: profiles/iccf_resources.txt.  The C entry: mtg_capi.hip.
#include "mtg_device.h"
#include "mtg_iccf_plan.h"

namespace {

struct MtgIccfKernelArgs {
    const double2 *dxt, *yv;   // the resident set
    int64_t N, t_stride;       // 0 (shared sampling) or N
    int64_t l0, Ls;            // this launch takes light curves [l0, l0 + Ls)
    const double4 *stats;      // [L]: ybar first -- mtg_lomb_scargle_stats_kernel's, unweighted
    const double *t2;          // [M] the companion's times, ascending
    const double2 *yv2;        // [L2][M]: y2 first
    const double4 *stats2;     // [L2]: ybar2 first, the same kernel's
    int64_t M, K;
    const double *tau;         // [K] as the caller gave them
    const int32_t *order;      // [K]: lane k of the grid takes the lag order[k] (ascending tau)
    int lag_blocks, mode;
    double *ccf;               // each NULL or [Ls][K] of the slab
    int64_t *n_a, *n_b;
};

__device__ __forceinline__ int64_t wave_uniform(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int64_t wave_min(int64_t v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t o = __shfl_xor((long long)v, m);
        v = o < v ? o : v;
    }
    return wave_uniform(v);
}

__device__ __forceinline__ int64_t wave_max(int64_t v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t o = __shfl_xor((long long)v, m);
        v = o > v ? o : v;
    }
    return wave_uniform(v);
}

// r of one half from its six sums, a the walked and b the interpolated series (the formula is symmetric in the two): the
// operation order of include/mtg.h
__device__ __forceinline__ double iccf_r(int64_t n, double Sa, double Saa, double Sb, double Sbb, double Sab)
{
#pragma clang fp contract(off)
    const double nan = __builtin_nan("");
    if (n < 2) return nan;
    const double dn = (double)n;
    const double C = Sab - (Sa * Sb) / dn;
    const double Va = Saa - (Sa * Sa) / dn;
    const double Vb = Sbb - (Sb * Sb) / dn;
    if (!(Va > 0.0) || !(Vb > 0.0)) return nan;
    const double r = C / __builtin_sqrt(Va * Vb);
    return __builtin_isfinite(r) ? r : nan;
}

// One half for one lane.  The walked series: P samples at the times wt(i) with RW rows of residuals wv(j, i); the
// interpolated one: Q nodes at nt(p) with RI rows nv(j, p); RW and RI are R or 1 (a row shared by the tile).  -> r[R], n.
template <int R, int RW, int RI, class WalkT, class WalkV, class NodeT, class NodeV>
__device__ __forceinline__ void iccf_half(int64_t P, int64_t Q, double shift, WalkT wt, WalkV wv, NodeT nt, NodeV nv, double (&r)[R],
                                          int64_t &n_out)
{
#pragma clang fp contract(off)
    const double first = nt(0), last = nt(Q - 1);
    // the lane's run [i0, i1): the first sample with x >= first, the first with x > last
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (wt(mid) + shift >= first) hi = mid; else lo = mid + 1;
    }
    const int64_t i0 = lo;
    hi = P;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (wt(mid) + shift > last) hi = mid; else lo = mid + 1;
    }
    const int64_t i1 = lo;
    // the bracket of the run's first sample: the first node beyond x, less one (node 0 is at or below x)
    int64_t p = 0;
    if (i0 < i1) {
        const double x = wt(i0) + shift;
        lo = 0; hi = Q;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (nt(mid) > x) hi = mid; else lo = mid + 1;
        }
        p = lo - 1;
    }
    double u0 = nt(p), u1 = p + 1 < Q ? nt(p + 1) : __builtin_inf();

    double Sw[RW], Sww[RW], Sv[RI], Svv[RI], Swv[R];
#pragma unroll
    for (int j = 0; j < RW; ++j) Sw[j] = Sww[j] = 0.0;
#pragma unroll
    for (int j = 0; j < RI; ++j) Sv[j] = Svv[j] = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) Swv[j] = 0.0;
    int64_t n = 0;

    const int64_t begin = wave_min(i0 < i1 ? i0 : P), end = wave_max(i0 < i1 ? i1 : 0);
    for (int64_t i = begin; i < end; ++i) {
        const double t = wt(i);                            // the same for the whole wave
        double w[RW];
#pragma unroll
        for (int j = 0; j < RW; ++j) w[j] = wv(j, i);
        if (i < i0 || i >= i1) continue;
        const double x = t + shift;
        while (u1 <= x) {                                  // at most Q - 1 times per lane over the whole walk
            ++p;
            u0 = u1;
            u1 = p + 1 < Q ? nt(p + 1) : __builtin_inf();
        }
        const bool at_end = p + 1 >= Q;                    // x == last: the value of the last node
        const int64_t q = at_end ? p : p + 1;
        const double wgt = (x - u0) / (u1 - u0);
        double v[RI];
#pragma unroll
        for (int j = 0; j < RI; ++j) {
            const double z0 = nv(j, p), z1 = nv(j, q);
            v[j] = at_end ? z0 : __builtin_fma(wgt, z1 - z0, z0);
        }
        n += 1;
#pragma unroll
        for (int j = 0; j < RW; ++j) {
            Sw[j] = Sw[j] + w[j];
            Sww[j] = __builtin_fma(w[j], w[j], Sww[j]);
        }
#pragma unroll
        for (int j = 0; j < RI; ++j) {
            Sv[j] = Sv[j] + v[j];
            Svv[j] = __builtin_fma(v[j], v[j], Svv[j]);
        }
#pragma unroll
        for (int j = 0; j < R; ++j) Swv[j] = __builtin_fma(w[RW == 1 ? 0 : j], v[RI == 1 ? 0 : j], Swv[j]);
    }
#pragma unroll
    for (int j = 0; j < R; ++j)
        r[j] = iccf_r(n, Sw[RW == 1 ? 0 : j], Sww[RW == 1 ? 0 : j], Sv[RI == 1 ? 0 : j], Svv[RI == 1 ? 0 : j], Swv[j]);
    n_out = n;
}

// R light curves per lane; PER: a companion row per light curve, else one for all; ALL: both halves, else half A alone
template <int R, bool PER, bool ALL>
__global__ void __launch_bounds__(MTG_ICCF_LANES, 2)
mtg_iccf_kernel(const MtgIccfKernelArgs a)
{
#pragma clang fp contract(off)
    constexpr int T = MTG_ICCF_LANES, RS = PER ? R : 1;    // RS: companion rows a tile reads
    const int64_t N = a.N, M = a.M, K = a.K;
    const int64_t tile = blockIdx.x / a.lag_blocks;
    const int64_t k = (int64_t)(blockIdx.x - tile * a.lag_blocks) * T + threadIdx.x;
    const bool live = k < K;                               // (idle lanes repeat the last lag and store nothing)
    const int64_t kout = a.order[live ? k : K - 1];
    const double tau = a.tau[kout];
    const int64_t lt = a.l0 + tile * R;                    // first light curve of the tile
    const int nl = (int)(a.l0 + a.Ls - lt < R ? a.l0 + a.Ls - lt : R);
    const double2 *dxt = a.dxt + lt * a.t_stride;
    const double *t2 = a.t2;

    // the rows of the tile (a lane of a partly filled tile repeats row 0 and stores nothing for it)
    const double2 *y[R], *y2[RS];
    double ybar[R], ybar2[RS];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int64_t l = lt + (j < nl ? j : 0);
        y[j] = a.yv + l * N;
        ybar[j] = a.stats[l].x;
    }
#pragma unroll
    for (int j = 0; j < RS; ++j) {
        const int64_t l = PER ? lt + (j < nl ? j : 0) : 0;
        y2[j] = a.yv2 + l * M;
        ybar2[j] = a.stats2[l].x;
    }
    auto resident_t = [&](int64_t i) { return dxt[i].y; };
    auto resident_r = [&](int j, int64_t i) { return y[j][i].x - ybar[j]; };
    auto companion_t = [&](int64_t i) { return t2[i]; };
    auto companion_s = [&](int j, int64_t i) { return y2[j][i].x - ybar2[j]; };

    const double nan = __builtin_nan("");
    double ra[R], rb[R];
    int64_t na = 0, nb = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) ra[j] = rb[j] = nan;
    if (!ALL || a.mode != MTG_ICCF_RESIDENT) iccf_half<R, R, RS>(N, M, tau, resident_t, resident_r, companion_t, companion_s, ra, na);
    if (ALL) iccf_half<R, RS, R>(M, N, -tau, companion_t, companion_s, resident_t, resident_r, rb, nb);
    if (!live) return;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= nl) continue;
        const int64_t at = (lt - a.l0 + j) * K + kout;
        if (a.ccf) a.ccf[at] = !ALL ? ra[j] : a.mode == MTG_ICCF_RESIDENT ? rb[j] : 0.5 * (ra[j] + rb[j]);
        if (a.n_a) a.n_a[at] = na;
        if (a.n_b) a.n_b[at] = nb;
    }
}

// one lane per light curve of the slab: the row's largest finite value and the first k attaining it, then the centroid of
// the lags whose value is finite and at or above threshold x peak, both sums with k ascending
__global__ void __launch_bounds__(MTG_ICCF_LANES)
mtg_iccf_peak_kernel(const double *ccf, int64_t K, const double *tau, double threshold, int64_t l0, int64_t Ls, double *peak,
                     int64_t *peak_index, double *centroid)
{
#pragma clang fp contract(off)
    const int64_t l = (int64_t)blockIdx.x * MTG_ICCF_LANES + threadIdx.x;
    if (l >= Ls) return;
    const double *row = ccf + l * K;
    const double nan = __builtin_nan("");
    double best = nan;
    int64_t at = -1;
    for (int64_t k = 0; k < K; ++k) {
        const double r = row[k];
        if (__builtin_isfinite(r) && (at < 0 || r > best)) { best = r; at = k; }
    }
    if (peak) peak[l0 + l] = best;
    if (peak_index) peak_index[l0 + l] = at;
    if (!centroid) return;
    double num = 0.0, den = 0.0;
    if (at >= 0) {
        const double cut = threshold * best;
        for (int64_t k = 0; k < K; ++k) {
            const double r = row[k];
            if (!__builtin_isfinite(r) || !(r >= cut)) continue;
            num = __builtin_fma(tau[k], r, num);
            den = den + r;
        }
    }
    centroid[l0 + l] = at >= 0 && den > 0.0 ? num / den : nan;
}

template <int R>
hipError_t iccf_launch(const MtgIccfKernelArgs &g, const MtgIccfPlan &plan, int64_t blocks, hipStream_t s)
{
    const dim3 grid((unsigned)blocks), lanes(MTG_ICCF_LANES);
    if (plan.per && plan.all) hipLaunchKernelGGL((mtg_iccf_kernel<R, true, true>), grid, lanes, 0, s, g);
    else if (plan.per) hipLaunchKernelGGL((mtg_iccf_kernel<R, true, false>), grid, lanes, 0, s, g);
    else if (plan.all) hipLaunchKernelGGL((mtg_iccf_kernel<R, false, true>), grid, lanes, 0, s, g);
    else hipLaunchKernelGGL((mtg_iccf_kernel<R, false, false>), grid, lanes, 0, s, g);
    return hipGetLastError();
}

}  // namespace

hipError_t mtg_launch_iccf(const MtgIccfArgs &q, const MtgIccfPlan &plan, int64_t l0, int64_t Ls, hipStream_t s)
{
    const MtgLombScargleArgs &ls = q.ls;
    const bool want_peak = q.peak || q.peak_index || q.centroid;
    if (ls.N < 2 || q.M < 2 || q.M >= MTG_ICCF_MAX_M || q.K < 1 || q.K > MTG_ICCF_PLAN_MAX_LAGS || Ls < 1 || l0 < 0 || l0 + Ls > ls.L ||
        Ls > plan.slab || plan.tile < 1 || (plan.tile != 1 && ls.t_stride != 0) || plan.lag_blocks != (q.K + MTG_ICCF_LANES - 1) / MTG_ICCF_LANES ||
        q.mode < MTG_ICCF_BOTH || q.mode > MTG_ICCF_RESIDENT || plan.all != (q.mode != MTG_ICCF_COMPANION) || (want_peak && !q.ccf) ||
        !(q.ccf || q.n_a || q.n_b))
        return hipErrorInvalidValue;
    const int64_t blocks = mtg_iccf_blocks(plan, Ls);
    if (blocks == 0) return hipErrorInvalidValue;
    MtgIccfKernelArgs g;
    g.dxt = ls.dxt; g.yv = ls.yv; g.N = ls.N; g.t_stride = ls.t_stride; g.l0 = l0; g.Ls = Ls;
    g.stats = reinterpret_cast<const double4 *>(ls.stats);
    g.t2 = q.t2; g.yv2 = q.yv2; g.stats2 = reinterpret_cast<const double4 *>(q.stats2); g.M = q.M;
    g.K = q.K; g.tau = q.tau; g.order = q.order; g.lag_blocks = (int)plan.lag_blocks; g.mode = q.mode;
    g.ccf = q.ccf; g.n_a = q.n_a; g.n_b = q.n_b;
    hipError_t e;
    switch (plan.tile) {
    case 1: e = iccf_launch<1>(g, plan, blocks, s); break;
    case MTG_ICCF_TILE: e = iccf_launch<MTG_ICCF_TILE>(g, plan, blocks, s); break;
    default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess || !want_peak) return e;
    hipLaunchKernelGGL(mtg_iccf_peak_kernel, dim3((unsigned)((Ls + MTG_ICCF_LANES - 1) / MTG_ICCF_LANES)), dim3(MTG_ICCF_LANES), 0, s,
                       q.ccf, q.K, q.tau, q.threshold, l0, Ls, q.peak, q.peak_index, q.centroid);
    return hipGetLastError();
}
