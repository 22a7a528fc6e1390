// mtg_wwz.hip -- Foster's weighted wavelet Z-transform (Foster 1996, AJ 112, 1709) of every resident light curve at a
// list of frequencies and window centres (mtg_wwz of include/mtg.h): the floating-mean Lomb-Scargle fit of
// mtg_lomb_scargle.hip with every sample weighted by a Gaussian window around tau whose width is a fixed number of cycles.
//
// For one (light curve, tau, f), with te_n = t_n - tau, s_n the statistical weight (sigma_n^-2 / sum sigma^-2, or 1),
// r_n = y_n - ybar of the Lomb-Scargle pre-pass and te_* the te_n of smallest magnitude:
//   E_n = ((4 pi^2 c f) f) (te_n te_n - te_* te_*),   w_n = s_n exp(-E_n), and w_n = 0 where E_n > 80 ln 2   (the cut)
//   sums of w, w^2, w c, w s, w c^2, w c s and of w r, w r^2, w r c, w r s, (c, s) = mtg_cycles_sincos(f, te_n);
// divided by sum w they are the means the header's formulas start from.  E_n is a product of rounded, monotone steps: it
// does not decrease with f or with |te_n|.
//
// One lane owns a frequency; a workgroup has one tau and a tile of R light curves on shared sampling, and walks the
// samples in the chunks of MTG_LS_CHUNK that mtg_ls_tile.h's sweep walks, on that header's pieces: MtgLsArgs inside
// WwzArgs, LsLane::locate with the tile and the frequency block of a grid that has the centres as a third factor and
// q.t0 = tau, ls_stage_chunk with the columns (s, r) and r of WwzColumns, ls_read_sample.  The ragged chunk, the partly
// filled tile, l0 > 0 and idle lanes are that header's; the chunk range, te^2 - te_*^2, the cut, the window, the ten
// sums, the solve and the [Ls][T][F] store are this file's.  Weighted, every light curve has its ten sums; unweighted
// the six weight and trigonometric sums are the tile's.
//
// Skipping.  A chunk all of whose samples are cut at the workgroup's lowest frequency is cut at every lane's (E is
// monotone in f), and the sample of a chunk nearest to tau is one of its ends or lies across tau (the times ascend, and
// so do the rounded te_n): the kept chunks are found from the chunks' end samples and form one range.  A cut sample adds
// +0 to sums that start at +0 and are never -0, so leaving a sample or a whole chunk out changes no bit: inside a kept
// chunk a lane passes its cut samples over, and a wave all of whose lanes do so skips the sample's arithmetic.
//
// Order.  Samples ascending; the sums of a chunk start from zero and are added to the running totals at its end.  The
// arithmetic of one (light curve, tau, f) is the same sequence of operations in every instantiation: an entry depends on
// (light curve, f, tau, c, statistic, weighted) alone.  No scratch, two waves per SIMD: profiles/wwz_resources.txt.
#include "mtg_ls_tile.h"
#include "mtg_wwz_plan.h"
#include "../../include/mtg.h"

static_assert(MTG_WWZ_CHUNK == MTG_LS_CHUNK, "mtg_wwz_plan.h budgets the chunk of the Lomb-Scargle sweep");
static_assert(MTG_WWZ_MAX_LANES == MTG_LS_THREADS, "the peaks are reduced by the Lomb-Scargle unit's kernel");

namespace {

#define MTG_WWZ_CUT (80.0 * 0x1.62e42fefa39efp-1)   /* 80 ln 2 */

struct WwzArgs {
    MtgLsArgs a;             // (power: NULL or the values [Ls][T][F] of this slab; normalization unused)
    int64_t T;
    const double *taus;      // [T]
    double kc;               // 4 pi^2 c
    int statistic;
    const double *near2;     // [samplings of the slab][T]: te_* te_*
    double *neff;            // NULL or [Ls][T][F] of this slab
};

// the chunk's columns hold (s, r) and r: the weight of a sample is s times the lane's window (unweighted the window alone)
struct WwzColumns {
    static __device__ __forceinline__ double2 weighted(double s, double r) { return make_double2(s, r); }
    static __device__ __forceinline__ double plain(double, double r) { return r; }
};

// te_* te_* of every (sampling of the slab, tau): the sample on either side of tau by bisection of the ascending times
__global__ void __launch_bounds__(64)
mtg_wwz_nearest_kernel(const double2 *__restrict__ dxt, int64_t N, int64_t t_stride, int64_t S, int64_t T, const double *__restrict__ taus,
                       double *__restrict__ near2)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (e >= S * T) return;
    const int64_t s = e / T;
    const double2 *t = dxt + s * t_stride;
    const double tau = taus[e - s * T];
    int64_t lo = 0, hi = N;   // -> the first sample at or after tau
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (t[mid].y < tau) lo = mid + 1; else hi = mid;
    }
    double best = __builtin_inf();
    for (int64_t n = lo - 1; n <= lo; ++n) {
        if (n < 0 || n >= N) continue;
        const double te = t[n].y - tau;
        const double m = te * te;
        if (m < best) best = m;
    }
    near2[e] = best;
}

// the weight and trigonometric sums of a lane
struct WwzTrig {
    double w, w2, c, s, cc, cs;
    __device__ __forceinline__ void zero() { w = w2 = c = s = cc = cs = 0.0; }
    __device__ __forceinline__ void add(double wg, double co, double si)
    {
        const double wc = wg * co;
        w += wg;
        w2 = __builtin_fma(wg, wg, w2);
        c = __builtin_fma(wg, co, c);
        s = __builtin_fma(wg, si, s);
        cc = __builtin_fma(wc, co, cc);
        cs = __builtin_fma(wc, si, cs);
    }
    __device__ __forceinline__ void fold(const WwzTrig &o) { w += o.w; w2 += o.w2; c += o.c; s += o.s; cc += o.cc; cs += o.cs; }
};

// a light curve's data sums
struct WwzData {
    double x, xx, xc, xs;
    __device__ __forceinline__ void zero() { x = xx = xc = xs = 0.0; }
    __device__ __forceinline__ void add(double wg, double r, double co, double si)
    {
        const double u = wg * r;
        x += u;
        xx = __builtin_fma(u, r, xx);
        xc = __builtin_fma(u, co, xc);
        xs = __builtin_fma(u, si, xs);
    }
    __device__ __forceinline__ void fold(const WwzData &o) { x += o.x; xx += o.xx; xc += o.xc; xs += o.xs; }
};

// the entry of one (light curve, tau, f) from its sums, and N_eff
__device__ __forceinline__ double wwz_solve(const WwzTrig &t, const WwzData &d, int statistic, double *neff)
{
#pragma clang fp contract(off)
    const double sw = t.w;
    const double C = t.c / sw, S = t.s / sw, CC = t.cc / sw, CS = t.cs / sw;
    const double X = d.x / sw, XX = d.xx / sw, XC = d.xc / sw, XS = d.xs / sw;
    *neff = (sw * sw) / t.w2;
    const double vx = XX - X * X;
    const double cc = CC - C * C, ss = (1.0 - CC) - S * S, cs = CS - C * S;
    const double xc = XC - X * C, xs = XS - X * S;
    const double det = cc * ss - cs * cs;
    if (!(det > 0.0)) return __builtin_nan("");
    if (statistic == MTG_WWZ_AMPLITUDE) {
        const double ca = ((ss * xc) - (cs * xs)) / det, cb = ((cc * xs) - (cs * xc)) / det;
        return sqrt(ca * ca + cb * cb);
    }
    const double vy = ((ss * xc) * xc + (cc * xs) * xs - 2.0 * ((cs * xc) * xs)) / det;
    // a variance that is not positive -- a window that holds no more than the three fitted parameters, or a fit exact to
    // the last bit -- has no ratio: NaN, which the peaks pass over, not an infinity that would be every map's peak
    if (statistic == MTG_WWZ_POWER) return vx > 0.0 ? vy / vx : __builtin_nan("");
    const double rest = vx - vy;
    return rest > 0.0 ? ((*neff - 3.0) * vy) / (2.0 * rest) : __builtin_nan("");   // MTG_WWZ_Z
}

// R light curves per lane; WEIGHTED: statistical weights from the light curve's own sigma (all ten sums are its own),
// else 1 (the weight and trigonometric sums are the tile's)
template <int R, bool WEIGHTED>
__global__ void __launch_bounds__(MTG_WWZ_MAX_LANES, 2)
mtg_wwz_kernel(const WwzArgs g)
{
#pragma clang fp contract(off)
    static_assert(WEIGHTED || R == 1 || R % 2 == 0, "the unweighted chunk is staged as pairs of light curves");
    constexpr int CH = MTG_LS_CHUNK;
    constexpr int NT = WEIGHTED ? R : 1;               // sets of weight and trigonometric sums kept per lane
    constexpr int NP = WEIGHTED ? R : (R + 1) / 2;     // 16-byte (R = 1 unweighted: 8-byte) columns of the chunk
    __shared__ MtgLsTab tab;
    __shared__ double te_s[CH], dd_s[CH];
    __shared__ double2 col_s[NP * CH];
    __shared__ double red[MTG_WWZ_MAX_LANES];
    __shared__ int range_s[2];

    mtg_ls_fill_tab(&tab);
    const MtgLsArgs &a = g.a;
    const int tid = threadIdx.x, nth = blockDim.x;
    // workgroup -> (tile, tau, frequency block), the frequency blocks fastest
    const int64_t per_tile = (int64_t)a.nfb * g.T;
    const int64_t tile = blockIdx.x / per_tile;
    const int64_t rest = blockIdx.x - tile * per_tile;
    const int64_t jt = rest / a.nfb;
    LsLane q;
    q.locate<R>(a, tile, (int)(rest - jt * a.nfb));
    q.t0 = g.taus[jt];   // elapsed times from the window's centre
    const double ts2 = g.near2[(a.t_stride ? q.lt - a.l0 : 0) * g.T + jt];
    const double af = (g.kc * q.f) * q.f;

    // the workgroup's lowest frequency, then the range of chunks it keeps
    red[tid] = q.f;
    if (tid == 0) { range_s[0] = 0x7fffffff; range_s[1] = 0; }
    __syncthreads();
    for (int h = nth / 2; h > 0; h >>= 1) {
        if (tid < h && red[tid + h] < red[tid]) red[tid] = red[tid + h];
        __syncthreads();
    }
    const double flow = red[0];
    const double alow = (g.kc * flow) * flow;
    const int nch = (int)((a.N + CH - 1) / CH);
    for (int c = tid; c < nch; c += nth) {
        const int64_t n0 = (int64_t)c * CH, n1 = (a.N - n0 < CH ? a.N : n0 + CH) - 1;
        const double te0 = q.dxt[n0].y - q.t0, te1 = q.dxt[n1].y - q.t0;
        const double m = te0 >= 0.0 ? te0 : te1 <= 0.0 ? -te1 : 0.0;   // the least |te| a sample of the chunk can have
        const double E = alow * (m * m - ts2);
        if (!(E > MTG_WWZ_CUT)) {
            atomicMin(&range_s[0], c);
            atomicMax(&range_s[1], c + 1);
        }
    }
    __syncthreads();
    const int c_lo = range_s[0], c_hi = range_s[1];

    WwzTrig tt[NT];
    WwzData ty[R];
#pragma unroll
    for (int i = 0; i < NT; ++i) tt[i].zero();
#pragma unroll
    for (int i = 0; i < R; ++i) ty[i].zero();

    for (int c = c_lo; c < c_hi; ++c) {
        const int64_t n0 = (int64_t)c * CH;
        const int len = (int)(a.N - n0 < CH ? a.N - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: the range)
        ls_stage_chunk<R, WEIGHTED, WwzColumns>(a, q, n0, len, te_s, col_s);
        for (int i = tid; i < len; i += nth) dd_s[i] = te_s[i] * te_s[i] - ts2;   // (te_s[i] is this thread's own store)
        __syncthreads();

        WwzTrig pt[NT];
        WwzData py[R];
#pragma unroll
        for (int i = 0; i < NT; ++i) pt[i].zero();
#pragma unroll
        for (int i = 0; i < R; ++i) py[i].zero();
        for (int i = 0; i < len; ++i) {
            const double E = af * dd_s[i];
            if (E > MTG_WWZ_CUT) continue;   // the cut: this sample's weight is 0
            const double win = exp(-E);
            double si, co, s[NT], r[R];
            mtg_cycles_sincos(q.f, te_s[i], &si, &co, &tab);
            ls_read_sample<R, WEIGHTED>(col_s, i, 1.0, s, r);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const double wg = WEIGHTED ? s[j < NT ? j : 0] * win : win;   // unweighted: the window alone, no factor
                if (j < NT) pt[j].add(wg, co, si);
                py[j].add(wg, r[j], co, si);
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) tt[i].fold(pt[i]);
#pragma unroll
        for (int i = 0; i < R; ++i) ty[i].fold(py[i]);
    }

    if (q.k >= a.F) return;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= q.nl) continue;
        double ne;
        const double v = wwz_solve(tt[WEIGHTED ? j : 0], ty[j], g.statistic, &ne);
        const int64_t at = ((q.lt - a.l0 + j) * g.T + jt) * a.F + q.k;
        if (a.power) a.power[at] = v;
        if (g.neff) g.neff[at] = ne;
    }
}

template <int R, bool WEIGHTED>
void wwz_launch(const WwzArgs &g, int64_t blocks, int lanes, hipStream_t s)
{
    hipLaunchKernelGGL((mtg_wwz_kernel<R, WEIGHTED>), dim3((unsigned)blocks), dim3(lanes), 0, s, g);
}

}  // namespace

hipError_t mtg_launch_wwz(const MtgWwzArgs &q, const MtgWwzPlan &plan, int64_t l0, int64_t Ls, hipStream_t s)
{
    constexpr int RW = mtg_wwz_full_tile(1), RU = mtg_wwz_full_tile(0);
    const MtgLombScargleArgs &ls = q.ls;
    const int64_t blocks = mtg_wwz_blocks(plan, q.T, Ls);
    const int R = plan.tile;
    if (blocks == 0 || plan.lanes > MTG_WWZ_MAX_LANES || (R != 1 && R != (ls.weighted ? RW : RU)) || (ls.t_stride != 0 && R != 1))
        return hipErrorInvalidValue;
    // te_*^2 of the slab's samplings: one row on shared sampling
    const int64_t S = ls.t_stride ? Ls : 1;
    hipLaunchKernelGGL(mtg_wwz_nearest_kernel, dim3((unsigned)((S * q.T + 63) / 64)), dim3(64), 0, s, ls.dxt + l0 * ls.t_stride, ls.N,
                       ls.t_stride, S, q.T, q.taus, q.nearest);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    WwzArgs g;
    g.a = mtg_ls_args(ls, l0, Ls, plan.nfb);
    g.T = q.T; g.taus = q.taus; g.kc = q.kc; g.statistic = q.statistic; g.near2 = q.nearest; g.neff = q.neff;
    if (ls.weighted) {
        if (R == 1) wwz_launch<1, true>(g, blocks, plan.lanes, s);
        else wwz_launch<RW, true>(g, blocks, plan.lanes, s);
    } else {
        if (R == 1) wwz_launch<1, false>(g, blocks, plan.lanes, s);
        else wwz_launch<RU, false>(g, blocks, plan.lanes, s);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ls.power && (ls.peak_power || ls.peak_index)) {   // a light curve's map is one row of T F entries to the Lomb-Scargle unit's reduction
        MtgLombScargleArgs rows = ls;
        rows.F = q.T * ls.F;
        mtg_launch_lomb_scargle_peaks(rows, l0, Ls, s);
        e = hipGetLastError();
    }
    return e;
}
