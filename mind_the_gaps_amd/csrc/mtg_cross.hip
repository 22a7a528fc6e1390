// mtg_cross.hip -- sums over the pairs (resident sample i, companion sample j) of every resident light curve and a second
// series on its own sampling, in bins of the signed time lag (mtg_cross_sums of include/mtg.h): what the discrete
// cross-correlation function of Edelson & Krolik (1988) and its locally normalised form are made from.
//
// For every pair, tau = fl(t2_j - t_i), and in the bin b with edges[b] <= tau < edges[b + 1]:
//   count += 1, lag += tau, p = r_i s_j: cf += p, cf2 = fma(p, p, cf2), sb += s_j, sbb = fma(s_j, s_j, sbb)
// with r = y - ybar and s = y2 - ybar2 of the Lomb-Scargle pre-pass (unweighted), run on each series.  sa and saa are
// formed by the reduction from the rows' counts (below).
//
// The sweep is mtg_lag.hip's: one lane owns a resident row i, a workgroup MTG_CROSS_LANES consecutive rows and, on shared
// resident sampling, a tile of R light curves; the companion is walked in chunks of MTG_CROSS_CHUNK columns staged in LDS,
// every lane reading the same column, so that tau and the bin decision are taken once per pair for the whole tile.  For
// a fixed row tau does not decrease with j, so the row's bin only moves up: the sums of the current bin stay in registers
// and memory is touched only when the bin changes.  What differs: every column is a pair (no i < j mask), lags are
// signed, and a row starts BELOW edges[0].
//   late start   the workgroup begins at the first chunk whose LAST column minus its FIRST row's time is >= edges[0]:
//                that row has the largest lags of the block and the rounded subtraction is monotone in both operands, so
//                no pair of any row with an earlier column is in a bin.
//   early exit   it stops at the first chunk whose first column minus its LAST row's time is >= edges[nbins].
// Both are the same for every lane of the workgroup.  A row that never enters a bin still writes its zeros.
// The companion's residuals are one LDS word per column when it is shared by the light curves (PER = false) and staged
// [column][light curve] when there is a row per light curve (PER = true).
//
// Order.  A row's partial for a bin starts from zero and takes the columns ascending; it is written once to the workspace
// of mtg_cross_plan.h.  mtg_cross_reduce_kernel then adds the rows of one (light curve, bin) by mtg_row_reduce.h: lane q
// the rows q, q + 256, ... ascending, then a binary tree.  A row's partial of sa is fl(r_i c) and of saa fl(fl(r_i^2) c)
// with c the row's pair count in the bin: the reduction forms them from the stored count and the resident data.  The
// arithmetic of a light curve is the same sequence of operations in every instantiation.  No atomics.  No scratch:
// profiles/cross_resources.txt.  The C entry: mtg_capi.hip.
#include "mtg_device.h"
#include "mtg_cross_plan.h"
#include "mtg_row_reduce.h"

namespace {

struct MtgCrossKernelArgs {
    const double2 *dxt, *yv;   // the resident set
    int64_t N, t_stride;       // 0 (shared sampling) or N
    int64_t l0, Ls;            // this launch takes light curves [l0, l0 + Ls)
    const double4 *stats;      // [L]: ybar first -- mtg_lomb_scargle_stats_kernel's, unweighted
    const double *t2;          // [M] the companion's times, ascending
    const double2 *yv2;        // [L2][M]: y2 first
    const double4 *stats2;     // [L2]: ybar2 first, the same kernel's
    int64_t M;
    int nbins, row_blocks, per_lc;   // per_lc: workspace arrays per light curve (2 or 4)
    const double *edges;       // [nbins + 1]
    double *ws;                // the slab's workspace: [per_lc][Ls][nbins][N], then lag [tiles][nbins][N], then count likewise
};

// the workspace's arrays: cf, cf2 (with everything sb, sbb behind them), then the tile's lag and count
__device__ __forceinline__ double *cross_ws_lc(const MtgCrossKernelArgs &a, int s) { return a.ws + (int64_t)s * a.Ls * a.nbins * a.N; }
__device__ __forceinline__ double *cross_ws_tile(const MtgCrossKernelArgs &a, int R, int s)
{
    return a.ws + (a.per_lc * a.Ls + s * ((a.Ls + R - 1) / R)) * a.nbins * a.N;
}

// R light curves per lane; PER: a companion row per light curve, else one for all; ALL: sb and sbb too
template <int R, bool PER, bool ALL>
__global__ void __launch_bounds__(MTG_CROSS_LANES, 2)
mtg_cross_kernel(const MtgCrossKernelArgs a)
{
#pragma clang fp contract(off)
    constexpr int CH = MTG_CROSS_CHUNK, T = MTG_CROSS_LANES;
    constexpr int RS = PER ? R : 1;                        // companion rows a tile reads
    constexpr int RB = ALL ? RS : 1;
    __shared__ double t_s[CH];
    __shared__ double edge_s[MTG_LAG_PLAN_MAX_BINS + 2];
    __shared__ __attribute__((aligned(16))) double s_s[CH * RS];

    const int tid = threadIdx.x, nb = a.nbins;
    const int64_t N = a.N, M = a.M;
    const int64_t tile = blockIdx.x / a.row_blocks;
    const int64_t row0 = (int64_t)(blockIdx.x - tile * a.row_blocks) * T;
    const int64_t lt = a.l0 + tile * R;                    // first light curve of the tile
    const int nl = (int)(a.l0 + a.Ls - lt < R ? a.l0 + a.Ls - lt : R);
    const double2 *dxt = a.dxt + lt * a.t_stride;
    const bool live = row0 + tid < N;                      // (idle lanes repeat the last row and store nothing)
    const int64_t i = live ? row0 + tid : N - 1;
    const double ti = dxt[i].y;
    const double t_first_row = dxt[row0].y;
    const double t_last_row = dxt[row0 + T <= N ? row0 + T - 1 : N - 1].y;

    double ri[R], cf[R], cf2[R], sb[RB], sbb[RB];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        ri[j] = j < nl ? a.yv[(lt + j) * N + i].x - a.stats[lt + j].x : 0.0;
        cf[j] = cf2[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) sb[j] = sbb[j] = 0.0;
    double lg = 0.0;
    int64_t cnt = 0;

    for (int e = tid; e <= nb; e += T) edge_s[e] = a.edges[e];
    const double first_edge = a.edges[0], last_edge = a.edges[nb];
    // the lane's bin: -1 below edges[0], nb at or beyond edges[nb]; `hi` is the edge at which it is left
    int b = -1;
    double hi = first_edge;

    // the sums of bin `bb` to the workspace, and zero again
    auto flush = [&](int bb) {
        const int64_t at = (int64_t)bb * N + i;
        if (live) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (j >= nl) continue;
                const int64_t lc = (lt - a.l0 + j) * nb * N + at;
                cross_ws_lc(a, 0)[lc] = cf[j];
                cross_ws_lc(a, 1)[lc] = cf2[j];
                if (ALL) { cross_ws_lc(a, 2)[lc] = sb[PER ? j : 0]; cross_ws_lc(a, 3)[lc] = sbb[PER ? j : 0]; }
            }
            cross_ws_tile(a, R, 0)[tile * nb * N + at] = lg;
            reinterpret_cast<int64_t *>(cross_ws_tile(a, R, 1))[tile * nb * N + at] = cnt;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) cf[j] = cf2[j] = 0.0;
#pragma unroll
        for (int j = 0; j < RB; ++j) sb[j] = sbb[j] = 0.0;
        lg = 0.0; cnt = 0;
    };

    // late start: skip the chunks whose last column is below the first edge even for the first row (the same for every lane)
    int64_t n0 = 0;
    for (; n0 < M; n0 += CH)
        if (a.t2[n0 + CH <= M ? n0 + CH - 1 : M - 1] - t_first_row >= first_edge) break;

    for (; n0 < M; n0 += CH) {
        if (a.t2[n0] - t_last_row >= last_edge) break;     // early exit (the same for every lane)
        const int len = (int)(M - n0 < CH ? M - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: the edges are in place)
        for (int c = tid; c < len; c += T) t_s[c] = a.t2[n0 + c];
        for (int e = tid; e < RS * CH; e += T) {
            const int j = e / CH, c = e - j * CH;
            if (c >= len) continue;
            double s = 0.0;
            if (!PER) s = a.yv2[n0 + c].x - a.stats2[0].x;
            else if (j < nl) s = a.yv2[(lt + j) * M + n0 + c].x - a.stats2[lt + j].x;
            s_s[c * RS + j] = s;
        }
        __syncthreads();

        for (int c = 0; c < len; ++c) {
            const double tau = t_s[c] - ti;
            while (tau >= hi) {                            // at most nbins + 1 times per row
                if (b >= 0) flush(b);
                ++b;
                hi = b < nb ? edge_s[b + 1] : __builtin_inf();
            }
            if (b < 0 || b >= nb) continue;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const double p = ri[j] * s_s[c * RS + (PER ? j : 0)];
                cf[j] = cf[j] + p;
                cf2[j] = __builtin_fma(p, p, cf2[j]);
            }
            if (ALL) {
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const double s = s_s[c * RS + j];
                    sb[j] = sb[j] + s;
                    sbb[j] = __builtin_fma(s, s, sbb[j]);
                }
            }
            lg = lg + tau; cnt += 1;
        }
    }
    // the bin the row ended in, and zeros for the bins it never entered
    for (int bb = b < 0 ? 0 : b; bb < nb; ++bb) flush(bb);
}

struct MtgCrossOut {
    int64_t *count;
    double *lag, *cf, *cf2, *sa, *sb, *saa, *sbb;   // each NULL or [L][nbins] of the call
};

// one workgroup per (light curve of the slab, bin): the rows' partials into the call's outputs at l0
template <int R>
__global__ void __launch_bounds__(MTG_CROSS_LANES)
mtg_cross_reduce_kernel(const MtgCrossKernelArgs a, const MtgCrossOut o)
{
#pragma clang fp contract(off)
    __shared__ double red[MTG_CROSS_LANES];
    __shared__ int64_t ired[MTG_CROSS_LANES];
    const int nb = a.nbins;
    const int64_t l = blockIdx.x / nb, b = blockIdx.x - l * nb;   // l: within the slab
    const int64_t lc = (l * nb + b) * a.N, tl = (l / R * nb + b) * a.N, at = (a.l0 + l) * nb + b;
    double *const outs[4] = {o.cf, o.cf2, o.sb, o.sbb};
    for (int s = 0; s < a.per_lc; ++s) {
        if (!outs[s]) continue;
        const double v = lag_row_sum(cross_ws_lc(a, s) + lc, a.N, red);
        if (threadIdx.x == 0) outs[s][at] = v;
    }
    if (o.lag) {
        const double v = lag_row_sum(cross_ws_tile(a, R, 0) + tl, a.N, red);
        if (threadIdx.x == 0) o.lag[at] = v;
    }
    const int64_t *counts = reinterpret_cast<const int64_t *>(cross_ws_tile(a, R, 1)) + tl;
    if (o.count) {
        const int64_t v = lag_row_sum(counts, a.N, ired);
        if (threadIdx.x == 0) o.count[at] = v;
    }
    // the local moments of the resident series: a row's partial is r_i, or r_i^2 rounded, times its pair count
    const double2 *y = a.yv + (a.l0 + l) * a.N;
    const double ybar = a.stats[a.l0 + l].x;
    if (o.sa) {
        const double v = lag_row_sum_of(a.N, red, [=](int64_t n) {
#pragma clang fp contract(off)
            return (y[n].x - ybar) * (double)counts[n];
        });
        if (threadIdx.x == 0) o.sa[at] = v;
    }
    if (o.saa) {
        const double v = lag_row_sum_of(a.N, red, [=](int64_t n) {
#pragma clang fp contract(off)
            const double r = y[n].x - ybar;
            const double rr = r * r;
            return rr * (double)counts[n];
        });
        if (threadIdx.x == 0) o.saa[at] = v;
    }
}

template <int R, bool PER>
hipError_t cross_launch(const MtgCrossKernelArgs &g, const MtgCrossOut &o, bool all, int64_t blocks, hipStream_t s)
{
    if (all) hipLaunchKernelGGL((mtg_cross_kernel<R, PER, true>), dim3((unsigned)blocks), dim3(MTG_CROSS_LANES), 0, s, g);
    else hipLaunchKernelGGL((mtg_cross_kernel<R, PER, false>), dim3((unsigned)blocks), dim3(MTG_CROSS_LANES), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mtg_cross_reduce_kernel<R>), dim3((unsigned)(g.Ls * g.nbins)), dim3(MTG_CROSS_LANES), 0, s, g, o);
    return hipGetLastError();
}

template <int R>
hipError_t cross_launch(const MtgCrossKernelArgs &g, const MtgCrossOut &o, const MtgCrossPlan &plan, int64_t blocks, hipStream_t s)
{
    return plan.per ? cross_launch<R, true>(g, o, plan.all, blocks, s) : cross_launch<R, false>(g, o, plan.all, blocks, s);
}

}  // namespace

hipError_t mtg_launch_cross(const MtgCrossArgs &q, const MtgCrossPlan &plan, int64_t l0, int64_t Ls, hipStream_t s)
{
    const MtgLombScargleArgs &ls = q.ls;
    const int64_t blocks = mtg_lag_launch_blocks(plan, ls.N, ls.t_stride, ls.L, q.nbins, l0, Ls);
    if (blocks == 0 || q.M < 1 || q.M >= MTG_CROSS_MAX_M || plan.per_lc != (plan.all ? 4 : 2) || plan.per_tile != 2) return hipErrorInvalidValue;
    MtgCrossKernelArgs g;
    g.dxt = ls.dxt; g.yv = ls.yv; g.N = ls.N; g.t_stride = ls.t_stride; g.l0 = l0; g.Ls = Ls;
    g.stats = reinterpret_cast<const double4 *>(ls.stats);
    g.t2 = q.t2; g.yv2 = q.yv2; g.stats2 = reinterpret_cast<const double4 *>(q.stats2); g.M = q.M;
    g.nbins = q.nbins; g.row_blocks = (int)plan.row_blocks; g.per_lc = plan.per_lc; g.edges = q.edges; g.ws = q.ws;
    MtgCrossOut o;
    o.count = q.count; o.lag = q.lag; o.cf = q.cf; o.cf2 = q.cf2; o.sa = q.sa; o.sb = q.sb; o.saa = q.saa; o.sbb = q.sbb;
    if (!plan.all && (o.sa || o.sb || o.saa || o.sbb)) return hipErrorInvalidValue;
    switch (plan.tile) {
    case 1: return cross_launch<1>(g, o, plan, blocks, s);
    case 4: return cross_launch<4>(g, o, plan, blocks, s);
    case MTG_CROSS_TILE: return cross_launch<MTG_CROSS_TILE>(g, o, plan, blocks, s);
    default: return hipErrorInvalidValue;
    }
}
