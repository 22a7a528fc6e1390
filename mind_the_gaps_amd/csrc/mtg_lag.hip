// mtg_lag.hip -- sums over the pairs of samples of every resident light curve in bins of the time lag (mtg_lag_sums of
// include/mtg.h): what the structure function and the discrete correlation function of Edelson & Krolik (1988) are
// normalised from.
//
// For every pair i < j of a light curve, tau = fl(t_j - t_i), and in the bin b with edges[b] <= tau < edges[b + 1]:
//   count += 1, lag += tau, sf = fma(d, d, sf) with d = y_j - y_i,
//   p = r_i r_j: cf += p, cf2 = fma(p, p, cf2),  noise += sigma_i^2 + sigma_j^2
// with r = y - ybar of the Lomb-Scargle pre-pass (unweighted).
//
// Two facts about ascending times shape the sweep.  One lane owns a row i and a workgroup a block of MTG_LAG_LANES
// consecutive rows and, on shared sampling, a tile of R light curves; it walks the columns j in chunks of MTG_LAG_CHUNK
// staged in LDS, every lane reading the same column (a broadcast), so that tau and the bin decision are taken once per
// pair for the whole tile.  And for a fixed row tau does not decrease with j, so the row's bin only moves up: the lane
// keeps the sums of its current bin in registers and the next edge beside them, and touches memory only when the bin
// changes.  The columns are staged sample-major, [column][light curve], so that a lane's reads of one column are
// consecutive (ds_read_b128 for two light curves).  A workgroup starts at the chunk that holds its own first row and
// stops at the first chunk whose first column is past the last edge for its LAST row (the row with the smallest lags;
// the rounded subtraction is monotone, so every other pair of that and the later chunks is past it too).
//
// Order.  A row's partial sum for a bin starts from zero and takes the columns ascending; it is written once to the
// workspace of mtg_lag_plan.h (zeros for the bins the row never enters).  mtg_lag_reduce_kernel then adds the rows of
// one (light curve, bin) by mtg_row_reduce.h: lane q the rows q, q + 256, ... ascending, then a binary tree over the lanes.  The arithmetic
// of a light curve is the same sequence of operations in every instantiation: an output depends on (light curve, edges)
// alone.  No atomics.  No scratch: profiles/lag_resources.txt.  The C entry: mtg_capi.hip.
#include "mtg_device.h"
#include "mtg_lag_plan.h"
#include "mtg_row_reduce.h"

namespace {

struct MtgLagKernelArgs {
    const double2 *dxt, *yv;
    int64_t N, t_stride;     // 0 (shared sampling) or N
    int64_t l0, Ls;          // this launch takes light curves [l0, l0 + Ls)
    const double4 *stats;    // [L]: ybar first -- mtg_lomb_scargle_stats_kernel's, unweighted
    int nbins, row_blocks;
    const double *edges;     // [nbins + 1]
    double *ws;              // the slab's workspace: [per_lc][Ls][nbins][N], then lag [tiles][nbins][N], then count likewise
};

// the workspace's arrays: sf first; with everything cf, cf2, noise behind it, then the tile's lag and count
__device__ __forceinline__ double *lag_ws_lc(const MtgLagKernelArgs &a, int s) { return a.ws + (int64_t)s * a.Ls * a.nbins * a.N; }
__device__ __forceinline__ double *lag_ws_tile(const MtgLagKernelArgs &a, int R, int s)
{
    return a.ws + (4 * a.Ls + s * ((a.Ls + R - 1) / R)) * a.nbins * a.N;
}

// R light curves per lane; ALL: every sum, else the structure function's alone
template <int R, bool ALL>
__global__ void __launch_bounds__(MTG_LAG_LANES, 2)
mtg_lag_kernel(const MtgLagKernelArgs a)
{
#pragma clang fp contract(off)
    constexpr int CH = MTG_LAG_CHUNK, T = MTG_LAG_LANES;
    static_assert(CH == T, "a row block starts at a chunk's first column");
    __shared__ double t_s[CH];
    __shared__ double edge_s[MTG_LAG_PLAN_MAX_BINS + 2];
    __shared__ __attribute__((aligned(16))) double y_s[CH * R];
    __shared__ __attribute__((aligned(16))) double r_s[ALL ? CH * R : 1];
    __shared__ __attribute__((aligned(16))) double v_s[ALL ? CH * R : 1];

    const int tid = threadIdx.x, nb = a.nbins;
    const int64_t N = a.N;
    const int64_t tile = blockIdx.x / a.row_blocks;
    const int64_t row0 = (int64_t)(blockIdx.x - tile * a.row_blocks) * T;
    const int64_t lt = a.l0 + tile * R;                    // first light curve of the tile
    const int nl = (int)(a.l0 + a.Ls - lt < R ? a.l0 + a.Ls - lt : R);
    const double2 *dxt = a.dxt + lt * a.t_stride;
    const bool live = row0 + tid < N;                      // (idle lanes repeat the last row, which has no pairs, and store nothing)
    const int64_t i = live ? row0 + tid : N - 1;
    const double ti = dxt[i].y;
    const double t_last_row = dxt[row0 + T <= N ? row0 + T - 1 : N - 1].y;

    double yi[R], ri[ALL ? R : 1], vi[ALL ? R : 1];
    double sf[R], cf[ALL ? R : 1], cf2[ALL ? R : 1], nz[ALL ? R : 1];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        double2 v = make_double2(0.0, 0.0);
        double ybar = 0.0;
        if (j < nl) { v = a.yv[(lt + j) * N + i]; ybar = a.stats[lt + j].x; }
        yi[j] = v.x; sf[j] = 0.0;
        if (ALL) { ri[j] = v.x - ybar; vi[j] = v.y; cf[j] = cf2[j] = nz[j] = 0.0; }
    }
    double lg = 0.0;
    int64_t cnt = 0;

    for (int e = tid; e <= nb; e += T) edge_s[e] = a.edges[e];
    const double last_edge = a.edges[nb];
    // the lane's bin: -1 below edges[0], nb at or beyond edges[nb]; `hi` is the edge at which it is left
    int b = -1;
    double hi = a.edges[0];

    // the sums of bin `bb` to the workspace, and zero again
    auto flush = [&](int bb) {
        const int64_t at = (int64_t)bb * N + i;
        if (live) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (j >= nl) continue;
                const int64_t lc = (lt - a.l0 + j) * nb * N + at;
                lag_ws_lc(a, 0)[lc] = sf[j];
                if (ALL) { lag_ws_lc(a, 1)[lc] = cf[j]; lag_ws_lc(a, 2)[lc] = cf2[j]; lag_ws_lc(a, 3)[lc] = nz[j]; }
            }
            if (ALL) {
                lag_ws_tile(a, R, 0)[tile * nb * N + at] = lg;
                reinterpret_cast<int64_t *>(lag_ws_tile(a, R, 1))[tile * nb * N + at] = cnt;
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            sf[j] = 0.0;
            if (ALL) cf[j] = cf2[j] = nz[j] = 0.0;
        }
        lg = 0.0; cnt = 0;
    };

    for (int64_t n0 = row0; n0 < N; n0 += CH) {
        if (dxt[n0].y - t_last_row >= last_edge) break;    // (the same for every lane)
        const int len = (int)(N - n0 < CH ? N - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: nothing)
        for (int c = tid; c < len; c += T) t_s[c] = dxt[n0 + c].y;
        for (int e = tid; e < R * CH; e += T) {
            const int j = e / CH, c = e - j * CH;
            if (c >= len) continue;
            double2 v = make_double2(0.0, 0.0);
            double ybar = 0.0;
            if (j < nl) { v = a.yv[(lt + j) * N + n0 + c]; ybar = a.stats[lt + j].x; }
            y_s[c * R + j] = v.x;
            if (ALL) { r_s[c * R + j] = v.x - ybar; v_s[c * R + j] = v.y; }
        }
        __syncthreads();

        for (int c = 0; c < len; ++c) {
            const double tau = t_s[c] - ti;
            if (n0 + c <= i) continue;                     // pairs i < j only
            while (tau >= hi) {                            // at most nbins + 1 times per row
                if (b >= 0) flush(b);
                ++b;
                hi = b < nb ? edge_s[b + 1] : __builtin_inf();
            }
            if (b < 0 || b >= nb) continue;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const double d = y_s[c * R + j] - yi[j];
                sf[j] = __builtin_fma(d, d, sf[j]);
                if (ALL) {
                    const double p = ri[j] * r_s[c * R + j];
                    cf[j] = cf[j] + p;
                    cf2[j] = __builtin_fma(p, p, cf2[j]);
                    nz[j] = nz[j] + (vi[j] + v_s[c * R + j]);
                }
            }
            if (ALL) { lg = lg + tau; cnt += 1; }
        }
    }
    // the bin the row ended in, and zeros for the bins it never entered
    for (int bb = b < 0 ? 0 : b; bb < nb; ++bb) flush(bb);
}

struct MtgLagOut {
    int64_t *count;
    double *lag, *sf, *cf, *cf2, *noise;   // each NULL or [L][nbins] of the call
};

// one workgroup per (light curve of the slab, bin): the rows' partials into the call's outputs at l0
template <int R>
__global__ void __launch_bounds__(MTG_LAG_LANES)
mtg_lag_reduce_kernel(const MtgLagKernelArgs a, const MtgLagOut o)
{
    __shared__ double red[MTG_LAG_LANES];
    __shared__ int64_t ired[MTG_LAG_LANES];
    const int nb = a.nbins;
    const int64_t l = blockIdx.x / nb, b = blockIdx.x - l * nb;   // l: within the slab
    const int64_t lc = (l * nb + b) * a.N, tl = (l / R * nb + b) * a.N, at = (a.l0 + l) * nb + b;
    double *const outs[4] = {o.sf, o.cf, o.cf2, o.noise};
    for (int s = 0; s < 4; ++s) {
        if (!outs[s]) continue;
        const double v = lag_row_sum(lag_ws_lc(a, s) + lc, a.N, red);
        if (threadIdx.x == 0) outs[s][at] = v;
    }
    if (o.lag) {
        const double v = lag_row_sum(lag_ws_tile(a, R, 0) + tl, a.N, red);
        if (threadIdx.x == 0) o.lag[at] = v;
    }
    if (o.count) {
        const int64_t v = lag_row_sum(reinterpret_cast<const int64_t *>(lag_ws_tile(a, R, 1)) + tl, a.N, ired);
        if (threadIdx.x == 0) o.count[at] = v;
    }
}

template <int R>
hipError_t lag_launch(const MtgLagKernelArgs &g, const MtgLagOut &o, bool all, int64_t blocks, hipStream_t s)
{
    if (all) hipLaunchKernelGGL((mtg_lag_kernel<R, true>), dim3((unsigned)blocks), dim3(MTG_LAG_LANES), 0, s, g);
    else hipLaunchKernelGGL((mtg_lag_kernel<R, false>), dim3((unsigned)blocks), dim3(MTG_LAG_LANES), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mtg_lag_reduce_kernel<R>), dim3((unsigned)(g.Ls * g.nbins)), dim3(MTG_LAG_LANES), 0, s, g, o);
    return hipGetLastError();
}

}  // namespace

hipError_t mtg_launch_lag(const MtgLagArgs &q, const MtgLagPlan &plan, int64_t l0, int64_t Ls, hipStream_t s)
{
    const MtgLombScargleArgs &ls = q.ls;
    const int64_t blocks = mtg_lag_launch_blocks(plan, ls.N, ls.t_stride, ls.L, q.nbins, l0, Ls);
    if (blocks == 0 || ls.N < 2 || plan.per_lc != (plan.all ? 4 : 1) || plan.per_tile != (plan.all ? 2 : 0)) return hipErrorInvalidValue;
    MtgLagKernelArgs g;
    g.dxt = ls.dxt; g.yv = ls.yv; g.N = ls.N; g.t_stride = ls.t_stride; g.l0 = l0; g.Ls = Ls;
    g.stats = reinterpret_cast<const double4 *>(ls.stats);
    g.nbins = q.nbins; g.row_blocks = (int)plan.row_blocks; g.edges = q.edges; g.ws = q.ws;
    MtgLagOut o;
    o.count = q.count; o.lag = q.lag; o.sf = q.sf; o.cf = q.cf; o.cf2 = q.cf2; o.noise = q.noise;
    if (!plan.all && (o.count || o.lag || o.cf || o.cf2 || o.noise)) return hipErrorInvalidValue;
    switch (plan.tile) {
    case 1: return lag_launch<1>(g, o, plan.all, blocks, s);
    case 4: return lag_launch<4>(g, o, plan.all, blocks, s);
    case MTG_LAG_TILE: return lag_launch<MTG_LAG_TILE>(g, o, plan.all, blocks, s);
    default: return hipErrorInvalidValue;
    }
}
