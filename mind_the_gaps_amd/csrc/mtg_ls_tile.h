// mtg_ls_tile.h -- the tile sweep of the Lomb-Scargle kernels, written once for one term (mtg_lomb_scargle.hip) and
// K harmonics (mtg_lomb_scargle_multi.hip).  A model says what a lane accumulates per sample and how the sums become
// the power p; everything with an edge is here: the ragged last chunk, the partly filled tile, a slab that starts at
// l0 > 0, idle lanes, and the launch geometry.  The pieces -- mtg_ls_args, LsLane, ls_stage_chunk, ls_read_sample --
// also serve the two sweeps that keep other sums per lane and so have a chunk loop of their own: mtg_epoch_fold.hip
// (time origin q.t0 = time_0) and mtg_wwz.hip (a third grid factor, q.t0 = tau, and its own column rule).
//
// One lane owns a frequency; a workgroup walks the samples in chunks of MTG_LS_CHUNK staged in LDS, every lane reading
// the same sample (a broadcast).  On shared sampling a lane carries the sums of a tile of R light curves
// (mtg_ls_plan.h), so that the (cos, sin) pair -- and the trigonometric sums too when the weights are 1 / N -- is
// computed once per tile.
//
// A model M has
//   M::Trig, M::Data   a lane's trigonometric sums (one set per light curve weighted, one per tile otherwise) and a light
//                      curve's data sums, each with zero() and fold(other);
//   M::accumulate      one sample: (cos, sin), the weights wt[NT] and the weighted residuals wr[R] into the chunk's sums;
//   M::Solve           prepare(Trig) -- once per lane unweighted, once per light curve weighted -- then solve(Data, &p):
//                      false where the system is not positive definite (the power is NaN).
//
// LDS: the 32 KiB (cos, sin) table, the chunk's elapsed times (2 KiB) and its columns, WEIGHTED (w, w r)[R][CHUNK]
// (R x 4 KiB), else w r as pairs of light curves (2j, 2j + 1)[R / 2][CHUNK] (R x 2 KiB; R = 1: [CHUNK] doubles) -- one
// ds_read_b128 per two sums either way.  At most 66 KiB (one term, R = 8 weighted / R = 16 unweighted): two workgroups
// of four waves on a CU's 160 KiB, two waves per SIMD.
//
// Order.  Samples ascending; the sums of a chunk start from zero and are added to the running totals at its end.  The
// arithmetic of one (light curve, frequency) is the same sequence of operations in every instantiation of a model, so
// that a power depends on (light curve, frequency, model, normalization, weighted) alone: not on L, the tile, F, the
// order of the frequencies, or on how the sampling is stored.
#ifndef MTG_LS_TILE_H
#define MTG_LS_TILE_H

#include "mtg_device.h"
#include "mtg_math.h"
#include "mtg_ls_phase.h"
#include "mtg_ls_plan.h"

struct MtgLsArgs {
    const double2 *dxt, *yv;
    int64_t N, t_stride;     // 0 (shared sampling) or N
    int64_t l0, Ls;          // this launch takes light curves [l0, l0 + Ls)
    const double4 *stats;    // [L]: ybar, YY, sum sigma^-2 (or N), 0 -- mtg_lomb_scargle_stats_kernel's
    int64_t F;
    const double *freqs;     // [F]
    int nfb;                 // workgroups along the frequencies
    int normalization;
    double *power;           // [Ls][F] of this slab
};

// the arguments of one slab's launch from the call's: light curves [l0, l0 + Ls), nfb workgroups along the frequencies
static inline MtgLsArgs mtg_ls_args(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, int64_t nfb)
{
    MtgLsArgs a;
    a.dxt = q.dxt; a.yv = q.yv; a.N = q.N; a.t_stride = q.t_stride; a.l0 = l0; a.Ls = Ls;
    a.stats = reinterpret_cast<const double4 *>(q.stats); a.F = q.F; a.freqs = q.freqs; a.nfb = (int)nfb;
    a.normalization = q.normalization; a.power = q.power;
    return a;
}

// The launch of one slab with R light curves per lane: false = more workgroups than a grid holds.  Narrow frequency
// lists leave most of a wide workgroup idle: one or two waves then (the arithmetic of a lane is the same).
struct MtgLsLaunch {
    int64_t blocks;
    int threads;
    MtgLsArgs a;
};
static inline bool mtg_ls_plan_launch(const MtgLombScargleArgs &q, int R, int64_t l0, int64_t Ls, MtgLsLaunch *g)
{
    g->threads = q.F <= 64 ? 64 : q.F <= 128 ? 128 : MTG_LS_THREADS;
    const int64_t nfb = (q.F + g->threads - 1) / g->threads, tiles = (Ls + R - 1) / R;
    if (nfb > 0x7fffffff / tiles) return false;
    g->blocks = nfb * tiles;
    g->a = mtg_ls_args(q, l0, Ls, nfb);
    return true;
}

// what a lane knows of its tile and its frequency
struct LsLane {
    int64_t lt;            // first light curve of the tile
    int nl;                // light curves in it
    int64_t k;             // the lane's frequency (idle lanes, k >= F, repeat the last one and store nothing)
    double f;
    const double2 *dxt;    // the tile's sampling
    double t0, w0;         // the origin of the elapsed times: its first time, unless the kernel sets another; 1 / N
    template <int R>
    __device__ __forceinline__ void locate(const MtgLsArgs &a, int64_t tile, int fb)
    {
        lt = a.l0 + tile * R;
        nl = (int)(a.l0 + a.Ls - lt < R ? a.l0 + a.Ls - lt : R);
        k = (int64_t)fb * blockDim.x + threadIdx.x;
        f = a.freqs[k < a.F ? k : a.F - 1];
        dxt = a.dxt + lt * a.t_stride;
        t0 = dxt[0].y;
        w0 = 1.0 / (double)a.N;
    }
    // a grid of frequency blocks, fastest, and tiles
    template <int R>
    __device__ __forceinline__ void locate(const MtgLsArgs &a)
    {
        const int64_t tile = blockIdx.x / a.nfb;
        locate<R>(a, tile, (int)(blockIdx.x - tile * a.nfb));
    }
};

// What a column of the chunk holds, from a sample's weight and residual: (w, w r) per light curve, and w0 r where the
// weights are 1 / N.  (mtg_wwz.hip, whose weight gets a factor per lane, has a rule of its own.)
struct LsColumns {
    static __device__ __forceinline__ double2 weighted(double w, double r) { return make_double2(w, w * r); }
    static __device__ __forceinline__ double plain(double w0, double r) { return w0 * r; }
};

// samples [n0, n0 + len) of the tile into LDS, elapsed from q.t0; a light curve beyond the tile adds zeros and is not stored
template <int R, bool WEIGHTED, class C = LsColumns>
__device__ __forceinline__ void ls_stage_chunk(const MtgLsArgs &a, const LsLane &q, int64_t n0, int len, double *te_s, double2 *col_s)
{
#pragma clang fp contract(off)
    constexpr int CH = MTG_LS_CHUNK;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int64_t lt = q.lt;
    for (int i = tid; i < len; i += nth) te_s[i] = q.dxt[n0 + i].y - q.t0;
    if (WEIGHTED) {
        for (int e = tid; e < R * CH; e += nth) {
            const int j = e / CH, i = e - j * CH;
            if (i >= len) continue;
            double2 o = make_double2(0.0, 0.0);
            if (j < q.nl) {
                const double4 st = a.stats[lt + j];
                const double2 v = a.yv[(lt + j) * a.N + n0 + i];
                o = C::weighted((1.0 / v.y) / st.z, v.x - st.x);
            }
            col_s[j * CH + i] = o;
        }
    } else if (R == 1) {
        const double ybar = a.stats[lt].x;
        double *col = reinterpret_cast<double *>(col_s);
        for (int i = tid; i < len; i += nth) col[i] = C::plain(q.w0, a.yv[lt * a.N + n0 + i].x - ybar);
    } else {
        for (int e = tid; e < (R + 1) / 2 * CH; e += nth) {
            const int j = e / CH, i = e - j * CH;
            if (i >= len) continue;
            double2 o = make_double2(0.0, 0.0);
            if (2 * j < q.nl) o.x = C::plain(q.w0, a.yv[(lt + 2 * j) * a.N + n0 + i].x - a.stats[lt + 2 * j].x);
            if (2 * j + 1 < q.nl) o.y = C::plain(q.w0, a.yv[(lt + 2 * j + 1) * a.N + n0 + i].x - a.stats[lt + 2 * j + 1].x);
            col_s[j * CH + i] = o;
        }
    }
}

// sample i of the chunk: w per set of trigonometric sums, w r per light curve
template <int R, bool WEIGHTED>
__device__ __forceinline__ void ls_read_sample(const double2 *col_s, int i, double w0, double (&wt)[WEIGHTED ? R : 1], double (&wr)[R])
{
    constexpr int CH = MTG_LS_CHUNK;
    if (WEIGHTED) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const double2 v = col_s[j * CH + i];
            wt[j] = v.x;
            wr[j] = v.y;
        }
    } else {
        wt[0] = w0;
        if (R == 1) {
            wr[0] = reinterpret_cast<const double *>(col_s)[i];
        } else {
#pragma unroll
            for (int j = 0; j < R / 2; ++j) {
                const double2 v = col_s[j * CH + i];
                wr[2 * j] = v.x;
                wr[2 * j + 1] = v.y;
            }
        }
    }
}

// the power in its normalisation: p = YY - chi^2 of the model, YY and sw = sum sigma^-2 (or N) the pre-pass's
__device__ __forceinline__ double ls_normalize(double p, double YY, double sw, int normalization)
{
#pragma clang fp contract(off)
    switch (normalization) {
    case MTG_LS_STANDARD: return p / YY;
    case MTG_LS_MODEL: return p / (YY - p);
    case MTG_LS_LOG: return -log(1.0 - p / YY);
    default: return p * (0.5 * sw);   // MTG_LS_PSD
    }
}

// The sweep: the body of a kernel of MTG_LS_THREADS lanes at most, two workgroups per CU.
template <class M, int R, bool WEIGHTED>
__device__ __forceinline__ void ls_tile_sweep(const MtgLsArgs &a)
{
#pragma clang fp contract(off)
    static_assert(WEIGHTED || R == 1 || R % 2 == 0, "the unweighted chunk is staged as pairs of light curves");
    constexpr int CH = MTG_LS_CHUNK;
    constexpr int NT = WEIGHTED ? R : 1;               // sets of trigonometric sums kept per lane
    constexpr int NP = WEIGHTED ? R : (R + 1) / 2;     // 16-byte (R = 1 unweighted: 8-byte) columns of the chunk
    __shared__ MtgLsTab tab;
    __shared__ double te_s[CH];
    __shared__ double2 col_s[NP * CH];

    mtg_ls_fill_tab(&tab);
    LsLane q;
    q.locate<R>(a);

    typename M::Trig tt[NT];
    typename M::Data ty[R];
#pragma unroll
    for (int i = 0; i < NT; ++i) tt[i].zero();
#pragma unroll
    for (int i = 0; i < R; ++i) ty[i].zero();

    for (int64_t n0 = 0; n0 < a.N; n0 += CH) {
        const int len = (int)(a.N - n0 < CH ? a.N - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: nothing)
        ls_stage_chunk<R, WEIGHTED>(a, q, n0, len, te_s, col_s);
        __syncthreads();

        typename M::Trig pt[NT];
        typename M::Data py[R];
#pragma unroll
        for (int i = 0; i < NT; ++i) pt[i].zero();
#pragma unroll
        for (int i = 0; i < R; ++i) py[i].zero();
        for (int i = 0; i < len; ++i) {
            double si, co, wt[NT], wr[R];
            mtg_cycles_sincos(q.f, te_s[i], &si, &co, &tab);
            ls_read_sample<R, WEIGHTED>(col_s, i, q.w0, wt, wr);
            M::template accumulate<NT, R>(co, si, wt, wr, pt, py);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) tt[i].fold(pt[i]);
#pragma unroll
        for (int i = 0; i < R; ++i) ty[i].fold(py[i]);
    }

    if (q.k >= a.F) return;
    typename M::Solve sv;
    if (!WEIGHTED) sv.prepare(tt[0]);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= q.nl) continue;
        if (WEIGHTED) sv.prepare(tt[j]);
        const double4 st = a.stats[q.lt + j];
        double p;
        a.power[(q.lt - a.l0 + j) * a.F + q.k] = sv.solve(ty[j], &p) ? ls_normalize(p, st.y, st.z, a.normalization) : __builtin_nan("");
    }
}

#endif
