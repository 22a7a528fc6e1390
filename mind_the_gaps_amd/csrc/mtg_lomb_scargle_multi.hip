// mtg_lomb_scargle_multi.hip -- the multi-harmonic Lomb-Scargle periodogram of every resident light curve
// (mtg_lomb_scargle_multi of include/mtg.h, nterms = K in 2 .. 5): astropy's LombScargle(fit_mean=True, center_data=True,
// nterms=K).power(method="chi2").
//
// With the weights w_n, ybar, r = y - ybar and YY of mtg_lomb_scargle.hip (its pre-pass serves) and
// phi_n = 2 pi f (t_n - t_0), the design row is x_n = (1, sin phi_n, cos phi_n, ..., sin K phi_n, cos K phi_n),
//   A = sum w x x^T,  b = sum w r x,  p = b^T A^-1 b.
// b_0 = sum w r = 0, so the bias column is eliminated beforehand: with h = sum w x (harmonic part) and A_hh the harmonic
// block, p = b_h^T (A_hh - h h^T)^-1 b_h -- the step CC = sum w c^2 - C^2 of the one-term kernel.  Products of two
// harmonics are half sums and differences of C_m = sum w cos m phi, S_m = sum w sin m phi, m = 0 .. 2 K (C_0 = sum w = 1,
// S_0 = 0): a lane carries 4 K trigonometric sums and, per light curve, the 2 K data sums sum w r sin m phi,
// sum w r cos m phi (m <= K).
//
// One lane owns a frequency; a workgroup walks the samples in chunks of MTG_LS_CHUNK staged in LDS.  The base pair
// (cos phi, sin phi) is mtg_cycles_sincos's, bit for bit the one-term kernel's; harmonic m follows from harmonic m - 1
// by one complex multiplication by that pair, m = 2 .. 2 K in this order.  On shared sampling a lane carries a tile of R
// light curves (mtg_ls_multi_plan.h: R per (K, weighted) such that two waves per SIMD need no scratch), so that pair and
// harmonics are computed once per tile -- and the trigonometric sums too when the weights are 1 / N.
//
// After the last chunk the 2 K x 2 K matrix is assembled and factored by an unrolled Cholesky in registers: once per
// (frequency, light curve) weighted, once per lane unweighted (the factor serves the tile).  A pivot that is not
// positive gives NaN.
//
// Order.  Samples ascending; the sums of a chunk start from zero and are added to the running totals at its end.  The
// arithmetic of one (light curve, frequency) is the same sequence of operations in every instantiation of a (K,
// weighted), so that a power depends on (light curve, frequency, K, normalization, weighted) alone: not on L, the tile,
// F, the order of the frequencies, or on how the sampling is stored.
#include "mtg_device.h"
#include "mtg_math.h"
#include "mtg_ls_phase.h"

namespace {

struct MtgLsMultiArgs {
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

// the trigonometric sums of a lane: c[m - 1] = sum w cos m phi, s[m - 1] = sum w sin m phi, m = 1 .. 2 K
template <int K>
struct LsHarm {
    double c[2 * K], s[2 * K];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int m = 0; m < 2 * K; ++m) c[m] = s[m] = 0.0;
    }
    __device__ __forceinline__ void fold(const LsHarm &o)
    {
#pragma unroll
        for (int m = 0; m < 2 * K; ++m) { c[m] += o.c[m]; s[m] += o.s[m]; }
    }
};

// the data sums of a light curve: c[m - 1] = sum w r cos m phi, s[m - 1] = sum w r sin m phi, m = 1 .. K
template <int K>
struct LsData {
    double c[K], s[K];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int m = 0; m < K; ++m) c[m] = s[m] = 0.0;
    }
    __device__ __forceinline__ void fold(const LsData &o)
    {
#pragma unroll
        for (int m = 0; m < K; ++m) { c[m] += o.c[m]; s[m] += o.s[m]; }
    }
};

// The lower Cholesky factor of M = A_hh - h h^T (order: sin phi, cos phi, sin 2 phi, cos 2 phi, ...), row-packed, with
// the reciprocals of its diagonal; ok = every pivot positive.
template <int K>
struct LsFactor {
    static constexpr int n = 2 * K;
    double l[n * (n + 1) / 2], rd[n];
    bool ok;

    // C_m and S_m for any integer m: C_0 = sum w = 1, S_0 = 0, C_-m = C_m, S_-m = -S_m
    static __device__ __forceinline__ double cm(const LsHarm<K> &g, int m) { return m == 0 ? 1.0 : g.c[(m < 0 ? -m : m) - 1]; }
    static __device__ __forceinline__ double sm(const LsHarm<K> &g, int m) { return m == 0 ? 0.0 : m < 0 ? -g.s[-m - 1] : g.s[m - 1]; }
    // entry (i, j) of M, i >= j: index 2 (a - 1) is sin a phi, 2 (a - 1) + 1 is cos a phi
    static __device__ __forceinline__ double entry(const LsHarm<K> &g, int i, int j)
    {
#pragma clang fp contract(off)
        const int a = i / 2 + 1, b = j / 2 + 1;
        const bool ci = i & 1, cj = j & 1;
        const double hi = ci ? g.c[a - 1] : g.s[a - 1], hj = cj ? g.c[b - 1] : g.s[b - 1];
        double e;
        if (!ci && !cj) e = 0.5 * (cm(g, a - b) - cm(g, a + b));        // sin a phi sin b phi
        else if (ci && cj) e = 0.5 * (cm(g, a - b) + cm(g, a + b));     // cos a phi cos b phi
        else if (!ci) e = 0.5 * (sm(g, a + b) + sm(g, a - b));          // sin a phi cos b phi
        else e = 0.5 * (sm(g, a + b) + sm(g, b - a));                   // cos a phi sin b phi
        return e - hi * hj;
    }
    __device__ __forceinline__ void factor(const LsHarm<K> &g)
    {
#pragma clang fp contract(off)
        ok = true;
#pragma unroll
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double v = entry(g, i, j);
#pragma unroll
                for (int k = 0; k < j; ++k) v = __builtin_fma(-l[i * (i + 1) / 2 + k], l[j * (j + 1) / 2 + k], v);
                if (j < i) {
                    l[i * (i + 1) / 2 + j] = v * rd[j];
                } else {
                    ok = ok && v > 0.0;
                    const double d = sqrt(v);
                    l[i * (i + 1) / 2 + i] = d;
                    rd[i] = 1.0 / d;
                }
            }
        }
    }
    // b^T M^-1 b = |z|^2 with L z = b, b = (YS_1, YC_1, YS_2, YC_2, ...)
    __device__ __forceinline__ double quad(const LsData<K> &y) const
    {
#pragma clang fp contract(off)
        double z[n], p = 0.0;
#pragma unroll
        for (int i = 0; i < n; ++i) {
            double v = (i & 1) ? y.c[i / 2] : y.s[i / 2];
#pragma unroll
            for (int k = 0; k < i; ++k) v = __builtin_fma(-l[i * (i + 1) / 2 + k], z[k], v);
            z[i] = v * rd[i];
            p = __builtin_fma(z[i], z[i], p);
        }
        return p;
    }
};

// K harmonics, R light curves per lane; WEIGHTED: weights from the light curve's own sigma (its trigonometric sums are
// its own), else 1 / N (they are the tile's).  LDS chunk as in mtg_lomb_scargle_kernel: te[CHUNK], then WEIGHTED
// (w, w r)[R][CHUNK], else w r as pairs of light curves (2j, 2j + 1)[R / 2][CHUNK] (R = 1: [CHUNK] doubles).
template <int K, int R, bool WEIGHTED>
__global__ void __launch_bounds__(MTG_LS_THREADS, 2)
mtg_lomb_scargle_multi_kernel(const MtgLsMultiArgs a)
{
#pragma clang fp contract(off)
    static_assert(WEIGHTED || R == 1 || R % 2 == 0, "the unweighted chunk is staged as pairs of light curves");
    constexpr int CH = MTG_LS_CHUNK;
    constexpr int NT = WEIGHTED ? R : 1;               // sets of trigonometric sums kept per lane
    constexpr int NP = WEIGHTED ? R : (R + 1) / 2;     // 16-byte (R = 1 unweighted: 8-byte) columns of the chunk
    __shared__ MtgLsTab tab;
    __shared__ double te_s[CH];
    __shared__ double2 col_s[NP * CH];

    const int tid = threadIdx.x, nth = blockDim.x;
    mtg_ls_fill_tab(&tab);
    const int64_t tile = blockIdx.x / a.nfb;
    const int fb = (int)(blockIdx.x - tile * a.nfb);
    const int64_t lt = a.l0 + tile * R;                 // first light curve of the tile
    const int nl = (int)(a.l0 + a.Ls - lt < R ? a.l0 + a.Ls - lt : R);   // light curves in it
    const int64_t k = (int64_t)fb * nth + tid;
    const double f = a.freqs[k < a.F ? k : a.F - 1];    // (idle lanes repeat the last frequency and store nothing)
    const double2 *dxt = a.dxt + lt * a.t_stride;
    const double t0 = dxt[0].y;
    const double w0 = 1.0 / (double)a.N;

    LsHarm<K> tt[NT];
    LsData<K> ty[R];
#pragma unroll
    for (int i = 0; i < NT; ++i) tt[i].zero();
#pragma unroll
    for (int i = 0; i < R; ++i) ty[i].zero();

    for (int64_t n0 = 0; n0 < a.N; n0 += CH) {
        const int len = (int)(a.N - n0 < CH ? a.N - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: nothing)
        for (int i = tid; i < len; i += nth) te_s[i] = dxt[n0 + i].y - t0;
        if (WEIGHTED) {
            for (int e = tid; e < R * CH; e += nth) {
                const int j = e / CH, i = e - j * CH;
                if (i >= len) continue;
                double2 o = make_double2(0.0, 0.0);    // a light curve beyond the tile adds zeros and is not stored
                if (j < nl) {
                    const double4 st = a.stats[lt + j];
                    const double2 v = a.yv[(lt + j) * a.N + n0 + i];
                    const double w = (1.0 / v.y) / st.z;
                    o = make_double2(w, w * (v.x - st.x));
                }
                col_s[j * CH + i] = o;
            }
        } else if (R == 1) {
            const double ybar = a.stats[lt].x;
            double *col = reinterpret_cast<double *>(col_s);
            for (int i = tid; i < len; i += nth) col[i] = w0 * (a.yv[lt * a.N + n0 + i].x - ybar);
        } else {
            for (int e = tid; e < NP * CH; e += nth) {
                const int j = e / CH, i = e - j * CH;
                if (i >= len) continue;
                double2 o = make_double2(0.0, 0.0);
                if (2 * j < nl) o.x = w0 * (a.yv[(lt + 2 * j) * a.N + n0 + i].x - a.stats[lt + 2 * j].x);
                if (2 * j + 1 < nl) o.y = w0 * (a.yv[(lt + 2 * j + 1) * a.N + n0 + i].x - a.stats[lt + 2 * j + 1].x);
                col_s[j * CH + i] = o;
            }
        }
        __syncthreads();

        LsHarm<K> pt[NT];
        LsData<K> py[R];
#pragma unroll
        for (int i = 0; i < NT; ++i) pt[i].zero();
#pragma unroll
        for (int i = 0; i < R; ++i) py[i].zero();
        for (int i = 0; i < len; ++i) {
            double s1, c1;
            mtg_cycles_sincos(f, te_s[i], &s1, &c1, &tab);
            // the chunk's operands: w per set of trigonometric sums, w r per light curve
            double wt[NT], wr[R];
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
            double cm = c1, sm = s1;
#pragma unroll
            for (int m = 0; m < 2 * K; ++m) {
                if (m > 0) {   // (cos, sin)((m + 1) phi) = (cos, sin)(m phi) x (cos, sin)(phi)
                    const double cn = __builtin_fma(cm, c1, -(sm * s1));
                    const double sn = __builtin_fma(sm, c1, cm * s1);
                    cm = cn;
                    sm = sn;
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    pt[j].c[m] = __builtin_fma(wt[j], cm, pt[j].c[m]);
                    pt[j].s[m] = __builtin_fma(wt[j], sm, pt[j].s[m]);
                }
                if (m < K) {
#pragma unroll
                    for (int j = 0; j < R; ++j) {
                        py[j].c[m] = __builtin_fma(wr[j], cm, py[j].c[m]);
                        py[j].s[m] = __builtin_fma(wr[j], sm, py[j].s[m]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) tt[i].fold(pt[i]);
#pragma unroll
        for (int i = 0; i < R; ++i) ty[i].fold(py[i]);
    }

    if (k >= a.F) return;
    LsFactor<K> fac;
    if (!WEIGHTED) fac.factor(tt[0]);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= nl) continue;
        if (WEIGHTED) fac.factor(tt[j]);
        const double4 st = a.stats[lt + j];
        const double YY = st.y;
        double out = __builtin_nan("");
        if (fac.ok) {
            const double p = fac.quad(ty[j]);
            switch (a.normalization) {
            case MTG_LS_STANDARD: out = p / YY; break;
            case MTG_LS_MODEL: out = p / (YY - p); break;
            case MTG_LS_LOG: out = -log(1.0 - p / YY); break;
            default: out = p * (0.5 * st.z); break;   // MTG_LS_PSD
            }
        }
        a.power[(lt - a.l0 + j) * a.F + k] = out;
    }
}

template <int K, int R, bool WEIGHTED>
void lsm_launch(const MtgLsMultiArgs &a, int64_t blocks, int threads, hipStream_t s)
{
    hipLaunchKernelGGL((mtg_lomb_scargle_multi_kernel<K, R, WEIGHTED>), dim3((unsigned)blocks), dim3(threads), 0, s, a);
}

// the two tiles of a (K, weighted): 1 and the full one of mtg_ls_multi_plan.h
template <int K>
void lsm_dispatch(const MtgLsMultiArgs &a, int R, int weighted, int64_t blocks, int threads, hipStream_t s)
{
    constexpr int RW = mtg_ls_multi_full_tile(K, 1), RU = mtg_ls_multi_full_tile(K, 0);
    if (weighted) {
        if (R == 1) lsm_launch<K, 1, true>(a, blocks, threads, s);
        else lsm_launch<K, RW, true>(a, blocks, threads, s);
    } else {
        if (R == 1) lsm_launch<K, 1, false>(a, blocks, threads, s);
        else lsm_launch<K, RU, false>(a, blocks, threads, s);
    }
}

}  // namespace

int mtg_launch_lomb_scargle_multi_powers(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, hipStream_t s)
{
    const int R = mtg_ls_multi_tile(q.nterms, q.L, q.t_stride == 0, q.weighted);
    if (R < 1) return 0;
    // narrow frequency lists leave most of a wide workgroup idle: one or two waves then (the arithmetic of a lane is the same)
    const int threads = q.F <= 64 ? 64 : q.F <= 128 ? 128 : MTG_LS_THREADS;
    const int64_t nfb = (q.F + threads - 1) / threads, tiles = (Ls + R - 1) / R;
    if (nfb > 0x7fffffff / tiles) return 0;
    MtgLsMultiArgs a;
    a.dxt = q.dxt; a.yv = q.yv; a.N = q.N; a.t_stride = q.t_stride; a.l0 = l0; a.Ls = Ls;
    a.stats = reinterpret_cast<const double4 *>(q.stats); a.F = q.F; a.freqs = q.freqs; a.nfb = (int)nfb;
    a.normalization = q.normalization; a.power = q.power;
    const int64_t blocks = nfb * tiles;
    switch (q.nterms) {
    case 2: lsm_dispatch<2>(a, R, q.weighted, blocks, threads, s); break;
    case 3: lsm_dispatch<3>(a, R, q.weighted, blocks, threads, s); break;
    case 4: lsm_dispatch<4>(a, R, q.weighted, blocks, threads, s); break;
    case 5: lsm_dispatch<5>(a, R, q.weighted, blocks, threads, s); break;
    default: return 0;
    }
    return 1;
}
