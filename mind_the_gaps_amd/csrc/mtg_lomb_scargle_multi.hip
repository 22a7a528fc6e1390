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
// The sweep over tiles of light curves, chunks of samples and frequencies, its LDS budget and its order of summation
// are mtg_ls_tile.h's, the one-term kernel's too; LsHarmonics<K> below is this unit's model.  The base pair
// (cos phi, sin phi) is mtg_cycles_sincos's, bit for bit the one-term kernel's; harmonic m follows from harmonic m - 1
// by one complex multiplication by that pair, m = 2 .. 2 K in this order.  The tile of R light curves per lane is
// mtg_ls_plan.h's: R per (K, weighted) such that two waves per SIMD need no scratch.
//
// After the last chunk the 2 K x 2 K matrix is assembled and factored by an unrolled Cholesky in registers: once per
// (frequency, light curve) weighted, once per lane unweighted (the factor serves the tile).  A pivot that is not
// positive gives NaN.
#include "mtg_ls_tile.h"

namespace {

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

// K phase-tied harmonics with a floating mean
template <int K>
struct LsHarmonics {
    typedef LsHarm<K> Trig;
    typedef LsData<K> Data;
    template <int NT, int R>
    static __device__ __forceinline__ void accumulate(double c1, double s1, const double (&wt)[NT], const double (&wr)[R], Trig (&pt)[NT],
                                                      Data (&py)[R])
    {
#pragma clang fp contract(off)
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
    struct Solve {
        LsFactor<K> fac;
        __device__ __forceinline__ void prepare(const Trig &g) { fac.factor(g); }
        __device__ __forceinline__ bool solve(const Data &y, double *p) const
        {
            if (!fac.ok) return false;
            *p = fac.quad(y);
            return true;
        }
    };
};

// K harmonics, R light curves per lane; WEIGHTED: weights from the light curve's own sigma (its trigonometric sums are
// its own), else 1 / N (they are the tile's)
template <int K, int R, bool WEIGHTED>
__global__ void __launch_bounds__(MTG_LS_THREADS, 2)
mtg_lomb_scargle_multi_kernel(const MtgLsArgs a)
{
    ls_tile_sweep<LsHarmonics<K>, R, WEIGHTED>(a);
}

template <int K, int R, bool WEIGHTED>
void lsm_launch(const MtgLsLaunch &g, hipStream_t s)
{
    hipLaunchKernelGGL((mtg_lomb_scargle_multi_kernel<K, R, WEIGHTED>), dim3((unsigned)g.blocks), dim3(g.threads), 0, s, g.a);
}

// the two tiles of a (K, weighted): 1 and the full one of mtg_ls_plan.h
template <int K>
void lsm_dispatch(const MtgLsLaunch &g, int R, int weighted, hipStream_t s)
{
    constexpr int RW = mtg_ls_full_tile(K, 1), RU = mtg_ls_full_tile(K, 0);
    if (weighted) {
        if (R == 1) lsm_launch<K, 1, true>(g, s);
        else lsm_launch<K, RW, true>(g, s);
    } else {
        if (R == 1) lsm_launch<K, 1, false>(g, s);
        else lsm_launch<K, RU, false>(g, s);
    }
}

}  // namespace

int mtg_launch_lomb_scargle_multi_powers(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, hipStream_t s)
{
    const int R = mtg_ls_tile(q.nterms, q.L, q.t_stride == 0, q.weighted);
    MtgLsLaunch g;
    if (R < 1 || !mtg_ls_plan_launch(q, R, l0, Ls, &g)) return 0;
    switch (q.nterms) {
    case 2: lsm_dispatch<2>(g, R, q.weighted, s); break;
    case 3: lsm_dispatch<3>(g, R, q.weighted, s); break;
    case 4: lsm_dispatch<4>(g, R, q.weighted, s); break;
    case 5: lsm_dispatch<5>(g, R, q.weighted, s); break;
    default: return 0;   // (one term: mtg_lomb_scargle.hip)
    }
    return 1;
}
