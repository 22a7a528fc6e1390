// mtg_predict_at.hip -- conditional mean / variance at NEW times from the semiseparable factorisation
// (celerite.GP.predict(y, t=ts, return_var=True)), in O((N + M C) J^2) per parameter vector and with no object of
// size N x M anywhere: celerite, and this project until now, form the dense cross-covariance K_* [M][N].
//
// Notation of mtg_predict_kernel (mtg_sampler.hip; W normalised by D):
//   forward    S_n = phi_n phi_n^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),  f_n = phi_n o (f_{n-1} + W_{n-1} z_{n-1})
//              W_n = (V_n - S_n U_n) / D_n,  D_n = d_n + k(0) - U_n^T S_n U_n,  z_n = r_n - U_n^T f_n
//   backward   g_n = phi_{n+1} o (g_{n+1} + U_{n+1} x_{n+1}),  x_n = z_n / D_n - W_n^T g_n            (x = K^-1 r)
//              G_n = U_n U_n^T / D_n + (I - U_n W_n^T) X_n (I - W_n U_n^T),  X_n = phi_{n+1} phi_{n+1}^T o G_{n+1}
// For a new time t* with n0 the last sample at or before it (-1: before the first one):
//   phi* = exp(-c (t* - t_n0)),     S* = phi* phi*^T o (S_n0 + D_n0 W_n0 W_n0^T),  f* = phi* o (f_n0 + W_n0 z_n0)
//   psi  = exp(-c (t_{n0+1} - t*)), X* = psi psi^T o G_{n0+1},                     g* = psi o (g_{n0+1} + U_{n0+1} x_{n0+1})
//   q = S* U*,  Wt = V* - q        (U*, V* the generators at t*; S*, f* = 0 for n0 = -1; X*, g* = 0 for n0 = N - 1)
//   mu*  = mean(t*) + U*^T f* + Wt^T g*
//   var* = k(0) - U*^T q - Wt^T X* Wt
// k_*^T K^-1 b = sum_n z*_n z^b_n / D_n with z* = L^-1 k_*: up to n0 the row k_* continues the lower triangle, which
// sums to U*^T S* U* and U*^T f*; beyond n0 the forward substitution's error vector starts at Wt and is carried by
// phi o (I - W U^T), which is what G and g accumulate from the other end.  The factors are those of the unchanged K.
// tests/predict_at_replay.py is the same in numpy.
//
// Two stages:
//   mtg_predict_at_factor_kernel   one lane per parameter vector (as mtg_predict_kernel): both sweeps, leaving U, W, phi,
//                                  D, z, x of every sample in the workspace and a checkpoint of (S, f) and of (G, g) at
//                                  every MTG_PAT_C-th sample (symmetric: J (J + 1) / 2 + J doubles each); a third sweep,
//                                  of the time-reversed series, for the variance before the first sample
//   mtg_predict_at_eval_kernel     one lane per (parameter vector, new time): binary search of t* among the light curve's
//                                  times, at most MTG_PAT_C stored steps replayed forward from the checkpoint at or
//                                  before n0 and backward from the one at or after n0 + 1 (no transcendental in the
//                                  replay), then the exp / sincos of the two partial steps and the J^2 combinations.
// Lanes of a wave work on one parameter vector and, the times being handed over in ascending order, on neighbouring
// t*: they replay the same stored rows, which the vector memory path serves as one broadcast access.
// Both are templates on J so that S, G and the generators live in registers (no scratch; the generic-J
// mtg_predict_kernel spills by design).  The replay (mtg_pat_replay.h, shared with mtg_predict_terms.hip) uses the very
// step functions of the factorisation, so the S and G it rebuilds are bit for bit those the stored W, D, x were made from; each (row, t*) is a lane of its own, so its
// result does not depend on the batch, on M or on the order of ts.
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"
#include "mtg_pat_replay.h"
// DATA: row r of a.data stands in for the light curve's y (the conditional draw conditions on y - y~, mtg_gp_cond_draw.hip)
template <int J, bool DATA>
__global__ void __launch_bounds__(64) mtg_predict_at_factor_kernel(MtgPredictAtArgs a)
{
#pragma clang fp contract(off)
    constexpr int SY = J * (J + 1) / 2, CK = SY + J, stride = 3 * J + 3;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // row of this slab
    if (r >= a.B) return;
    const int64_t e = a.row0 + r;                                       // row of the batch
    if (a.status[e] != MTG_ST_OK) return;
    PatCoef<J> k;
    pat_load_coef<J>(a, e, k);
    const int64_t lc = a.lc_index ? a.lc_index[e] : 0;
    const int64_t N = a.N;
    const double2 *yv = a.yv + lc * N, *dxt = a.dxt + lc * a.t_stride;
    double *wk = a.work + r * N * stride;
    double *ckf = a.ckf + r * a.nck * CK, *ckb = a.ckb + r * a.nck * CK;

    double S[SY], f[J], Wp[J], U[J], V[J], ph[J];
    const double t_first = dxt[0].y;
#pragma unroll
    for (int i = 0; i < SY; ++i) S[i] = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) { f[i] = 0.0; Wp[i] = 0.0; }
    double Dp = 1.0, zp = 0.0;
    bool bad = false;
    for (int64_t n = 0; n < N; ++n) {
        const double dx = dxt[n].x, t = dxt[n].y;
        pat_decay<J>(k, dx, ph);
        pat_generators<J>(k, t, t_first, U, V);
        pat_fwd_step<J>(S, f, ph, Wp, Dp, zp);
        if (n % MTG_PAT_C == 0) {
            double *c = ckf + (n / MTG_PAT_C) * CK;
#pragma unroll
            for (int i = 0; i < SY; ++i) c[i] = S[i];
#pragma unroll
            for (int i = 0; i < J; ++i) c[SY + i] = f[i];
        }
        double yn;
        if constexpr (DATA) yn = a.data[r * N + n]; else yn = yv[n].x;
        double D = yv[n].y + k.asum, z = yn - (k.slope * t + k.icpt);
        double Wn[J];
#pragma unroll
        for (int i = 0; i < J; ++i) z -= U[i] * f[i];
        pat_pivot<J>(S, U, V, Wn, D);
        bad = bad || !(D > 0.0);
        double *w = wk + n * stride;
#pragma unroll
        for (int i = 0; i < J; ++i) { Wn[i] /= D; w[i] = U[i]; w[J + i] = Wn[i]; w[2 * J + i] = ph[i]; Wp[i] = Wn[i]; }
        w[3 * J] = D; w[3 * J + 1] = z;
        Dp = D; zp = z;
    }
    if (bad) { a.status[e] = MTG_ST_NOTPD; return; }

    double g[J], Un[J], phn[J];
    double *G = S;
#pragma unroll
    for (int i = 0; i < SY; ++i) G[i] = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) { g[i] = 0.0; Un[i] = 0.0; phn[i] = 0.0; }
    double xn = 0.0;
    for (int64_t n = N - 1; n >= 0; --n) {
        double *w = wk + n * stride;
        double Wn[J];
#pragma unroll
        for (int i = 0; i < J; ++i) { U[i] = w[i]; Wn[i] = w[J + i]; }
        const double D = w[3 * J];
        pat_bwd_g<J>(g, phn, Un, xn);
        double x = w[3 * J + 1] / D;
#pragma unroll
        for (int i = 0; i < J; ++i) x -= Wn[i] * g[i];
        w[3 * J + 2] = x;
        if (a.want_var) pat_bwd_G<J>(G, phn, U, Wn, D);
        if (n % MTG_PAT_C == 0) {
            double *c = ckb + (n / MTG_PAT_C) * CK;
            if (a.want_var) {
#pragma unroll
                for (int i = 0; i < SY; ++i) c[i] = G[i];
            }
#pragma unroll
            for (int i = 0; i < J; ++i) c[SY + i] = g[i];
        }
#pragma unroll
        for (int i = 0; i < J; ++i) { Un[i] = U[i]; phn[i] = w[2 * J + i]; }
        xn = x;
    }
    if (!a.want_var) return;

    // ---- the factorisation of the time-reversed series, for the variance BEFORE the first sample ----------------
    // There Wt = V* meets G_0 unreduced: var* = k(0) - V*^T X* V* cancels from |G|, whose own recurrence subtracts, and
    // a long-memory kernel (k(0) / d ~ 1e9) is left with 2.5e-9 k(0) of error, 1400 times its bound.  Seen from the other
    // end the same time lies AFTER the last sample, where var* = k(0) - U*^T S* U* comes from the S recurrence, a sum of
    // positive terms.  One more forward sweep, last sample first, phases at the time elapsed from the last sample
    // backwards; kept: S + D W W^T after the first sample, J (J + 1) / 2 doubles per row.
    const double t_last = dxt[N - 1].y;
#pragma unroll
    for (int i = 0; i < SY; ++i) S[i] = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) { f[i] = 0.0; Wp[i] = 0.0; }
    Dp = 1.0;
    for (int64_t n = N - 1; n >= 0; --n) {
        const double dx = n < N - 1 ? dxt[n + 1].x : 0.0;
        pat_decay<J>(k, dx, ph);
        pat_generators<J>(k, t_last, dxt[n].y, U, V);
        pat_fwd_step<J>(S, f, ph, Wp, Dp, 0.0);
        double D = yv[n].y + k.asum;
        pat_pivot<J>(S, U, V, Wp, D);
#pragma unroll
        for (int i = 0; i < J; ++i) Wp[i] /= D;
        Dp = D;
    }
    double *c = a.ckr + r * SY;
#pragma unroll
    for (int i = 0; i < J; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) c[pat_sy(i, j)] = S[pat_sy(i, j)] + Dp * Wp[i] * Wp[j];
}

template <int J>
__global__ void __launch_bounds__(64) mtg_predict_at_eval_kernel(MtgPredictAtArgs a)
{
#pragma clang fp contract(off)
    constexpr int SY = J * (J + 1) / 2;
    int64_t r, m;
    if (!pat_row_time(a.B, a.M, r, m)) return;
    const int64_t e = a.row0 + r;
    const int64_t slot = a.order ? a.order[m] : m;     // the times are visited in ascending order, stored where they were given
    if (a.status[e] != MTG_ST_OK) {
        a.mu[r * a.M + slot] = NAN;
        if (a.want_var) a.var[r * a.M + slot] = NAN;
        return;
    }
    PatCoef<J> k;
    pat_load_coef<J>(a, e, k);
    const PatRow<J> w(a, r, e);
    const double ts = a.ts[slot];
    const int64_t n0 = pat_locate(w.dxt, w.N, ts);

    double Us[J], Wt[J], ph[J], T[SY], v[J];           // Wt: V* until q = S* U* is taken off it; T, v: (S*, f*), then (X*, g*)
    pat_generators<J>(k, ts, w.dxt[0].y, Us, Wt);
    double mu = k.slope * ts + k.icpt, var = k.k0;
    if (n0 >= 0) {
        pat_replay_fwd<J>(k, w, n0, ts, T, v);
        double uq, uf;
        pat_combine_before<J>(PatHeld<J>{T, v}, Us, Wt, uq, uf);
        mu += uf;
        var -= uq;
    }
    const bool use_G = a.want_var && n0 >= 0;      // before the first sample the variance comes from the reversed sweep
    if (n0 < w.N - 1) {
        pat_replay_bwd<J>(k, w, n0, ts, use_G, T, v, ph);
        mu += pat_combine_wg<J>(Wt, v);
        if (use_G) var -= pat_combine_quad<J>(ph, T, Wt);
    }
    if (a.want_var && n0 < 0) {
        double Ur[J];
        pat_reversed_at<J>(k, w, ts, ph, Ur);
        var -= pat_combine_quad<J>(ph, w.ckr, Ur);
    }
    a.mu[r * a.M + slot] = mu;
    if (a.want_var) a.var[r * a.M + slot] = var;
}

// a model without a celerite term (white noise only, J = 0): K is diagonal, the prediction is the mean and the
// noise-free variance is 0; one lane per row checks the pivots, one per (row, t*) writes
__global__ void __launch_bounds__(64) mtg_predict_at_white_factor_kernel(MtgPredictAtArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.B) return;
    const int64_t e = a.row0 + r;
    if (a.status[e] != MTG_ST_OK) return;
    const double2 *yv = a.yv + (a.lc_index ? a.lc_index[e] : 0) * a.N;
    const double asum = a.coef[a.lay.asum() * a.cstride + e];
    bool bad = false;
    for (int64_t n = 0; n < a.N; ++n) bad = bad || !(yv[n].y + asum > 0.0);
    if (bad) a.status[e] = MTG_ST_NOTPD;
}

__global__ void __launch_bounds__(64) mtg_predict_at_white_eval_kernel(MtgPredictAtArgs a)
{
#pragma clang fp contract(off)
    int64_t r, m;
    if (!pat_row_time(a.B, a.M, r, m)) return;
    const int64_t e = a.row0 + r;
    const bool ok = a.status[e] == MTG_ST_OK;
    const double slope = a.coef[a.lay.mean(0) * a.cstride + e], icpt = a.coef[a.lay.mean(1) * a.cstride + e];
    a.mu[r * a.M + m] = ok ? slope * a.ts[m] + icpt : NAN;
    if (a.want_var) a.var[r * a.M + m] = ok ? 0.0 : NAN;
}

template <int J>
struct PatFactorLaunch {
    static void launch(const MtgPredictAtArgs &a, hipStream_t s)
    {
        const dim3 rows((unsigned)((a.B + 63) / 64));
        if (a.data) hipLaunchKernelGGL((mtg_predict_at_factor_kernel<J, true>), rows, dim3(64), 0, s, a);
        else hipLaunchKernelGGL((mtg_predict_at_factor_kernel<J, false>), rows, dim3(64), 0, s, a);
    }
};

template <int J>
struct PatLaunch {
    static void launch(const MtgPredictAtArgs &a, hipStream_t s)
    {
        PatFactorLaunch<J>::launch(a, s);
        hipLaunchKernelGGL(mtg_predict_at_eval_kernel<J>, dim3((unsigned)(a.B * ((a.M + 63) / 64))), dim3(64), 0, s, a);
    }
};

// the first stage alone, for mtg_predict_terms.hip's evaluation: the same kernels as below
int mtg_launch_predict_at_factor(const MtgPredictAtArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J != 0) return pat_dispatch_rank<PatFactorLaunch>(J, a, s);
    hipLaunchKernelGGL(mtg_predict_at_white_factor_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
    return 1;
}

// both stages for rows [row0, row0 + B) of the batch; J = nr0 + 2 nc0 in 0 .. MTG_MAX_J (returns 0 otherwise)
int mtg_launch_predict_at(const MtgPredictAtArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J != 0) return pat_dispatch_rank<PatLaunch>(J, a, s);
    hipLaunchKernelGGL(mtg_predict_at_white_factor_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(mtg_predict_at_white_eval_kernel, dim3((unsigned)(a.B * ((a.M + 63) / 64))), dim3(64), 0, s, a);
    return 1;
}
