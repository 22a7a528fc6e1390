// mtg_loglike_grad.hip -- the log-likelihood and its exact gradient by the free parameters, in one forward sweep:
// one lane per (row e, free parameter p) carries the semiseparable factorisation and its directional derivative by
// theta[p] in registers.  No adjoint pass, no per-sample workspace; the cost grows with P (a lane repeats its row's
// primal), which is the price of the simplest form that is exact.
//
// Notation of mtg_gp_draw.hip (W normalised by D), tangents as mtg_factor_step_tangent.h carries them (rotated frame):
//   S_n = phi phi^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),   f_n = phi o (f_{n-1} + W_{n-1} z_{n-1})
//   D_n = sigma_n^2 + asum - U^T S U,   W_n = (V - S U) / D_n,   z_n = y_n - mean(t_n) - U^T f_n
//   lnL = -1/2 sum (z^2 / D + ln D) - N/2 ln 2 pi
//   dlnL / dtheta_p = -1/2 sum (2 z z' / D - z^2 D' / D^2 + D' / D),   z' = -(slope' t + icpt') - U~^T f - U^T f~
// tests/loglike_grad_replay.py is the same in numpy.
//
// Two kernels.  mtg_grad_tangent_kernel expands d coef[slot] / d theta[p] into dcoef[slot][e P + p] from the primal
// coefficients mtg_prepare_kernel has left in the workspace (mtg_prepare_tangent.h).  mtg_loglike_grad_kernel<J> is the
// sweep: 64-lane workgroups over the lanes l = e P + p, so that the lanes of a row are neighbours and read the same
// samples (one address per row: the loads of a wave touch as many cache lines as it holds rows).  A lane's arithmetic
// reads nothing of its neighbours: a row's bits do not depend on the batch it travels in, and every lane of a row
// forms the same primal, hence the same verdict on the pivots.  The lane p = 0 writes the row's lnL and status; the prior's
// verdict is read from a copy the sweep never writes (MtgGradArgs::verdict).
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"
#include "mtg_factor_step_tangent.h"
#include "mtg_prepare_tangent.h"

__global__ void __launch_bounds__(256) mtg_grad_tangent_kernel(MtgGradArgs a)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.P) return;
    const int64_t e = l / a.P;
    const int p = (int)(l - e * a.P);
    const int32_t st = a.status[e];
    if (p == 0) a.verdict[e] = st;                 // the sweep reads this copy and writes a.status: no word is both read and written there
    if (st != MTG_ST_OK) return;                   // a rejected row has no coefficients
    mtg_prepare_tangent_one(a.model, a.theta + e * a.P, a.coef + e, a.cstride, p, a.dcoef + l, a.dstride);
}

template <int J>
__global__ void __launch_bounds__(64) mtg_loglike_grad_kernel(MtgGradArgs a)
{
#pragma clang fp contract(off)
    constexpr int JA = J > 0 ? J : 1, SY = JA * (JA + 1) / 2;
    const int64_t l = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (l >= a.B * a.P) return;
    const int64_t e = l / a.P;
    const int p = (int)(l - e * a.P);
    if (a.verdict[e] != MTG_ST_OK) {
        a.grad[l] = NAN;
        return;
    }
    const int64_t N = a.N;
    const int64_t lc = a.lc_index ? a.lc_index[e] : 0;
    const double2 *yv = a.yv + lc * N, *dxt = a.dxt + lc * a.t_stride;
    const double *dcoef = a.dcoef + l;

    PatCoef<JA> k;
    PatCoefTangent<JA> dk;
    double asum, slope, icpt, dasum, dslope, dicpt;
    if constexpr (J > 0) {
        pat_load_coef<J>(a, e, k);
        pat_load_coef_tangent<J>(dcoef, a.dstride, a.lay, k.NR, dk);
        asum = k.asum; slope = k.slope; icpt = k.icpt;
        dasum = dk.asum; dslope = dk.slope; dicpt = dk.icpt;
    } else {                                       // a white model: the diagonal and the mean only
        asum = a.coef[a.lay.asum() * a.cstride + e];
        slope = a.coef[a.lay.mean(0) * a.cstride + e];
        icpt = a.coef[a.lay.mean(1) * a.cstride + e];
        dasum = dcoef[a.lay.asum() * a.dstride];
        dslope = dcoef[a.lay.mean(0) * a.dstride];
        dicpt = dcoef[a.lay.mean(1) * a.dstride];
    }
    double S[SY], f[JA], Wp[JA], dS[SY], df[JA], dWp[JA];
#pragma unroll
    for (int i = 0; i < SY; ++i) { S[i] = 0.0; dS[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < JA; ++i) { f[i] = 0.0; Wp[i] = 0.0; df[i] = 0.0; dWp[i] = 0.0; }
    const double t_first = dxt[0].y;
    double Dp = 1.0, zp = 0.0, dDp = 0.0, dzp = 0.0;
    double sum = 0.0, gsum = 0.0;
    bool bad = false;

    double2 xt = dxt[0], ys = yv[0];
    for (int64_t n = 0; n < N; ++n) {
        const double dx = xt.x, t = xt.y, yn = ys.x;
        double D = ys.y + asum, dD = dasum, uf = 0.0, duf = 0.0;
        if (n + 1 < N) { xt = dxt[n + 1]; ys = yv[n + 1]; }       // the next sample's loads fly during this one's step
        if constexpr (J > 0) {
            double U[J], V[J], ph[J], dU[J], rate[J], lag[J], Wn[J];
            pat_decay<J>(k, dx, ph);
            pat_generators<J>(k, t, t_first, U, V);
#pragma unroll
            for (int i = 0; i < J; ++i) { rate[i] = -(dk.c[i] * dx); lag[i] = dk.d[i] * dx; }
            pat_fwd_step_tangent<J>(S, f, dS, df, ph, rate, Wp, dWp, Dp, dDp, zp, dzp);
            pat_fwd_step<J>(S, f, ph, Wp, Dp, zp);
            pat_turn_tangent<J>(k.NR, S, f, dS, df, lag);
            pat_generators_tangent<J>(dk, k.NR, V, dU);
#pragma unroll
            for (int i = 0; i < J; ++i) { uf += U[i] * f[i]; duf += dU[i] * f[i] + U[i] * df[i]; }
            pat_pivot<J>(S, U, V, Wn, D);
#pragma unroll
            for (int i = 0; i < J; ++i) Wp[i] = Wn[i] / D;
            pat_pivot_tangent<J>(S, dS, U, dU, Wp, 1.0 / D, dasum, dWp, dD);
        }
        bad = bad || !(D > 0.0);
        const double z = yn - (slope * t + icpt) - uf;
        const double dz = -(dslope * t + dicpt) - duf;
        const double rD = 1.0 / D, zr = z * rD;
        sum += z * zr + log(D);
        gsum += 2.0 * zr * dz - zr * zr * dD + dD * rD;
        Dp = D; zp = z; dDp = dD; dzp = dz;
    }
    if (bad) {
        a.grad[l] = NAN;
        if (p == 0) { a.status[e] = MTG_ST_NOTPD; a.out[e] = -INFINITY; }
        return;
    }
    a.grad[l] = -0.5 * gsum;
    if (p == 0) a.out[e] = -0.5 * sum - 0.5 * (double)N * 1.8378770664093453;   // ln 2 pi
}

template <int J>
struct GradLaunch {
    static void launch(const MtgGradArgs &a, hipStream_t s)
    {
        if constexpr (J <= MTG_GRAD_MAX_J) {
            const int64_t lanes = a.B * a.P;
            hipLaunchKernelGGL((mtg_loglike_grad_kernel<J>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, a);
        }
    }
};

// the whole batch; J = nr0 + 2 nc0 in 0 .. MTG_GRAD_MAX_J (returns 0 otherwise, nothing launched)
int mtg_launch_loglike_grad(const MtgGradArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J < 0 || J > MTG_GRAD_MAX_J) return 0;
    const int64_t lanes = a.B * a.P;
    hipLaunchKernelGGL(mtg_grad_tangent_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a);
    if (J != 0) return pat_dispatch_rank<GradLaunch>(J, a, s);
    GradLaunch<0>::launch(a, s);
    return 1;
}
