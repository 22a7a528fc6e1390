// mtg_factor_step_tangent.h -- the directional derivative of mtg_factor_step.h's forward step by one parameter, with
// the tangent state in registers next to the primal one (template on the rank J, runtime split NR real slots | complex
// pairs).  The primal is computed by mtg_factor_step.h's own functions; these read its state and never write it.
//
// Rotated frame.  A frequency d reaches the generators of its (cos, sin) pair through the phase d (t_n - t_0), so the
// plain tangent of every vector x of the pair (U, V, f, W, the rows and columns of S) is x' = x~ + d' (t_n - t_0) R x,
// R the quarter turn (x_cos, x_sin) -> (-x_sin, x_cos).  The scalars D_n and z_n do not turn: the elapsed-time terms
// cancel in every sample's contribution, after having been formed (t_n - t_0) / lag times larger than what is left.
// What is carried here is x~: U~ and V~ hold a' and b' only (V~ = 0), and each step turns the carried tangents by the
// lag alone, f~ -= d' dx R f, S~ -= d' dx (R S + S R^T) -- exact, R commuting with a pair's common decay.  Measured
// on the host replay against the quad-precision truth at N = 1000 (tests/test_loglike_grad_cpu.py): worst error in units
// of sqrt(N) u G_p 59.6 plain against 12.4 rotated, and 59.6 against 1.07 without the Matern-3/2 model.
#pragma once
#include "mtg_factor_step.h"

template <int J>
struct PatCoefTangent {
    double a[J], b[J], c[J], d[J];   // per slot, as PatCoef
    double slope, icpt, asum;
};

// dcoef: this lane's column of the tangent workspace (slot stride ds); NR: the row's real slots (PatCoef::NR)
template <int J>
__device__ __forceinline__ void pat_load_coef_tangent(const double *dcoef, int64_t ds, const MtgCoefLayout &lay, int NR,
                                                      PatCoefTangent<J> &dk)
{
#pragma unroll
    for (int i = 0; i < J; ++i) {
        if (i < NR) {
            dk.a[i] = dcoef[lay.ar(i) * ds]; dk.c[i] = dcoef[lay.cr(i) * ds]; dk.b[i] = 0.0; dk.d[i] = 0.0;
        } else {
            const int q = (i - NR) >> 1;
            dk.a[i] = dcoef[lay.ac(q) * ds]; dk.b[i] = dcoef[lay.bc(q) * ds];
            dk.c[i] = dcoef[lay.cc(q) * ds]; dk.d[i] = dcoef[lay.dc(q) * ds];
        }
    }
    dk.asum = dcoef[lay.asum() * ds];
    dk.slope = dcoef[lay.mean(0) * ds];
    dk.icpt = dcoef[lay.mean(1) * ds];
}

// U~ from the generators V = (1 | cos | sin) pat_generators has just made: a' | a' cos + b' sin | a' sin - b' cos
template <int J>
__device__ __forceinline__ void pat_generators_tangent(const PatCoefTangent<J> &dk, int NR, const double *V, double *dU)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < J; ++i) {
        if (i < NR) dU[i] = dk.a[i];
        else if (((i - NR) & 1) == 0) dU[i] = dk.a[i] * V[i] + dk.b[i] * V[i + 1 < J ? i + 1 : i];
        else dU[i] = dk.a[i] * V[i] - dk.b[i] * V[i > 0 ? i - 1 : 0];
    }
}

// the tangent of pat_fwd_step, from the state BEFORE it (call it first): with T = S + Dp Wp Wp^T, g = f + Wp zp and
// phi' = rate phi (rate_i = -c'_i dx),
//   S~ <- phi phi^T o ((rate_i + rate_j) T + S~ + Dp' Wp Wp^T + Dp (Wp~ Wp^T + Wp Wp~^T)),
//   f~ <- phi o (rate g + f~ + Wp~ zp + Wp zp')
template <int J>
__device__ __forceinline__ void pat_fwd_step_tangent(const double *S, const double *f, double *dS, double *df, const double *ph,
                                                     const double *rate, const double *Wp, const double *dWp, double Dp,
                                                     double dDp, double zp, double dzp)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < J; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double T = S[pat_sy(i, j)] + Dp * Wp[i] * Wp[j];
            const double dT = dS[pat_sy(i, j)] + dDp * Wp[i] * Wp[j] + Dp * (dWp[i] * Wp[j] + Wp[i] * dWp[j]);
            dS[pat_sy(i, j)] = ph[i] * ph[j] * ((rate[i] + rate[j]) * T + dT);
        }
        const double g = f[i] + Wp[i] * zp;
        df[i] = ph[i] * (rate[i] * g + (df[i] + dWp[i] * zp + Wp[i] * dzp));
    }
}

// the turn by the lag, from the state AFTER pat_fwd_step: f~ -= lag R f, S~ -= lag_i (R S)_ij + lag_j (R S)_ji,
// (R x)_cos = -x_sin, (R x)_sin = x_cos, lag_i = d'_i dx (0 on a real slot)
template <int J>
__device__ __forceinline__ void pat_turn_tangent(int NR, const double *S, const double *f, double *dS, double *df, const double *lag)
{
#pragma clang fp contract(off)
    // (the partner's entry is picked by value from the two candidates, and a real slot takes part with its lag of 0:
    // an index or a conditional store that depends on NR would send the register arrays to scratch)
#pragma unroll
    for (int i = 0; i < J; ++i) {
        constexpr int last = J - 1;
        const int up = i < last ? i + 1 : i, dn = i > 0 ? i - 1 : 0;
        const bool ci = ((i - NR) & 1) == 0;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const int uq = j < last ? j + 1 : j, dq = j > 0 ? j - 1 : 0;
            const bool cj = ((j - NR) & 1) == 0;
            // lag_i (R S)_ij + lag_j (R S)_ji
            const double ti = lag[i] * (ci ? -S[pat_sy(up, j)] : S[pat_sy(dn, j)]);
            const double tj = lag[j] * (cj ? -S[pat_sy(uq, i)] : S[pat_sy(dq, i)]);
            dS[pat_sy(i, j)] -= ti + tj;
        }
        df[i] -= lag[i] * (ci ? -f[up] : f[dn]);
    }
}

// the tangent of the pivot of sample n: with q = S U, q~ = S~ U + S U~,
//   D' = asum' - U~^T q - U^T q~,   W~ = (V~ - q~ - W D') / D   (V~ = 0; W = pat_pivot's Wn / D)
template <int J>
__device__ __forceinline__ void pat_pivot_tangent(const double *S, const double *dS, const double *U, const double *dU,
                                                  const double *W, double rD, double dasum, double *dW, double &dD)
{
#pragma clang fp contract(off)
    double dq[J];
    dD = dasum;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        double q = 0.0, t = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            q += S[pat_sy(i, j)] * U[j];
            t += dS[pat_sy(i, j)] * U[j] + S[pat_sy(i, j)] * dU[j];
        }
        dq[i] = t;
        dD -= dU[i] * q + U[i] * t;
    }
#pragma unroll
    for (int i = 0; i < J; ++i) dW[i] = (-dq[i] - W[i] * dD) * rD;
}
