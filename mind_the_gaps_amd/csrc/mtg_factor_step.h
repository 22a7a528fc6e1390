// mtg_factor_step.h -- the forward step of the semiseparable factorisation with the state in registers (template on
// the rank J, runtime split NR real slots | complex pairs): coefficient load and row constants, generators, decay, the
// (S, f) recurrence and the pivot; the state of a forward sweep with its innovation step (PatState); the backward
// recurrences; and the switch from a runtime rank to the template.
// Shared by
//   mtg_predict_at.hip       the factorisation, written out from the step functions (its z is taken off y - mean term by
//                            term, a rounding of its own), and, through mtg_pat_replay.h, the replay at new times
//   mtg_predict_terms.hip    the same replay (mtg_pat_replay.h)
//   mtg_gp_draw.hip          PatState::advance: the draw y = mean + L sqrt(D) q
//   mtg_whiten.hip           PatState::advance: its inverse q = D^-1/2 L^-1 (y - mean)
//   mtg_gp_cond_draw.hip     PatState::advance on the merged series
//   mtg_loglike_grad.hip     the step functions, interleaved with those of mtg_factor_step_tangent.h
#pragma once
#include "mtg_math.h"
#include "mtg_device.h"

template <int J>
struct PatCoef {
    double a[J], b[J], c[J], d[J];   // per slot: real j: (a_j, -, c_j, -); complex k: both slots (a_k, b_k, c_k, d_k)
    double k0, slope, icpt, asum;
    int NR;
};

__host__ __device__ constexpr int pat_sy(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

template <int J>
__device__ __forceinline__ void pat_load_coef(const MtgRowArgs &a, int64_t e, PatCoef<J> &k)
{
#pragma clang fp contract(off)
    const int NR = a.nr0 + 2 * a.sig[e];
    const double *cf = a.coef + e;
    const int64_t cs = a.cstride;
    k.NR = NR;
    double k0 = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        if (i < NR) {
            k.a[i] = cf[a.lay.ar(i) * cs]; k.c[i] = cf[a.lay.cr(i) * cs]; k.b[i] = 0.0; k.d[i] = 0.0;
            k0 += k.a[i];
        } else {
            const int q = (i - NR) >> 1;
            k.a[i] = cf[a.lay.ac(q) * cs]; k.b[i] = cf[a.lay.bc(q) * cs];
            k.c[i] = cf[a.lay.cc(q) * cs]; k.d[i] = cf[a.lay.dc(q) * cs];
            if (((i - NR) & 1) == 0) k0 += k.a[i];
        }
    }
    k.k0 = k0;
    k.asum = cf[a.lay.asum() * cs];
    k.slope = cf[a.lay.mean(0) * cs];
    k.icpt = cf[a.lay.mean(1) * cs];
}

// the constants of row e: the diagonal's asum and the mean's slope and intercept into k, and for J > 0 the terms beside
// them; J = 0 is the white model, which has no term to load (JA: the rank the arrays are sized for, at least 1)
template <int J, int JA>
__device__ __forceinline__ void pat_load_row(const MtgRowArgs &a, int64_t e, PatCoef<JA> &k)
{
    if constexpr (J > 0) {
        static_assert(J == JA, "the rank of the coefficients");
        pat_load_coef<J>(a, e, k);
    } else {
        k.asum = a.coef[a.lay.asum() * a.cstride + e];
        k.slope = a.coef[a.lay.mean(0) * a.cstride + e];
        k.icpt = a.coef[a.lay.mean(1) * a.cstride + e];
    }
}

// generators at time t: the phase at the elapsed time, reduced modulo 2 pi before it is rounded (mtg_math.h)
template <int J>
__device__ __forceinline__ void pat_generators(const PatCoef<J> &k, double t, double t_first, double *U, double *V)
{
#pragma clang fp contract(off)
    double sn = 0.0, cn = 1.0;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        if (i < k.NR) { U[i] = k.a[i]; V[i] = 1.0; }
        else if (((i - k.NR) & 1) == 0) {
            mtg_elapsed_sincos(k.d[i], t, t_first, &sn, &cn);
            U[i] = k.a[i] * cn + k.b[i] * sn; V[i] = cn;
        } else { U[i] = k.a[i] * sn - k.b[i] * cn; V[i] = sn; }
    }
}

// exp(-c dx) per slot (dx >= 0), one exp per term
template <int J>
__device__ __forceinline__ void pat_decay(const PatCoef<J> &k, double dx, double *ph)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < J; ++i) {
        if (i < k.NR || ((i - k.NR) & 1) == 0) ph[i] = exp(-k.c[i] * dx);
        else ph[i] = ph[i > 0 ? i - 1 : 0];
    }
}

// S <- phi phi^T o (S + Dp Wp Wp^T),  f <- phi o (f + Wp zp)
template <int J>
__device__ __forceinline__ void pat_fwd_step(double *S, double *f, const double *ph, const double *Wp, double Dp, double zp)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < J; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) S[pat_sy(i, j)] = ph[i] * ph[j] * (S[pat_sy(i, j)] + Dp * Wp[i] * Wp[j]);
        f[i] = ph[i] * (f[i] + Wp[i] * zp);
    }
}

// the pivot of sample n: q = S U,  Wn = V - q (not yet divided by D),  D -= U^T q
template <int J>
__device__ __forceinline__ void pat_pivot(const double *S, const double *U, const double *V, double *Wn, double &D)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < J; ++i) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) q += S[pat_sy(i, j)] * U[j];
        Wn[i] = V[i] - q;
        D -= U[i] * q;
    }
}

// The state of a forward sweep, one lane per row: S, f of the recurrence and what the sample before has left -- its
// W (divided by D), its pivot D and its innovation v (z of the likelihood, sqrt(D) q of a draw).
template <int J>
struct PatState {
    double S[J * (J + 1) / 2], f[J], Wp[J], Dp, vp;

    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int i = 0; i < J * (J + 1) / 2; ++i) S[i] = 0.0;
#pragma unroll
        for (int i = 0; i < J; ++i) { f[i] = 0.0; Wp[i] = 0.0; }
        Dp = 1.0; vp = 0.0;
    }

    // the innovation step of the sample at time t, dx after the one before: decay, generators, (S, f) forward, then the
    // pivot.  D comes in as the sample's diagonal (sigma^2 + asum; k(0) at a noise-free new time) and goes out as its
    // pivot; -> U^T f, what the samples before predict of this one.  The caller forms the innovation v from it and
    // hands (D, v) back with leave(); W of this sample is kept here.
    __device__ __forceinline__ double advance(const PatCoef<J> &k, double dx, double t, double t_first, double &D)
    {
#pragma clang fp contract(off)
        double U[J], V[J], ph[J], Wn[J], uf = 0.0;
        pat_decay<J>(k, dx, ph);
        pat_generators<J>(k, t, t_first, U, V);
        pat_fwd_step<J>(S, f, ph, Wp, Dp, vp);
#pragma unroll
        for (int i = 0; i < J; ++i) uf += U[i] * f[i];
        pat_pivot<J>(S, U, V, Wn, D);
#pragma unroll
        for (int i = 0; i < J; ++i) Wp[i] = Wn[i] / D;
        return uf;
    }

    __device__ __forceinline__ void leave(double D, double v) { Dp = D; vp = v; }
};

// ---- the backward recurrences of the new-time prediction (mtg_predict_at.hip, mtg_predict_terms.hip) ----
// g <- phn o (g + Un xn): g_n from g_{n+1} and sample n + 1
template <int J>
__device__ __forceinline__ void pat_bwd_g(double *g, const double *phn, const double *Un, double xn)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < J; ++i) g[i] = phn[i] * (g[i] + Un[i] * xn);
}

// G <- U U^T / D + (I - U W^T) X (I - W U^T),  X = phn phn^T o G: G_n from G_{n+1} and sample n
// (forming A = I - U W^T explicitly and the product A X with it was tried: J^3 instead of J^2, and no more accurate --
// 0.78 of the bound on `signatures` against 0.013)
template <int J>
__device__ __forceinline__ void pat_bwd_G(double *G, const double *phn, const double *U, const double *W, double D)
{
#pragma clang fp contract(off)
    double XW[J], wxw = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) G[pat_sy(i, j)] = phn[i] * phn[j] * G[pat_sy(i, j)];
#pragma unroll
    for (int i = 0; i < J; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) s += G[pat_sy(i, j)] * W[j];
        XW[i] = s;
    }
#pragma unroll
    for (int i = 0; i < J; ++i) wxw += W[i] * XW[i];
    const double h = wxw + 1.0 / D;
#pragma unroll
    for (int i = 0; i < J; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j)
            G[pat_sy(i, j)] = G[pat_sy(i, j)] - U[i] * XW[j] - XW[i] * U[j] + U[i] * U[j] * h;
}

// F<J>::launch(args...) for the rank J in 1 .. MTG_MAX_J; 0 = no such rank (rank 0, the white model, is the caller's)
template <template <int> class F, class... A>
int pat_dispatch_rank(int J, const A &...args)
{
    switch (J) {
    case 1: F<1>::launch(args...); break;
    case 2: F<2>::launch(args...); break;
    case 3: F<3>::launch(args...); break;
    case 4: F<4>::launch(args...); break;
    case 5: F<5>::launch(args...); break;
    case 6: F<6>::launch(args...); break;
    case 7: F<7>::launch(args...); break;
    case 8: F<8>::launch(args...); break;
    case 9: F<9>::launch(args...); break;
    case 10: F<10>::launch(args...); break;
    default: return 0;
    }
    return 1;
}
