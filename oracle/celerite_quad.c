/*
 * oracle/celerite_quad.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The one-sweep celerite recurrence of oracle/celerite_ref.c (fused_impl) restated in __float128
 * (libquadmath): the truth every likelihood kernel is held to at large N.  An O(N J^2) sweep in quad
 * precision carries ~1e-34 relative rounding per operation, so its lnL is exact to the last bit of a
 * double wherever the float64 problem itself is (well or badly) conditioned to less than ~1e15.
 *
 * Inputs are the float64 values the kernels see, promoted exactly:
 *   yerr_n = fl64(dy_n + 1e-12) (rounded in double, as gpmodelling.py and Engine.set_lightcurves do);
 *   the constant / linear mean as given (the linear mean evaluated in quad);
 *   phases d t_n and exponents c (t_n - t_{n-1}) formed in quad from the double t;
 *   coefficients built from theta IN QUAD (oracle_quad_logprob_batch: the definition of lnL(theta)), or taken
 *   as raw float64 coefficients (oracle_quad_coeffs_batch: the truth of Engine.loglike_coeffs).
 *
 * Per row: lnL as a double pair (hi, lo), the error scale S = 1/2 (sum |ln D_n| + sum z_n^2 / D_n + N ln 2 pi)
 * and the status (0 ok, 2 non-positive pivot, 3 non-finite, -1 bad input).  reverse != 0 sweeps the
 * time-reversed series (residual first, then the sweep with |dx| and the phases at t_{N-1} - t): the likelihood
 * is invariant under reversal and under a shift of the phase origin, so the two directions are independent rounding
 * paths of one value -- the trigonometric values included.
 *
 * Resolution: every covariance entry the sweep implies carries ~2^-113 of the signal amplitude A (the sum of the
 * |a|, |b| and the jitter) in rounding, so the quad value is itself uncertain by ~N 2^-113 A / min(yerr^2) in lnL.
 * That is below 2^-53 |lnL| except where A / yerr^2 approaches 1e19 (the top corners of the prior box);
 * tests/test_quad_oracle.py holds it to that bound.
 *
 * Built on demand (`make -C oracle liboracle_quad.so`, oracle/quad.py); only tests/ use it.
 */
#include <math.h>
#include <quadmath.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define ORACLE_API __attribute__((visibility("default")))

typedef __float128 Q;

enum { K_REAL = 0, K_COMPLEX3, K_COMPLEX4, K_SHO, K_MATERN32, K_JITTER, K_DRW, K_LORENTZIAN, K_COSINUS, K_BPL };

#define QMAXJ 32

static int nparams(int kind)
{
    static const int n[] = {2, 3, 4, 3, 2, 1, 2, 3, 2, 3};
    return kind >= 0 && kind <= 9 ? n[kind] : -1;
}

typedef struct {
    int jr, jc;
    Q ar[QMAXJ], cr[QMAXJ], ac[QMAXJ / 2], bc[QMAXJ / 2], cc[QMAXJ / 2], dc[QMAXJ / 2];
    Q jitter;
} qcoeffs;

/* celerite_ref.c:oracle_build_coeffs in quad: every exp, sqrt and product of theta formed in __float128 */
static int build_coeffs_q(int nterms, const int *kinds, const double *extra, const double *p, qcoeffs *k)
{
    int jr = 0, jc = 0;
    Q jitter = 0;
    for (int i = 0; i < nterms; ++i) {
        if (nparams(kinds[i]) < 0) return -1;
        if (jr + 2 > QMAXJ || jc + 1 > QMAXJ / 2) return -1;
        switch (kinds[i]) {
        case K_REAL:
            k->ar[jr] = expq(p[0]); k->cr[jr] = expq(p[1]); ++jr;
            break;
        case K_COMPLEX3:
            k->ac[jc] = expq(p[0]); k->bc[jc] = 0; k->cc[jc] = expq(p[1]); k->dc[jc] = expq(p[2]); ++jc;
            break;
        case K_COMPLEX4:
            k->ac[jc] = expq(p[0]); k->bc[jc] = expq(p[1]); k->cc[jc] = expq(p[2]); k->dc[jc] = expq(p[3]); ++jc;
            break;
        case K_SHO: {
            /* the regime is decided on Q = exp(log_Q) in quad: at Q = 1/2 exactly both forms are singular */
            const Q S0 = expq(p[0]), Qf = expq(p[1]), w0 = expq(p[2]);
            if (Qf < 0.5Q) {
                const Q f = sqrtq(1 - 4 * Qf * Qf);
                k->ar[jr] = 0.5Q * S0 * w0 * Qf * (1 + 1 / f); k->cr[jr] = 0.5Q * w0 / Qf * (1 - f); ++jr;
                k->ar[jr] = 0.5Q * S0 * w0 * Qf * (1 - 1 / f); k->cr[jr] = 0.5Q * w0 / Qf * (1 + f); ++jr;
            } else {
                const Q f = sqrtq(4 * Qf * Qf - 1);
                k->ac[jc] = S0 * w0 * Qf; k->bc[jc] = S0 * w0 * Qf / f;
                k->cc[jc] = 0.5Q * w0 / Qf; k->dc[jc] = 0.5Q * w0 / Qf * f; ++jc;
            }
            break;
        }
        case K_MATERN32: {
            const Q eps = extra ? (Q)extra[i] : (Q)0.01;   /* the double the builders are handed */
            const Q w0 = sqrtq(3) * expq(-(Q)p[1]);
            const Q S0 = expq(2 * (Q)p[0]) / w0;
            k->ac[jc] = w0 * S0; k->bc[jc] = w0 * w0 * S0 / eps; k->cc[jc] = w0; k->dc[jc] = eps; ++jc;
            break;
        }
        case K_JITTER:
            jitter += expq(2 * (Q)p[0]);
            break;
        case K_DRW:
            k->ar[jr] = expq(p[0]); k->cr[jr] = expq(p[1]); ++jr;   /* 0.5 w0 / Q with Q = 1/2 */
            break;
        case K_LORENTZIAN:
            k->ar[jr] = 0; k->cr[jr] = 0; ++jr;
            k->ac[jc] = expq(p[0]); k->bc[jc] = 0;
            k->cc[jc] = 0.5Q * expq(p[2]) / expq(p[1]); k->dc[jc] = expq(p[2]); ++jc;
            break;
        case K_COSINUS:
            k->ac[jc] = expq(p[0]); k->bc[jc] = 0; k->cc[jc] = 0; k->dc[jc] = expq(p[1]); ++jc;
            break;
        case K_BPL:
            k->ac[jc] = expq(p[0]); k->bc[jc] = expq(p[1]); k->cc[jc] = expq(p[2]); k->dc[jc] = expq(p[2]); ++jc;
            break;
        }
        p += nparams(kinds[i]);
    }
    if (jr + 2 * jc > QMAXJ) return -1;
    k->jr = jr; k->jc = jc; k->jitter = jitter;
    return 0;
}

/*
 * fused_impl in quad.  mean_kind 1: mu = slope t + intercept (in quad), else mu = mean_params[0].
 * The residual and the variance are laid out first (in the sweep's order), then swept.
 */
static int sweep_q(long N, const double *t, const double *y, const double *dy, const qcoeffs *k, int mean_kind,
                   const double *mean_params, int reverse, Q *r, Q *var, double *hi, double *lo, double *scale)
{
    const int jr = k->jr, jc = k->jc, J = jr + 2 * jc;
    Q S[QMAXJ * QMAXJ], f[QMAXJ], W[QMAXJ], U[QMAXJ], V[QMAXJ], ph[QMAXJ];
    Q asum = k->jitter;
    for (int j = 0; j < jr; ++j) asum += k->ar[j];
    for (int c = 0; c < jc; ++c) asum += k->ac[c];
    for (long n = 0; n < N; ++n) {
        const long m = reverse ? N - 1 - n : n;
        const Q mu = mean_kind == 1 ? (Q)mean_params[0] * (Q)t[m] + (Q)mean_params[1] : (Q)mean_params[0];
        const double yerr = dy[m] + 1e-12;                     /* gpmodelling.py:54, in double */
        r[n] = (Q)y[m] - mu;
        var[n] = (Q)yerr * (Q)yerr + asum;
    }
    memset(S, 0, sizeof(Q) * (size_t)J * J);
    memset(f, 0, sizeof(Q) * (size_t)J);
    memset(W, 0, sizeof(Q) * (size_t)J);
    /* reversed: t'_n = t_{N-1} - t_{N-1-n}, exact in quad -- the phases too take another rounding path */
    const Q sgn = reverse ? -1 : 1, t0 = reverse ? (Q)t[N - 1] : 0;
    Q logdet = 0, labs = 0, dot = 0, zprev = 0, Dp = 1;
    for (long n = 0; n < N; ++n) {
        const long m = reverse ? N - 1 - n : n, mp = reverse ? m + 1 : m - 1;
        const Q tn = t0 + sgn * (Q)t[m];
        const Q dx = n > 0 ? sgn * ((Q)t[m] - (Q)t[mp]) : 0;
        for (int j = 0; j < jr; ++j) { U[j] = k->ar[j]; V[j] = 1; ph[j] = expq(-k->cr[j] * dx); }
        for (int c = 0; c < jc; ++c) {
            Q sd, cd;
            sincosq(k->dc[c] * tn, &sd, &cd);
            const Q e = expq(-k->cc[c] * dx);
            U[jr + 2 * c] = k->ac[c] * cd + k->bc[c] * sd;
            U[jr + 2 * c + 1] = k->ac[c] * sd - k->bc[c] * cd;
            V[jr + 2 * c] = cd;
            V[jr + 2 * c + 1] = sd;
            ph[jr + 2 * c] = ph[jr + 2 * c + 1] = e;
        }
        Q Dn = var[n], z = r[n];
        if (n > 0) {
            for (int i = 0; i < J; ++i) {
                for (int j = 0; j <= i; ++j) {
                    const Q s = ph[i] * ph[j] * (S[i * J + j] + Dp * W[i] * W[j]);
                    S[i * J + j] = s; S[j * J + i] = s;
                }
                f[i] = ph[i] * (f[i] + W[i] * zprev);
                z -= U[i] * f[i];
            }
        }
        for (int i = 0; i < J; ++i) {
            Q q = 0;
            for (int j = 0; j < J; ++j) q += S[i * J + j] * U[j];
            W[i] = V[i] - q;
            Dn -= U[i] * q;
        }
        if (!(Dn > 0)) { *hi = -INFINITY; *lo = 0.0; *scale = NAN; return 2; }
        for (int i = 0; i < J; ++i) W[i] /= Dn;
        const Q l = logq(Dn);
        logdet += l;
        labs += fabsq(l);
        dot += z * z / Dn;
        zprev = z;
        Dp = Dn;
    }
    const Q nl2pi = (Q)N * logq(2 * M_PIq);
    const Q ll = -0.5Q * (dot + logdet + nl2pi);
    const double h = (double)ll;
    if (!isfinite(h)) { *hi = -INFINITY; *lo = 0.0; *scale = NAN; return 3; }
    *hi = h;
    *lo = (double)(ll - (Q)h);
    *scale = (double)(0.5Q * (labs + dot + nl2pi));
    return 0;
}

static Q *alloc_work(long N) { return (Q *)malloc(sizeof(Q) * 2 * (size_t)(N > 0 ? N : 1)); }

/*
 * lnL(theta) for a batch.  params: [B][PF] full vectors (kernel parameters in `+` order, then the mean: 1 value for
 * mean_kind 0, (slope, intercept) for 1).  t: [N] shared; y, dy: [L][N]; lc_index: [B] or NULL.  No prior.
 * Returns 0, or -1 when a row had an unknown term kind / too many terms (its status is -1).
 */
ORACLE_API int oracle_quad_logprob_batch(long N, long L, const double *t, const double *y, const double *dy,
                                         int nterms, const int *kinds, const double *extra, int mean_kind, int PF,
                                         long B, const double *params, const int *lc_index, int reverse,
                                         int nthreads, double *hi, double *lo, double *scale, int *status)
{
    int bad = 0;
    int nk = 0;
    (void)L;
    for (int i = 0; i < nterms; ++i) nk += nparams(kinds[i]) > 0 ? nparams(kinds[i]) : 0;
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
#pragma omp parallel num_threads(nthreads)
#endif
    {
        Q *work = alloc_work(N);
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
        for (long b = 0; b < B; ++b) {
            const double *p = params + (size_t)b * PF;
            const long lc = lc_index ? lc_index[b] : 0;
            qcoeffs k;
            if (!work || build_coeffs_q(nterms, kinds, extra, p, &k) != 0) {
                hi[b] = NAN; lo[b] = 0.0; scale[b] = NAN; status[b] = -1; bad = 1; continue;
            }
            status[b] = sweep_q(N, t, y + (size_t)lc * N, dy + (size_t)lc * N, &k, mean_kind, p + nk, reverse,
                                work, work + N, hi + b, lo + b, scale + b);
        }
        free(work);
    }
    return bad ? -1 : 0;
}

/*
 * The raw-coefficient entry (the truth of Engine.loglike_coeffs): float64 coefficients [B][jr] / [B][jc], jitter [B]
 * (NULL = 0), mean_params [B][1 or 2], promoted exactly.
 */
ORACLE_API int oracle_quad_coeffs_batch(long N, long L, const double *t, const double *y, const double *dy, long B,
                                        int jr, int jc, const double *ar, const double *cr, const double *ac,
                                        const double *bc, const double *cc, const double *dc, const double *jitter,
                                        int mean_kind, const double *mean_params, const int *lc_index, int reverse,
                                        int nthreads, double *hi, double *lo, double *scale, int *status)
{
    const int nm = mean_kind == 1 ? 2 : 1;
    (void)L;
    if (jr < 0 || jc < 0 || jr + 2 * jc > QMAXJ || jc > QMAXJ / 2) return -1;
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
#pragma omp parallel num_threads(nthreads)
#endif
    {
        Q *work = alloc_work(N);
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
        for (long b = 0; b < B; ++b) {
            const long lc = lc_index ? lc_index[b] : 0;
            qcoeffs k;
            k.jr = jr; k.jc = jc;
            k.jitter = jitter ? (Q)jitter[b] : 0;
            for (int j = 0; j < jr; ++j) { k.ar[j] = ar[b * jr + j]; k.cr[j] = cr[b * jr + j]; }
            for (int c = 0; c < jc; ++c) {
                k.ac[c] = ac[b * jc + c]; k.bc[c] = bc[b * jc + c]; k.cc[c] = cc[b * jc + c]; k.dc[c] = dc[b * jc + c];
            }
            if (!work) { hi[b] = NAN; lo[b] = 0.0; scale[b] = NAN; status[b] = -1; continue; }
            status[b] = sweep_q(N, t, y + (size_t)lc * N, dy + (size_t)lc * N, &k, mean_kind,
                                mean_params + (size_t)b * nm, reverse, work, work + N, hi + b, lo + b, scale + b);
        }
        free(work);
    }
    return 0;
}

/* the quad coefficient builders alone, rounded to double (against tests/golden/coeff_golden.npz) */
ORACLE_API int oracle_quad_build_coeffs(int nterms, const int *kinds, const double *extra, const double *p,
                                        int *jr_out, double *ar, double *cr, int *jc_out, double *ac, double *bc,
                                        double *cc, double *dc, double *jitter_out)
{
    qcoeffs k;
    if (build_coeffs_q(nterms, kinds, extra, p, &k) != 0) return -1;
    for (int j = 0; j < k.jr; ++j) { ar[j] = (double)k.ar[j]; cr[j] = (double)k.cr[j]; }
    for (int c = 0; c < k.jc; ++c) {
        ac[c] = (double)k.ac[c]; bc[c] = (double)k.bc[c]; cc[c] = (double)k.cc[c]; dc[c] = (double)k.dc[c];
    }
    *jr_out = k.jr; *jc_out = k.jc; *jitter_out = (double)k.jitter;
    return 0;
}

/* the prediction and solve recurrences in quad (oracle/predict_sweep.h): oracle_quad_predict_batch,
 * oracle_quad_apply_inverse, oracle_quad_predict_at -- the truth of tests/golden/predict_golden.npz */
#define R Q
#define PS_API ORACLE_API
#define PS_EXP expq
#define PS_FABS fabsq
#define PS_SINCOS sincosq
#define PS_COEFFS qcoeffs
#define PS_BUILD build_coeffs_q
#define PS_NPARAMS nparams
#define PS_ENTRY(name) oracle_quad_##name
#include "predict_sweep.h"
