/*
 * oracle/predict_sweep.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The O(N J^2) prediction and solve recurrences of celerite, written once for two
 * arithmetic types.  oracle/celerite_quad.c includes it with R = __float128 (the truth of
 * tests/golden/predict_golden.npz); oracle/celerite_ref.c includes it with R = double, the phase at the absolute time
 * (cos(d t), sin(d t)) as celerite forms it ("c64": how far honest float64 arithmetic lands from the truth).
 *
 * Per parameter vector, in the sweep's order n (m = N-1-n when reversed, else m = n):
 *   generators   U_n, V_n, phi_n (phi_n = exp(-c (t_n - t_{n-1}))), d_n = yerr_n^2 + jitter, K_nn = yerr_n^2 + sum a
 *   factor       K = L D L^T, L_nm = U_n^T Phi(n, m) W_m (n > m): S, D_n, W_n (celerite's compute)
 *   solve        K^-1 b: forward f_n = phi_n (f_{n-1} + W_{n-1} z_{n-1}), z_n = b_n - U_n^T f_n, then backward
 *                g_n = phi_{n+1} (g_{n+1} + U_{n+1} x_{n+1}), x_n = z_n / D_n - W_n^T g_n
 *   diag(K^-1)   (K^-1)_nn = 1/D_n + W_n^T X_n W_n, X_n = Phi_{n+1} G_{n+1} Phi_{n+1},
 *                G_n = U_n U_n^T / D_n + (I - U_n W_n^T) X_n (I - W_n U_n^T)
 *   matvec       K x with the O(N J) semiseparable product (celerite's dot)
 * K^-1 b and diag(K^-1) are equivariant under time reversal, so the reversed sweep (phases at t_{N-1} - t, exact in
 * quad) is a second rounding path to the same values.
 *
 * The includer defines R, PS_EXP, PS_FABS, PS_SINCOS(x, &s, &c), PS_COEFFS (a struct with jr, jc, ar, cr, ac, bc, cc,
 * dc, jitter of type R), PS_BUILD(nterms, kinds, extra, p, &k) -> 0 / -1, PS_NPARAMS(kind) and PS_ENTRY(name), the
 * exported names of the three entries at the end.
 */
#ifndef PS_ENTRY
#error "define R, PS_EXP, PS_FABS, PS_SINCOS, PS_COEFFS, PS_BUILD, PS_NPARAMS and PS_ENTRY before including"
#endif

#define PS_MAXJ 32

typedef struct {
    long N;
    int J;
    R *mem, *U, *V, *ph, *W, *D, *d, *kd;
} ps_fac;

static int ps_alloc(ps_fac *f, long N, int J)
{
    const size_t nJ = (size_t)N * (size_t)(J > 0 ? J : 1);
    f->N = N; f->J = J;
    f->mem = (R *)malloc(sizeof(R) * (4 * nJ + 3 * (size_t)N));
    if (!f->mem) return -1;
    f->U = f->mem; f->V = f->U + nJ; f->ph = f->V + nJ; f->W = f->ph + nJ;
    f->D = f->W + nJ; f->d = f->D + N; f->kd = f->d + N;
    return 0;
}

static void ps_free(ps_fac *f) { free(f->mem); f->mem = NULL; }

static long ps_index(long N, long n, int reverse) { return reverse ? N - 1 - n : n; }

static void ps_generators(ps_fac *f, const double *t, const double *dy, const PS_COEFFS *k, int reverse)
{
    const long N = f->N;
    const int jr = k->jr, jc = k->jc, J = f->J;
    R asum = k->jitter;
    for (int j = 0; j < jr; ++j) asum += k->ar[j];
    for (int c = 0; c < jc; ++c) asum += k->ac[c];
    for (long n = 0; n < N; ++n) {
        const long m = ps_index(N, n, reverse);
        const double yerr = dy[m] + 1e-12;                      /* gpmodelling.py:54, in double */
        const R tn = reverse ? (R)t[N - 1] - (R)t[m] : (R)t[m];
        const R dx = n == 0 ? (R)0 : reverse ? (R)t[m + 1] - (R)t[m] : (R)t[m] - (R)t[m - 1];
        R *U = f->U + (size_t)n * J, *V = f->V + (size_t)n * J, *ph = f->ph + (size_t)n * J;
        f->d[n] = (R)yerr * (R)yerr + k->jitter;
        f->kd[n] = (R)yerr * (R)yerr + asum;
        for (int j = 0; j < jr; ++j) { U[j] = k->ar[j]; V[j] = 1; ph[j] = PS_EXP(-k->cr[j] * dx); }
        for (int c = 0; c < jc; ++c) {
            R sd, cd;
            PS_SINCOS(k->dc[c] * tn, &sd, &cd);
            U[jr + 2 * c] = k->ac[c] * cd + k->bc[c] * sd;
            U[jr + 2 * c + 1] = k->ac[c] * sd - k->bc[c] * cd;
            V[jr + 2 * c] = cd;
            V[jr + 2 * c + 1] = sd;
            ph[jr + 2 * c] = ph[jr + 2 * c + 1] = PS_EXP(-k->cc[c] * dx);
        }
    }
}

/* K = L D L^T; 0, or 2 at the first pivot that is not positive */
static int ps_factor(ps_fac *f)
{
    const long N = f->N;
    const int J = f->J;
    R S[PS_MAXJ * PS_MAXJ];
    memset(S, 0, sizeof(R) * (size_t)J * J);
    for (long n = 0; n < N; ++n) {
        const R *U = f->U + (size_t)n * J, *V = f->V + (size_t)n * J, *ph = f->ph + (size_t)n * J;
        R *W = f->W + (size_t)n * J;
        R Dn = f->kd[n];
        if (n > 0) {
            const R *Wp = W - J, Dp = f->D[n - 1];
            for (int i = 0; i < J; ++i)
                for (int j = 0; j <= i; ++j) {
                    const R s = ph[i] * ph[j] * (S[i * J + j] + Dp * Wp[i] * Wp[j]);
                    S[i * J + j] = s; S[j * J + i] = s;
                }
        }
        for (int i = 0; i < J; ++i) {
            R q = 0;
            for (int j = 0; j < J; ++j) q += S[i * J + j] * U[j];
            W[i] = V[i] - q;
            Dn -= U[i] * q;
        }
        if (!(Dn > 0)) return 2;
        f->D[n] = Dn;
        for (int i = 0; i < J; ++i) W[i] /= Dn;
    }
    return 0;
}

/* b <- K^-1 b (b in the sweep's order) */
static void ps_solve(const ps_fac *f, R *b)
{
    const long N = f->N;
    const int J = f->J;
    R g[PS_MAXJ];
    R zp = 0;
    for (int i = 0; i < J; ++i) g[i] = 0;
    for (long n = 0; n < N; ++n) {
        const R *U = f->U + (size_t)n * J, *ph = f->ph + (size_t)n * J;
        R z = b[n];
        if (n > 0)
            for (int i = 0; i < J; ++i) {
                g[i] = ph[i] * (g[i] + f->W[(size_t)(n - 1) * J + i] * zp);
                z -= U[i] * g[i];
            }
        b[n] = z;
        zp = z;
    }
    R xn = 0;
    for (int i = 0; i < J; ++i) g[i] = 0;
    for (long n = N - 1; n >= 0; --n) {
        const R *W = f->W + (size_t)n * J;
        R x = b[n] / f->D[n];
        if (n < N - 1)
            for (int i = 0; i < J; ++i) {
                g[i] = f->ph[(size_t)(n + 1) * J + i] * (g[i] + f->U[(size_t)(n + 1) * J + i] * xn);
                x -= W[i] * g[i];
            }
        b[n] = x;
        xn = x;
    }
}

/* kinv_n = (K^-1)_nn */
static void ps_diag_inv(const ps_fac *f, R *kinv)
{
    const long N = f->N;
    const int J = f->J;
    R G[PS_MAXJ * PS_MAXJ], X[PS_MAXJ * PS_MAXJ], XW[PS_MAXJ];
    memset(G, 0, sizeof(R) * (size_t)J * J);
    for (long n = N - 1; n >= 0; --n) {
        const R *U = f->U + (size_t)n * J, *W = f->W + (size_t)n * J;
        const R *php = n < N - 1 ? f->ph + (size_t)(n + 1) * J : NULL;
        for (int i = 0; i < J; ++i)
            for (int j = 0; j < J; ++j) X[i * J + j] = php ? php[i] * php[j] * G[i * J + j] : (R)0;
        R wxw = 0;
        for (int i = 0; i < J; ++i) {
            R s = 0;
            for (int j = 0; j < J; ++j) s += X[i * J + j] * W[j];
            XW[i] = s;
            wxw += W[i] * s;
        }
        const R rD = 1 / f->D[n];
        kinv[n] = rD + wxw;
        for (int i = 0; i < J; ++i)
            for (int j = 0; j < J; ++j)
                G[i * J + j] = X[i * J + j] - U[i] * XW[j] - XW[i] * U[j] + U[i] * U[j] * (wxw + rD);
    }
}

/* y = K x (both in the sweep's order) */
static void ps_matvec(const ps_fac *f, const R *x, R *y)
{
    const long N = f->N;
    const int J = f->J;
    R g[PS_MAXJ];
    for (long n = 0; n < N; ++n) y[n] = f->kd[n] * x[n];
    for (int i = 0; i < J; ++i) g[i] = 0;
    for (long n = 1; n < N; ++n)
        for (int i = 0; i < J; ++i) {
            g[i] = f->ph[(size_t)n * J + i] * (g[i] + f->V[(size_t)(n - 1) * J + i] * x[n - 1]);
            y[n] += f->U[(size_t)n * J + i] * g[i];
        }
    for (int i = 0; i < J; ++i) g[i] = 0;
    for (long n = N - 2; n >= 0; --n)
        for (int i = 0; i < J; ++i) {
            g[i] = f->ph[(size_t)(n + 1) * J + i] * (g[i] + f->U[(size_t)(n + 1) * J + i] * x[n + 1]);
            y[n] += f->V[(size_t)n * J + i] * g[i];
        }
}

/* k(tau) without the jitter (terms.Term.get_value) */
static R ps_kval(const PS_COEFFS *k, R tau)
{
    tau = PS_FABS(tau);
    R v = 0;
    for (int j = 0; j < k->jr; ++j) v += k->ar[j] * PS_EXP(-k->cr[j] * tau);
    for (int c = 0; c < k->jc; ++c) {
        R s, co;
        PS_SINCOS(k->dc[c] * tau, &s, &co);
        v += PS_EXP(-k->cc[c] * tau) * (k->ac[c] * co + k->bc[c] * s);
    }
    return v;
}

static R ps_mean(int mean_kind, const double *mp, double t)
{
    return mean_kind == 1 ? (R)mp[0] * (R)t + (R)mp[1] : (R)mp[0];
}

/* v as a double pair: hi = fl64(v), lo = fl64(v - hi) (0 when R is double); lo may be NULL */
static void ps_put(R v, double *hi, double *lo, size_t i)
{
    hi[i] = (double)v;
    if (lo) lo[i] = (double)(v - (R)hi[i]);
}

static int ps_nk(int nterms, const int *kinds)
{
    int nk = 0;
    for (int i = 0; i < nterms; ++i) {
        if (PS_NPARAMS(kinds[i]) < 0) return -1;
        nk += PS_NPARAMS(kinds[i]);
    }
    return nk;
}

/* coefficients, generators and factorisation of one parameter vector: 0, 2 (not positive definite) or -1 */
static int ps_setup(ps_fac *f, long N, const double *t, const double *dy, int nterms, const int *kinds,
                    const double *extra, const double *p, int reverse, PS_COEFFS *k)
{
    if (PS_BUILD(nterms, kinds, extra, p, k) != 0) return -1;
    if (ps_alloc(f, N, k->jr + 2 * k->jc) != 0) return -1;
    ps_generators(f, t, dy, k, reverse);
    return ps_factor(f);
}


/*
 * Conditional mean and variance at the training times for B parameter vectors (Engine.predict):
 *   mu_n  = [mean_n] + r_n - d_n (K^-1 r)_n,  r = y - mean, d_n = yerr_n^2 + jitter -- mean_n added under mean_kind 1
 *           only: a constant mean is the light curve's y_offset, which Engine.predict leaves out;
 *   var_n = d_n - d_n^2 (K^-1)_nn  (the noise-free variance: no jitter, no yerr);
 *   s_mu  = |r_n| + d_n |(K^-1 r)_n|,  s_var = d_n + d_n^2 (K^-1)_nn  (the scales of the two cancellations).
 * params [B][PF] (kernel, then the mean: 1 constant or (slope, intercept)); y, dy [L][N]; outputs [B][N] in time
 * order; mu_lo, var_lo (NULL, or both given) the remainders of the values rounded into mu, var.  status: 0, 2 (not
 * positive definite: outputs NaN), -1 (bad input or no memory).
 */
PS_API int PS_ENTRY(predict_batch)(long N, long L, const double *t, const double *y, const double *dy, int nterms,
                                   const int *kinds, const double *extra, int mean_kind, int PF, long B,
                                   const double *params, const int *lc_index, int reverse, int nthreads, double *mu,
                                   double *var, double *s_mu, double *s_var, double *mu_lo, double *var_lo,
                                   int *status)
{
    const int nk = ps_nk(nterms, kinds);
    (void)L;
    if (nk < 0 || N < 1) return -1;
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 1)
#endif
    for (long b = 0; b < B; ++b) {
        const double *p = params + (size_t)b * PF;
        const long lc = lc_index ? lc_index[b] : 0;
        const double *yl = y + (size_t)lc * N, *dyl = dy + (size_t)lc * N;
        double *mo = mu + (size_t)b * N, *vo = var + (size_t)b * N, *sm = s_mu + (size_t)b * N,
               *sv = s_var + (size_t)b * N;
        PS_COEFFS k;
        ps_fac f = {0};
        R *r = NULL;
        int st = ps_setup(&f, N, t, dyl, nterms, kinds, extra, p, reverse, &k);
        if (st == 0 && !(r = (R *)malloc(sizeof(R) * 3 * (size_t)N))) st = -1;
        if (st != 0) {
            for (long n = 0; n < N; ++n) mo[n] = vo[n] = sm[n] = sv[n] = NAN;
            if (mu_lo) for (long n = 0; n < N; ++n) mu_lo[(size_t)b * N + n] = var_lo[(size_t)b * N + n] = NAN;
        } else {
            R *x = r + N, *kinv = r + 2 * N;
            for (long n = 0; n < N; ++n) {
                const long m = ps_index(N, n, reverse);
                r[n] = (R)yl[m] - ps_mean(mean_kind, p + nk, t[m]);
            }
            memcpy(x, r, sizeof(R) * (size_t)N);
            ps_solve(&f, x);
            ps_diag_inv(&f, kinv);
            for (long n = 0; n < N; ++n) {
                const long m = ps_index(N, n, reverse);
                const R d = f.d[n], dx = d * x[n], ddk = d * d * kinv[n];
                const R mean = mean_kind == 1 ? ps_mean(mean_kind, p + nk, t[m]) : (R)0;
                ps_put(mean + (r[n] - dx), mo, mu_lo ? mu_lo + (size_t)b * N : NULL, (size_t)m);
                ps_put(d - ddk, vo, var_lo ? var_lo + (size_t)b * N : NULL, (size_t)m);
                sm[m] = (double)(PS_FABS(r[n]) + PS_FABS(dx));
                sv[m] = (double)(d + ddk);
            }
        }
        status[b] = st;
        free(r);
        ps_free(&f);
    }
    return 0;
}

/*
 * K^-1 b for M columns b [N][M] (row n: sample n of every column) at one parameter vector p (kernel parameters first;
 * the mean's are ignored) -> x [N][M] (x_lo: the remainders, or NULL).  resid (NULL: not computed) gets K x - b of the solution before it is rounded,
 * formed with ps_matvec in the same arithmetic.  Returns the status (0, 2, -1).
 */
PS_API int PS_ENTRY(apply_inverse)(long N, const double *t, const double *dy, int nterms, const int *kinds,
                                   const double *extra, const double *p, long M, const double *b, int reverse,
                                   int nthreads, double *x, double *x_lo, double *resid)
{
    PS_COEFFS k;
    ps_fac f = {0};
    int st = ps_nk(nterms, kinds) < 0 || N < 1 ? -1 : ps_setup(&f, N, t, dy, nterms, kinds, extra, p, reverse, &k);
    if (st != 0) { ps_free(&f); return st; }
    int bad = 0;
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 1)
#endif
    for (long c = 0; c < M; ++c) {
        R *v = (R *)malloc(sizeof(R) * 3 * (size_t)N);
        if (!v) { bad = 1; continue; }
        R *b0 = v + N, *kx = v + 2 * N;
        for (long n = 0; n < N; ++n) b0[n] = v[n] = (R)b[(size_t)ps_index(N, n, reverse) * M + c];
        ps_solve(&f, v);
        if (resid) ps_matvec(&f, v, kx);
        for (long n = 0; n < N; ++n) {
            const size_t o = (size_t)ps_index(N, n, reverse) * M + c;
            ps_put(v[n], x, x_lo, o);
            if (resid) resid[o] = (double)(kx[n] - b0[n]);
        }
        free(v);
    }
    ps_free(&f);
    return bad ? -1 : 0;
}

/*
 * The prediction at new times ts [Ns] (GP.predict(y, t=ts, return_var=True), celerite's expressions):
 *   mu_s  = mean(ts_s) + k_s^T K^-1 r,  k_s = k(ts_s - t) (no jitter);  var_s = k(0) - k_s^T K^-1 k_s;
 *   s_mu  = |mean(ts_s)| + sum_n |k_sn (K^-1 r)_n|,  s_var = k(0) + |k_s^T K^-1 k_s|.
 * The mean here is the whole mean, a constant one included (GP.predict adds it).  p: [PF] as predict_batch's rows.
 * mu_lo, var_lo: the remainders, or NULL.  Returns the status (0, 2, -1).
 */
PS_API int PS_ENTRY(predict_at)(long N, const double *t, const double *y, const double *dy, int nterms,
                                const int *kinds, const double *extra, int mean_kind, const double *p, long Ns,
                                const double *ts, int reverse, int nthreads, double *mu, double *var, double *s_mu,
                                double *s_var, double *mu_lo, double *var_lo)
{
    PS_COEFFS k;
    ps_fac f = {0};
    const int nk = ps_nk(nterms, kinds);
    int st = nk < 0 || N < 1 ? -1 : ps_setup(&f, N, t, dy, nterms, kinds, extra, p, reverse, &k);
    if (st != 0) { ps_free(&f); return st; }
    R *alpha = (R *)malloc(sizeof(R) * (size_t)N);
    if (!alpha) { ps_free(&f); return -1; }
    for (long n = 0; n < N; ++n) {
        const long m = ps_index(N, n, reverse);
        alpha[n] = (R)y[m] - ps_mean(mean_kind, p + nk, t[m]);
    }
    ps_solve(&f, alpha);
    const R k0 = ps_kval(&k, 0);
    int bad = 0;
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 1)
#endif
    for (long s = 0; s < Ns; ++s) {
        R *ks = (R *)malloc(sizeof(R) * 2 * (size_t)N);
        if (!ks) { bad = 1; continue; }
        R *v = ks + N, m_ = 0, am = 0, kk = 0;
        for (long n = 0; n < N; ++n) {
            ks[n] = v[n] = ps_kval(&k, (R)ts[s] - (R)t[ps_index(N, n, reverse)]);
            m_ += ks[n] * alpha[n];
            am += PS_FABS(ks[n] * alpha[n]);
        }
        ps_solve(&f, v);
        for (long n = 0; n < N; ++n) kk += ks[n] * v[n];
        const R mean = ps_mean(mean_kind, p + nk, ts[s]);
        ps_put(mean + m_, mu, mu_lo, (size_t)s);
        ps_put(k0 - kk, var, var_lo, (size_t)s);
        s_mu[s] = (double)(PS_FABS(mean) + am);
        s_var[s] = (double)(k0 + PS_FABS(kk));
        free(ks);
    }
    free(alpha);
    ps_free(&f);
    return bad ? -1 : 0;
}
