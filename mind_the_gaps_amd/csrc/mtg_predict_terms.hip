// mtg_predict_terms.hip -- conditional mean / variance at new times of ONE COMPONENT k_c of the sum kernel given the
// data (celerite.GP.predict(y, t, kernel=k_c)), for T components at once:
//   mu_c*  = [mean(t*)] + k_c(t*, t) K^-1 r,     var_c* = k_c(0) - k_c,*^T K^-1 k_c,*,     K the covariance of the WHOLE model.
// celerite forms the dense M x N cross-covariance of the sub-kernel.  In the notation of mtg_predict_at.hip's header the
// row k_c,* is what the generators at t* make of it: restricted to the slots of the selected terms,
//   Um = U* on selected slots, 0 elsewhere;  Vm likewise;  k_c(0) = sum of a over the selected slots
//   q = S* Um,  Wt = Vm - q
//   mu_c*  = [mean(t*)] + Um^T f* + Wt^T g*
//   var_c* = k_c(0) - Um^T q - Wt^T X* Wt       (before the first sample: k_c(0) - Urm^T S' Urm of the reversed sweep)
// while S*, f*, X*, g* -- the factorisation, the checkpoints and both replays -- belong to K and do not know the mask.
// The first stage is mtg_predict_at's own (mtg_launch_predict_at_factor).  The evaluation stage below is one lane per
// (row, t*) like mtg_predict_at_eval_kernel and replays ONCE: forward to (S*, f*), which it parks in LDS (S* and X*
// share registers, as there), backward to (X*, g*), then a loop over the T masks of J^2 work each, S* read back from LDS.
// A lane reads only what it parked itself (element i of lane l at i * 64 + l: no bank conflict, no barrier).
// Which slot belongs to which term comes from the expansion (mtg_prepare.h, OWNER), per row: an over-damped SHO term
// owns two real slots, an under-damped one a complex pair.
// With every term selected and MTG_TERMS_MEAN the operations and their order are mtg_predict_at_eval_kernel's: the
// results are bit for bit the same.  Each (row, t*, mask) depends on nothing else of the call.
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"

template <int J>
__global__ void __launch_bounds__(64) mtg_predict_terms_eval_kernel(MtgPredictTermsArgs a)
{
#pragma clang fp contract(off)
    constexpr int SY = J * (J + 1) / 2, CK = SY + J, stride = 3 * J + 3;
    __shared__ double park[CK * 64];                   // (S*, f*) of every lane while T, v hold (X*, g*)
    const int lane = threadIdx.x;
    const int64_t mblocks = (a.M + 63) / 64;
    const int64_t r = (int64_t)blockIdx.x / mblocks;
    const int64_t m = ((int64_t)blockIdx.x % mblocks) * 64 + threadIdx.x;
    if (r >= a.B || m >= a.M) return;
    const int64_t e = a.row0 + r;
    const int64_t slot = a.order ? a.order[m] : m;     // the times are visited in ascending order, stored where they were given
    double *mu_out = a.mu + r * a.T * a.M + slot;      // [T] of stride M
    double *var_out = a.want_var ? a.var + r * a.T * a.M + slot : nullptr;
    if (a.status[e] != MTG_ST_OK) {
        for (int c = 0; c < a.T; ++c) {
            mu_out[c * a.M] = NAN;
            if (a.want_var) var_out[c * a.M] = NAN;
        }
        return;
    }
    PatCoef<J> k;
    pat_load_coef<J>(a, e, k);
    int own[J];                                        // the term of every slot of this row
#pragma unroll
    for (int i = 0; i < J; ++i)
        own[i] = a.owner[(int64_t)(i < k.NR ? i : a.lay.nr_max + ((i - k.NR) >> 1)) * a.cstride + e];
    const int64_t lc = a.lc_index ? a.lc_index[e] : 0;
    const int64_t N = a.N;
    const double2 *dxt = a.dxt + lc * a.t_stride;
    const double *wk = a.work + r * N * stride;
    const double *ckf = a.ckf + r * a.nck * CK, *ckb = a.ckb + r * a.nck * CK;
    const double ts = a.ts[slot];

    // n0: the last sample with t_n <= t* (-1: none)
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (dxt[mid].y <= ts) lo = mid + 1; else hi = mid;
    }
    const int64_t n0 = lo - 1;

    double Us[J], Vs[J], ph[J], T[SY], v[J];
    pat_generators<J>(k, ts, dxt[0].y, Us, Vs);
    if (n0 >= 0) {
        // (S, f) of the checkpoint at or before n0, the stored steps up to n0, then the partial step to t*
        const int64_t c0 = n0 / MTG_PAT_C;
        const double *c = ckf + c0 * CK;
#pragma unroll
        for (int i = 0; i < SY; ++i) T[i] = c[i];
#pragma unroll
        for (int i = 0; i < J; ++i) v[i] = c[SY + i];
        double phs[J];
        pat_decay<J>(k, ts - dxt[n0].y, phs);
        for (int64_t n = c0 * MTG_PAT_C; n <= n0; ++n) {
            const double *w = wk + n * stride;
            double Wn[J];
#pragma unroll
            for (int i = 0; i < J; ++i) Wn[i] = w[J + i];
            if (n < n0) {
#pragma unroll
                for (int i = 0; i < J; ++i) ph[i] = w[stride + 2 * J + i];
            } else {
#pragma unroll
                for (int i = 0; i < J; ++i) ph[i] = phs[i];
            }
            pat_fwd_step<J>(T, v, ph, Wn, w[3 * J], w[3 * J + 1]);
        }
#pragma unroll
        for (int i = 0; i < SY; ++i) park[i * 64 + lane] = T[i];
#pragma unroll
        for (int i = 0; i < J; ++i) park[(SY + i) * 64 + lane] = v[i];
    }
    const bool use_G = a.want_var && n0 >= 0;      // before the first sample the variance comes from the reversed sweep
    if (n0 < N - 1) {
        // (G, g) of the checkpoint at or after n0 + 1 (beyond the last sample: zero), the stored steps down to n0 + 1,
        // then the partial step to t*
        const int64_t n1 = n0 + 1;
        int64_t p = (n1 + MTG_PAT_C - 1) / MTG_PAT_C * MTG_PAT_C;
        if (p < N) {
            const double *c = ckb + (p / MTG_PAT_C) * CK;
            if (use_G) {
#pragma unroll
                for (int i = 0; i < SY; ++i) T[i] = c[i];
            }
#pragma unroll
            for (int i = 0; i < J; ++i) v[i] = c[SY + i];
        } else {
            p = N;
#pragma unroll
            for (int i = 0; i < SY; ++i) T[i] = 0.0;
#pragma unroll
            for (int i = 0; i < J; ++i) v[i] = 0.0;
        }
        double Un[J];
        for (int64_t n = p - 1; n >= n1; --n) {
            const double *w = wk + n * stride;
            double xn = 0.0;
            if (n + 1 < N) {
#pragma unroll
                for (int i = 0; i < J; ++i) { Un[i] = w[stride + i]; ph[i] = w[stride + 2 * J + i]; }
                xn = w[stride + 3 * J + 2];
            } else {
#pragma unroll
                for (int i = 0; i < J; ++i) { Un[i] = 0.0; ph[i] = 0.0; }
            }
            pat_bwd_g<J>(v, ph, Un, xn);
            if (use_G) {
                double Um[J], Wm[J];
#pragma unroll
                for (int i = 0; i < J; ++i) { Um[i] = w[i]; Wm[i] = w[J + i]; }
                pat_bwd_G<J>(T, ph, Um, Wm, w[3 * J]);
            }
        }
        const double *w = wk + n1 * stride;
        pat_decay<J>(k, dxt[n1].y - ts, ph);           // psi: X* = psi psi^T o T
#pragma unroll
        for (int i = 0; i < J; ++i) Un[i] = w[i];
        pat_bwd_g<J>(v, ph, Un, w[3 * J + 2]);
    }
    const bool reversed = a.want_var && n0 < 0;
    if (reversed) {
        // seen from the other end t* lies after the last sample of the reversed series: var* = k(0) - U'^T S' U';
        // S' = phr phr^T o the reversed sweep's checkpoint goes where the (unused) X* would be, U' in place of V'
        const double *c = a.ckr + r * SY;
        double phr[J], Vr[J];
        pat_decay<J>(k, dxt[0].y - ts, phr);
#pragma unroll
        for (int i = 0; i < J; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) T[pat_sy(i, j)] = c[pat_sy(i, j)];
        double Ur[J];
        pat_generators<J>(k, dxt[N - 1].y, ts, Ur, Vr);
        const double mean = k.slope * ts + k.icpt;
        for (int c1 = 0; c1 < a.T; ++c1) {
            const uint32_t mask = a.masks[c1];
            double Wt[J], Urm[J], var = 0.0;
#pragma unroll
            for (int i = 0; i < J; ++i) {
                const bool sel = (mask >> own[i]) & 1u;
                Wt[i] = sel ? Vs[i] : 0.0;
                Urm[i] = sel ? Ur[i] : 0.0;
                if (sel && (i < k.NR || ((i - k.NR) & 1) == 0)) var += k.a[i];
            }
            double mu = (mask & MTG_TERMS_MEAN) ? mean : 0.0;
            if (n0 < N - 1) {
                double wg = 0.0;
#pragma unroll
                for (int i = 0; i < J; ++i) wg += Wt[i] * v[i];
                mu += wg;
            }
            double usu = 0.0;
#pragma unroll
            for (int i = 0; i < J; ++i) {
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < J; ++j) q += phr[i] * phr[j] * T[pat_sy(i, j)] * Urm[j];
                usu += Urm[i] * q;
            }
            var -= usu;
            mu_out[c1 * a.M] = mu;
            var_out[c1 * a.M] = var;
        }
        return;
    }
    const double mean = k.slope * ts + k.icpt;
    for (int c1 = 0; c1 < a.T; ++c1) {
        const uint32_t mask = a.masks[c1];
        double Um[J], Wt[J], var = 0.0;
#pragma unroll
        for (int i = 0; i < J; ++i) {
            const bool sel = (mask >> own[i]) & 1u;
            Um[i] = sel ? Us[i] : 0.0;
            Wt[i] = sel ? Vs[i] : 0.0;
            if (sel && (i < k.NR || ((i - k.NR) & 1) == 0)) var += k.a[i];     // k_c(0), summed as pat_load_coef sums k(0)
        }
        double mu = (mask & MTG_TERMS_MEAN) ? mean : 0.0;
        if (n0 >= 0) {
            // (pat_pivot's arithmetic, written out, as in mtg_predict_at_eval_kernel)
            double uq = 0.0, uf = 0.0;
#pragma unroll
            for (int i = 0; i < J; ++i) {
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < J; ++j) q += park[pat_sy(i, j) * 64 + lane] * Um[j];
                Wt[i] -= q;
                uq += Um[i] * q;
                uf += Um[i] * park[(SY + i) * 64 + lane];
            }
            mu += uf;
            var -= uq;
        }
        if (n0 < N - 1) {
            double wg = 0.0;
#pragma unroll
            for (int i = 0; i < J; ++i) wg += Wt[i] * v[i];
            mu += wg;
            if (use_G) {
                double wxw = 0.0;
#pragma unroll
                for (int i = 0; i < J; ++i) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < J; ++j) s += ph[i] * ph[j] * T[pat_sy(i, j)] * Wt[j];
                    wxw += Wt[i] * s;
                }
                var -= wxw;
            }
        }
        mu_out[c1 * a.M] = mu;
        if (a.want_var) var_out[c1 * a.M] = var;
    }
}

// a model without a celerite term (white noise only, J = 0): no term has a slot, every component is the mean or 0
__global__ void __launch_bounds__(64) mtg_predict_terms_white_eval_kernel(MtgPredictTermsArgs a)
{
#pragma clang fp contract(off)
    const int64_t mblocks = (a.M + 63) / 64;
    const int64_t r = (int64_t)blockIdx.x / mblocks;
    const int64_t m = ((int64_t)blockIdx.x % mblocks) * 64 + threadIdx.x;
    if (r >= a.B || m >= a.M) return;
    const int64_t e = a.row0 + r;
    const bool ok = a.status[e] == MTG_ST_OK;
    const double slope = a.coef[a.lay.mean(0) * a.cstride + e], icpt = a.coef[a.lay.mean(1) * a.cstride + e];
    const double mean = slope * a.ts[m] + icpt;
    for (int c = 0; c < a.T; ++c) {
        const int64_t o = (r * a.T + c) * a.M + m;
        a.mu[o] = !ok ? NAN : (a.masks[c] & MTG_TERMS_MEAN) ? mean : 0.0;
        if (a.want_var) a.var[o] = ok ? 0.0 : NAN;
    }
}

template <int J>
struct PtermsLaunch {
    static void launch(const MtgPredictTermsArgs &a, hipStream_t s)
    {
        hipLaunchKernelGGL(mtg_predict_terms_eval_kernel<J>, dim3((unsigned)(a.B * ((a.M + 63) / 64))), dim3(64), 0, s, a);
    }
};

// the evaluation stage for rows [row0, row0 + B) of the batch; J = nr0 + 2 nc0 in 0 .. MTG_MAX_J (returns 0 otherwise)
int mtg_launch_predict_terms_eval(const MtgPredictTermsArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J != 0) return pat_dispatch_rank<PtermsLaunch>(J, a, s);
    hipLaunchKernelGGL(mtg_predict_terms_white_eval_kernel, dim3((unsigned)(a.B * ((a.M + 63) / 64))), dim3(64), 0, s, a);
    return 1;
}
