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
// The search, both replays and every combination are mtg_pat_replay.h's, the code mtg_predict_at_eval_kernel calls in the
// same order: with every term selected and MTG_TERMS_MEAN the mask changes no generator, so the results are bit for bit
// the same because the two kernels run the same functions, not two copies kept in step.  Each (row, t*, mask) depends
// on nothing else of the call.
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"
#include "mtg_pat_replay.h"

// the generators A, B restricted to the slots of the mask's terms (0 elsewhere) -> k_c(0), summed as pat_load_coef sums k(0)
template <int J>
__device__ __forceinline__ double pterms_select(const PatCoef<J> &k, const int *own, uint32_t mask, const double *A, double *Am,
                                                const double *B, double *Bm)
{
#pragma clang fp contract(off)
    double k0 = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        const bool sel = (mask >> own[i]) & 1u;
        Am[i] = sel ? A[i] : 0.0;
        Bm[i] = sel ? B[i] : 0.0;
        if (sel && (i < k.NR || ((i - k.NR) & 1) == 0)) k0 += k.a[i];
    }
    return k0;
}

template <int J>
__global__ void __launch_bounds__(64) mtg_predict_terms_eval_kernel(MtgPredictTermsArgs a)
{
#pragma clang fp contract(off)
    constexpr int SY = J * (J + 1) / 2;
    __shared__ double park[PatParked<J>::DOUBLES];     // (S*, f*) of every lane while T, v hold (X*, g*)
    int64_t r, m;
    if (!pat_row_time(a.B, a.M, r, m)) return;
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
    const PatRow<J> w(a, r, e);
    const double ts = a.ts[slot];
    const int64_t n0 = pat_locate(w.dxt, w.N, ts);

    // one replay for all T components: forward to (S*, f*), parked; backward to (X*, g*) in the same registers
    double Us[J], Vs[J], ph[J], T[SY], v[J];
    double *mine = park + threadIdx.x;
    pat_generators<J>(k, ts, w.dxt[0].y, Us, Vs);
    if (n0 >= 0) {
        pat_replay_fwd<J>(k, w, n0, ts, T, v);
        PatParked<J>::park(mine, T, v);
    }
    const bool use_G = a.want_var && n0 >= 0;      // before the first sample the variance comes from the reversed sweep
    if (n0 < w.N - 1) pat_replay_bwd<J>(k, w, n0, ts, use_G, T, v, ph);
    const double mean = k.slope * ts + k.icpt;
    if (a.want_var && n0 < 0) {
        // S' of the reversed sweep goes where the (unused) X* would be, U' in place of U*: var_c* = k_c(0) - U'm^T S' U'm
        double phr[J], Ur[J];
        pat_reversed_at<J>(k, w, ts, phr, Ur);
#pragma unroll
        for (int i = 0; i < SY; ++i) T[i] = w.ckr[i];
        for (int c1 = 0; c1 < a.T; ++c1) {
            const uint32_t mask = a.masks[c1];
            double Wt[J], Urm[J];
            double var = pterms_select<J>(k, own, mask, Vs, Wt, Ur, Urm);
            double mu = (mask & MTG_TERMS_MEAN) ? mean : 0.0;
            if (n0 < w.N - 1) mu += pat_combine_wg<J>(Wt, v);
            var -= pat_combine_quad<J>(phr, T, Urm);
            mu_out[c1 * a.M] = mu;
            var_out[c1 * a.M] = var;
        }
        return;
    }
    for (int c1 = 0; c1 < a.T; ++c1) {
        const uint32_t mask = a.masks[c1];
        double Um[J], Wt[J];
        double var = pterms_select<J>(k, own, mask, Us, Um, Vs, Wt);
        double mu = (mask & MTG_TERMS_MEAN) ? mean : 0.0;
        if (n0 >= 0) {
            double uq, uf;
            pat_combine_before<J>(PatParked<J>{mine}, Um, Wt, uq, uf);
            mu += uf;
            var -= uq;
        }
        if (n0 < w.N - 1) {
            mu += pat_combine_wg<J>(Wt, v);
            if (use_G) var -= pat_combine_quad<J>(ph, T, Wt);
        }
        mu_out[c1 * a.M] = mu;
        if (a.want_var) var_out[c1 * a.M] = var;
    }
}

// a model without a celerite term (white noise only, J = 0): no term has a slot, every component is the mean or 0
__global__ void __launch_bounds__(64) mtg_predict_terms_white_eval_kernel(MtgPredictTermsArgs a)
{
#pragma clang fp contract(off)
    int64_t r, m;
    if (!pat_row_time(a.B, a.M, r, m)) return;
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
