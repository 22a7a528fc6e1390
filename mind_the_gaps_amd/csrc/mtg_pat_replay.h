// mtg_pat_replay.h -- the evaluation at a NEW time t* from what mtg_predict_at_factor_kernel has left of a row
// (notation and derivation: the header of mtg_predict_at.hip): which lane takes which (row, time), the search for n0,
// the checkpoints, the two replays to (S*, f*) and (X*, g*), and the J^2 combinations of them with the generators at
// t*.  Written once for mtg_predict_at_eval_kernel (all terms: the generators as they are, S* in registers) and
// mtg_predict_terms_eval_kernel (the generators masked per component, S* parked in LDS): the two call the same code in
// the same order, which is why all terms selected is bit for bit mtg_predict_at.  Everything is force-inlined, a
// template on the rank J, and rounds as written (no contraction), like the step functions it calls.
#pragma once
#include "mtg_factor_step.h"

// One lane per (row of the slab, entry of a list of M times), 64 times per workgroup: the grid is B ceil(M / 64).
// -> false for a lane beyond the list
__device__ __forceinline__ bool pat_row_time(int64_t B, int64_t M, int64_t &r, int64_t &m)
{
    const int64_t mblocks = (M + 63) / 64;
    r = (int64_t)blockIdx.x / mblocks;
    m = ((int64_t)blockIdx.x % mblocks) * 64 + threadIdx.x;
    return r < B && m < M;
}

// n0: the last sample with t_n <= t* (-1: none)
__device__ __forceinline__ int64_t pat_locate(const double2 *dxt, int64_t N, double ts)
{
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (dxt[mid].y <= ts) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// a checkpoint (S | G, f | g) as the factor stage stores it: the symmetric half, then the vector; the matrix is left
// alone where the variance is not wanted (it was not stored)
template <int J>
__device__ __forceinline__ void pat_ck_load(const double *c, double *S, double *f, bool with_S = true)
{
    constexpr int SY = J * (J + 1) / 2;
    if (with_S) {
#pragma unroll
        for (int i = 0; i < SY; ++i) S[i] = c[i];
    }
#pragma unroll
    for (int i = 0; i < J; ++i) f[i] = c[SY + i];
}

// what the factor stage has left of row r of the slab (row e of the batch)
template <int J>
struct PatRow {
    static constexpr int SY = J * (J + 1) / 2, CK = SY + J, stride = 3 * J + 3;
    int64_t N;
    const double2 *dxt;             // (dx, t) of its light curve
    const double *wk;               // [N][3 J + 3]: U, W, phi, D, z, x
    const double *ckf, *ckb, *ckr;  // checkpoints of (S, f) and (G, g); S + D W W^T of the reversed sweep

    __device__ __forceinline__ PatRow(const MtgPredictAtArgs &a, int64_t r, int64_t e)
        : N(a.N), dxt(a.dxt + (a.lc_index ? a.lc_index[e] : 0) * a.t_stride), wk(a.work + r * a.N * stride),
          ckf(a.ckf + r * a.nck * CK), ckb(a.ckb + r * a.nck * CK), ckr(a.ckr + r * SY)
    {
    }
};

// (S*, f*) at t* (n0 >= 0): the checkpoint at or before n0, the stored steps up to n0, then the partial step to t*
template <int J>
__device__ __forceinline__ void pat_replay_fwd(const PatCoef<J> &k, const PatRow<J> &w, int64_t n0, double ts, double *T, double *v)
{
#pragma clang fp contract(off)
    constexpr int stride = PatRow<J>::stride;
    const int64_t c0 = n0 / MTG_PAT_C;
    pat_ck_load<J>(w.ckf + c0 * PatRow<J>::CK, T, v);
    double ph[J], phs[J];
    pat_decay<J>(k, ts - w.dxt[n0].y, phs);
    for (int64_t n = c0 * MTG_PAT_C; n <= n0; ++n) {
        const double *s = w.wk + n * stride;
        double Wn[J];
#pragma unroll
        for (int i = 0; i < J; ++i) Wn[i] = s[J + i];
        if (n < n0) {
#pragma unroll
            for (int i = 0; i < J; ++i) ph[i] = s[stride + 2 * J + i];
        } else {
#pragma unroll
            for (int i = 0; i < J; ++i) ph[i] = phs[i];
        }
        pat_fwd_step<J>(T, v, ph, Wn, s[3 * J], s[3 * J + 1]);
    }
}

// (G_{n0+1} in T, g* in v) and psi, the partial decay from t* to sample n0 + 1 (n0 < N - 1): X* = psi psi^T o T.  The
// checkpoint at or after n0 + 1 (beyond the last sample: zero), the stored steps down to n0 + 1, then the partial step
// to t*.  Without use_G the matrix is neither loaded nor stepped.
template <int J>
__device__ __forceinline__ void pat_replay_bwd(const PatCoef<J> &k, const PatRow<J> &w, int64_t n0, double ts, bool use_G, double *T,
                                               double *v, double *psi)
{
#pragma clang fp contract(off)
    constexpr int SY = PatRow<J>::SY, stride = PatRow<J>::stride;
    const int64_t N = w.N, n1 = n0 + 1;
    int64_t p = (n1 + MTG_PAT_C - 1) / MTG_PAT_C * MTG_PAT_C;
    if (p < N) {
        pat_ck_load<J>(w.ckb + (p / MTG_PAT_C) * PatRow<J>::CK, T, v, use_G);
    } else {
        p = N;
#pragma unroll
        for (int i = 0; i < SY; ++i) T[i] = 0.0;
#pragma unroll
        for (int i = 0; i < J; ++i) v[i] = 0.0;
    }
    double Un[J];
    for (int64_t n = p - 1; n >= n1; --n) {
        const double *s = w.wk + n * stride;
        double xn = 0.0;
        if (n + 1 < N) {
#pragma unroll
            for (int i = 0; i < J; ++i) { Un[i] = s[stride + i]; psi[i] = s[stride + 2 * J + i]; }
            xn = s[stride + 3 * J + 2];
        } else {
#pragma unroll
            for (int i = 0; i < J; ++i) { Un[i] = 0.0; psi[i] = 0.0; }
        }
        pat_bwd_g<J>(v, psi, Un, xn);
        if (use_G) {
            double Um[J], Wm[J];
#pragma unroll
            for (int i = 0; i < J; ++i) { Um[i] = s[i]; Wm[i] = s[J + i]; }
            pat_bwd_G<J>(T, psi, Um, Wm, s[3 * J]);
        }
    }
    const double *s = w.wk + n1 * stride;
    pat_decay<J>(k, w.dxt[n1].y - ts, psi);
#pragma unroll
    for (int i = 0; i < J; ++i) Un[i] = s[i];
    pat_bwd_g<J>(v, psi, Un, s[3 * J + 2]);
}

// before the first sample (n0 < 0) the variance comes from the reversed sweep, where t* lies after the last sample:
// the decay phr from t* to the first sample and the reversed series' generators U' at t*
template <int J>
__device__ __forceinline__ void pat_reversed_at(const PatCoef<J> &k, const PatRow<J> &w, double ts, double *phr, double *Ur)
{
    double Vr[J];
    pat_decay<J>(k, w.dxt[0].y - ts, phr);
    pat_generators<J>(k, w.dxt[w.N - 1].y, ts, Ur, Vr);
}

// ---- where (S*, f*) is read from: the lane's registers, or the lane's column of an LDS park -------------------------
template <int J>
struct PatHeld {
    const double *S, *f;
    __device__ __forceinline__ double s(int i) const { return S[i]; }
    __device__ __forceinline__ double fv(int i) const { return f[i]; }
};

// element i of lane l at i * 64 + l: a lane reads only what it parked itself (no bank conflict, no barrier)
template <int J>
struct PatParked {
    static constexpr int SY = J * (J + 1) / 2, DOUBLES = (SY + J) * 64;
    const double *mine;             // the park, from this lane's element 0
    __device__ __forceinline__ double s(int i) const { return mine[i * 64]; }
    __device__ __forceinline__ double fv(int i) const { return mine[(SY + i) * 64]; }
    static __device__ __forceinline__ void park(double *mine, const double *S, const double *f)
    {
#pragma unroll
        for (int i = 0; i < SY; ++i) mine[i * 64] = S[i];
#pragma unroll
        for (int i = 0; i < J; ++i) mine[(SY + i) * 64] = f[i];
    }
};

// ---- the combinations: U, V are the generators at t*, as they are or masked to a component's slots -------------------
// up to n0:  q = S* U,  Wt -= q (Wt comes in as V),  uq = U^T q,  uf = U^T f*
// (pat_pivot's arithmetic, written out: U^T q is summed from 0 here, not taken off a pivot)
template <int J, class Held>
__device__ __forceinline__ void pat_combine_before(const Held &h, const double *U, double *Wt, double &uq, double &uf)
{
#pragma clang fp contract(off)
    uq = 0.0; uf = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) q += h.s(pat_sy(i, j)) * U[j];
        Wt[i] -= q;
        uq += U[i] * q;
        uf += U[i] * h.fv(i);
    }
}

// beyond n0:  wg = Wt^T g*
template <int J>
__device__ __forceinline__ double pat_combine_wg(const double *Wt, const double *g)
{
#pragma clang fp contract(off)
    double wg = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) wg += Wt[i] * g[i];
    return wg;
}

// w^T (ph ph^T o T) w:  beyond n0, Wt^T X* Wt with the partial decay psi and T = G_{n0+1};  before the first sample,
// U'^T S' U' with the decay to the first sample and T the reversed sweep's checkpoint
template <int J>
__device__ __forceinline__ double pat_combine_quad(const double *ph, const double *T, const double *w)
{
#pragma clang fp contract(off)
    double wxw = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) s += ph[i] * ph[j] * T[pat_sy(i, j)] * w[j];
        wxw += w[i] * s;
    }
    return wxw;
}
