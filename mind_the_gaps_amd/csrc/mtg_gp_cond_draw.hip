// mtg_gp_cond_draw.hip -- draws of the process GIVEN the data, at new times (celerite.GP.sample_conditional), by
// Matheron's rule in O((N + M) J^2) per draw: celerite forms the dense M x N cross-covariance and factors a dense
// M x M conditional covariance.
//
//   (y~, f*) ~ N(0, k(dt) + diag(sigma^2 + jitter | 0))   a joint prior draw at the epochs and at the new times
//   y*_cond  = f* + mean(t*) + k_*^T K^-1 ((y - y~) - mean(t))
//
// The second term is what mtg_predict_at computes for the light curve y - y~ (MtgPredictAtArgs::data): its kernels run
// unchanged behind the sweep of this file, which is the factor step of mtg_gp_draw.hip (y = L sqrt(D) q, same notation)
// on the MERGED series -- the N epochs and the Mu unique new times in ascending order, a new time equal to an epoch after
// it.  An epoch carries the diagonal sigma_n^2 + jitter and leaves y_n - y~_n; a new time carries the diagonal 0 and
// leaves the latent f*_u.  Its pivot k(0) - U^T S U is the conditional variance of the process there given the merged
// points before it: positive because the new times are unique and every epoch is noisy.  The merge is a comparison of
// the next epoch with the next new time inside the sweep, both held in registers: no table of the merged order exists,
// with one sampling or with one per light curve.  A rank-0 (white) model has no latent process: f* = 0 and no pivot at a new time.
//
// One lane per draw, the state in registers (a template on the rank J as mtg_gp_draw_kernel).  A lane stores one double
// per merged point into its own row, as the factor stage that follows stores 3 J + 3 of them per epoch into its own.
//
// Normals.  The caller's: row b holds the N epochs' normals, then one per entry of ts; a new time takes that of its
// first entry.  The device's: Philox4x32-10 keyed by the seed, counter (k, purpose, low word, high word of g) with g the
// draw's global index (mtg_set_stream_base) and
//     purpose MTG_PURPOSE_GP_COND_EPOCH = 13:  block k gives the Box-Muller pair of epochs 2k, 2k + 1
//     purpose MTG_PURPOSE_GP_COND_NEW   = 14:  block k gives the pair of the unique new times of rank 2k, 2k + 1
// so that a draw depends on (seed, g, theta, its light curve, the set of new times) alone: not on the batch, on slabs,
// or on the order of ts.  tests/gp_cond_draw_replay.py is the same in numpy.
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"
#include "mtg_pat_replay.h"
#include "mtg_sampler_dev.h"

template <int J, bool GIVEN>
__global__ void __launch_bounds__(64) mtg_gp_cond_draw_kernel(MtgGpCondDrawArgs a)
{
#pragma clang fp contract(off)
    constexpr int JA = J > 0 ? J : 1;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // row of this slab
    if (r >= a.B) return;
    const int64_t e = a.row0 + r;                                       // row of the batch
    if (a.status[e] != MTG_ST_OK) return;
    const int64_t N = a.N, Mu = a.Mu;
    const int64_t lc = a.lc_index ? a.lc_index[e] : 0;
    const double2 *yv = a.yv + lc * N, *dxt = a.dxt + lc * a.t_stride;
    double *data = a.data + r * N, *fs = a.fs + r * Mu;

    PatCoef<JA> k;
    pat_load_row<J>(a, e, k);
    PatState<JA> st;
    st.reset();
    const double t_first = dxt[0].y;
    // the next epoch (its time, y and sigma^2) and the next new time wait in registers, fetched as soon as the one before
    // is taken, so that the loads run under the step's arithmetic; +inf: none left (the times are finite)
    double te = t_first, tn = Mu > 0 ? a.tu[0] : INFINITY;
    double2 ye = yv[0];
    double tp = tn < te ? tn : te;                                      // the merged point before this one
    double qe0 = 0.0, qe1 = 0.0, qn0 = 0.0, qn1 = 0.0;
    bool bad = false;
    const uint64_t g = (uint64_t)(a.draw0 + e);                         // global index of this draw: random counters only

    int64_t n = 0, u = 0;
    while (n < N || u < Mu) {
        const bool fresh = tn < te;                                     // the next merged point is a new time
        const double t = fresh ? tn : te, yn = ye.x, dn = ye.y;
        double qi;
        if constexpr (GIVEN) {
            qi = a.normals[r * (N + a.M) + (fresh ? N + a.first[u] : n)];
        } else if (fresh) {
            if ((u & 1) == 0) philox_normal_pair((uint32_t)(u >> 1), MTG_PURPOSE_GP_COND_NEW, g, a.seed_lo, a.seed_hi, qn0, qn1);
            qi = (u & 1) ? qn1 : qn0;
        } else {
            if ((n & 1) == 0) philox_normal_pair((uint32_t)(n >> 1), MTG_PURPOSE_GP_COND_EPOCH, g, a.seed_lo, a.seed_hi, qe0, qe1);
            qi = (n & 1) ? qe1 : qe0;
        }
        const int64_t at = fresh ? u : n;
        if (fresh) { ++u; tn = u < Mu ? a.tu[u] : INFINITY; }
        else if (++n < N) { te = dxt[n].y; ye = yv[n]; }
        else te = INFINITY;
        double out = 0.0;
        if (J > 0 || !fresh) {
            double D = fresh ? 0.0 : dn + k.asum, uf = 0.0;
            if constexpr (J > 0) {
                if (fresh) D = k.k0;
                uf = st.advance(k, t - tp, t, t_first, D);
            }
            bad = bad || !(D > 0.0);
            const double v = sqrt(D) * qi;
            out = v + uf;
            st.leave(D, v);
            tp = t;
        }
        if (fresh) fs[at] = out;
        else data[at] = yn - out;
    }
    if (bad) a.status[e] = MTG_ST_NOTPD;
}

// y[r][m] = mu[r][inv[m]] + f*[r][inv[m]]: every entry of the caller's ts takes the value of its unique time
__global__ void __launch_bounds__(64) mtg_gp_cond_scatter_kernel(MtgGpCondDrawArgs a)
{
#pragma clang fp contract(off)
    int64_t r, m;
    if (!pat_row_time(a.B, a.M, r, m)) return;
    const int64_t u = a.inv[m];
    a.y[r * a.M + m] = a.status[a.row0 + r] == MTG_ST_OK ? a.mu[r * a.Mu + u] + a.fs[r * a.Mu + u] : NAN;
}

template <int J>
struct CondDrawLaunch {
    static void launch(const MtgGpCondDrawArgs &a, hipStream_t s)
    {
        const dim3 grid((unsigned)((a.B + 63) / 64)), block(64);
        if (a.normals) hipLaunchKernelGGL((mtg_gp_cond_draw_kernel<J, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mtg_gp_cond_draw_kernel<J, false>), grid, block, 0, s, a);
    }
};

// the sweep for rows [row0, row0 + B) of the batch; J = nr0 + 2 nc0 in 0 .. MTG_MAX_J (returns 0 otherwise)
int mtg_launch_gp_cond_draw(const MtgGpCondDrawArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J != 0) return pat_dispatch_rank<CondDrawLaunch>(J, a, s);
    CondDrawLaunch<0>::launch(a, s);
    return 1;
}

void mtg_launch_gp_cond_scatter(const MtgGpCondDrawArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mtg_gp_cond_scatter_kernel, dim3((unsigned)(a.B * ((a.M + 63) / 64))), dim3(64), 0, s, a);
}
