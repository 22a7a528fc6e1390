// mtg_epoch_fold.hip -- the epoch-folding periodogram (Leahy et al. 1983) and the phase-folded profiles of every resident
// light curve at a list of frequencies (mtg_epoch_fold and mtg_phase_fold of include/mtg.h).
//
// With the weights w_n, r_n = y_n - ybar, YY and sw of mtg_lomb_scargle.hip (the same pre-pass) and the phase bin
// b_n = floor(nbins frac(f (t_n - time_0))) of mtg_ls_phase.h, the product taken exactly:
//   W_b = sum_{n in b} w_n, S_b = sum_{n in b} w_n r_n,   p = sum_{b : W_b > 0} S_b^2 / W_b
// -- p = YY - chi^2 of the best profile that is constant on every bin, the quantity ls_normalize turns into the four
// normalisations.
//
// One lane owns a frequency; the workgroup walks the samples in the chunks mtg_ls_tile.h stages, every lane reading the
// same sample.  The bin is known only at run time, so the sums are kept in LDS as [bin][lane] (mtg_ef_plan.h: layout,
// banks, tile and lanes): per sample one bin index for the tile and one 16-byte read-modify-write per light curve
// (weighted) or per pair of light curves and 8 bytes for the tile's W (weights 1 / N).  A lane touches its own entries
// only: no atomics, and no barrier but the chunk's.
//
// Order.  Samples ascending into the bin's running sum, one addition each; then the bins ascending.  The arithmetic of
// one (light curve, frequency) is the same in every instantiation: a power depends on (light curve, frequency, nbins,
// time_0, normalization, weighted) alone, and is what the formula gives from the stored wsum and wrsum bit for bit.
// No scratch: profiles/epoch_fold_resources.txt.  The C entries, with the other entries' call helpers: mtg_capi.hip.
#include "mtg_ls_tile.h"
#include "mtg_ef_plan.h"

static_assert(MTG_EF_CHUNK == MTG_LS_CHUNK, "mtg_ef_plan.h budgets the chunk mtg_ls_tile.h stages");

namespace {

enum { EF_MAX_LANES = 256, EF_AUX_LANES = 64, EF_MAX_BINS = 32 };

struct MtgEfArgs {
    MtgLsArgs a;             // (power NULL: the bins alone)
    int nbins;
    double time_0;
    double *wsum, *wrsum;    // NULL or [Ls][F][nbins] of this slab
};

// R light curves per lane; WEIGHTED: weights from the light curve's own sigma, else 1 / N (W is the tile's)
template <int R, bool WEIGHTED>
__global__ void __launch_bounds__(EF_MAX_LANES)
mtg_epoch_fold_kernel(const MtgEfArgs g)
{
#pragma clang fp contract(off)
    static_assert(WEIGHTED || R == 1 || R % 2 == 0, "the unweighted chunk is staged as pairs of light curves");
    constexpr int CH = MTG_LS_CHUNK;
    constexpr bool OWN_W = WEIGHTED || R == 1;         // (W, S) per light curve; else W per tile and S as pairs
    constexpr int NT = WEIGHTED ? R : 1;
    constexpr int NP = WEIGHTED ? R : (R + 1) / 2;     // 16-byte columns of the chunk, and of the sums
    __shared__ double te_s[CH];
    __shared__ double2 col_s[NP * CH];
    extern __shared__ __attribute__((aligned(16))) double2 acc[];   // [NP][nbins][lanes], then OWN_W ? nothing : W [nbins][lanes]

    const MtgLsArgs &a = g.a;
    const int nb = g.nbins, T = blockDim.x, lane = threadIdx.x;
    double *const wt_s = reinterpret_cast<double *>(acc + NP * nb * T);
    LsLane q;
    q.locate<R>(a);
    q.t0 = g.time_0;   // elapsed times from the call's epoch, not from the tile's first sample

    for (int e = 0; e < NP * nb; ++e) acc[e * T + lane] = make_double2(0.0, 0.0);
    if (!OWN_W)
        for (int b = 0; b < nb; ++b) wt_s[b * T + lane] = 0.0;

    for (int64_t n0 = 0; n0 < a.N; n0 += CH) {
        const int len = (int)(a.N - n0 < CH ? a.N - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: nothing)
        ls_stage_chunk<R, WEIGHTED>(a, q, n0, len, te_s, col_s);
        __syncthreads();
        for (int i = 0; i < len; ++i) {
            double wt[NT], wr[R];
            const int at = mtg_cycles_bin(q.f, te_s[i], nb) * T + lane;
            ls_read_sample<R, WEIGHTED>(col_s, i, q.w0, wt, wr);
            if (OWN_W) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    double2 v = acc[j * nb * T + at];
                    v.x += wt[WEIGHTED ? j : 0];
                    v.y += wr[j];
                    acc[j * nb * T + at] = v;
                }
            } else {
                wt_s[at] += wt[0];
#pragma unroll
                for (int j = 0; j < R / 2; ++j) {
                    double2 v = acc[j * nb * T + at];
                    v.x += wr[2 * j];
                    v.y += wr[2 * j + 1];
                    acc[j * nb * T + at] = v;
                }
            }
        }
    }

    if (q.k >= a.F) return;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= q.nl) continue;
        const int64_t row = (q.lt - a.l0 + j) * a.F + q.k;
        double p = 0.0;
        for (int b = 0; b < nb; ++b) {
            double W, S;
            if (OWN_W) {
                const double2 v = acc[(j * nb + b) * T + lane];
                W = v.x; S = v.y;
            } else {
                const double2 v = acc[(j / 2 * nb + b) * T + lane];
                W = wt_s[b * T + lane]; S = j % 2 ? v.y : v.x;
            }
            if (g.wsum) g.wsum[row * nb + b] = W;
            if (g.wrsum) g.wrsum[row * nb + b] = S;
            if (W > 0.0) p = p + (S * S) / W;
        }
        if (a.power) {
            const double4 st = a.stats[q.lt + j];
            a.power[row] = ls_normalize(p, st.y, st.z, a.normalization);
        }
    }
}

// count and sum of sigma^2 of every bin: one lane per frequency, one row of workgroups per light curve of the slab, the
// samples read from global memory (every lane the same one).  For the handful of frequencies of mtg_phase_fold.
__global__ void __launch_bounds__(EF_AUX_LANES)
mtg_phase_fold_counts_kernel(const MtgEfArgs g, int64_t *__restrict__ count, double *__restrict__ varsum)
{
#pragma clang fp contract(off)
    __shared__ double vs[EF_MAX_BINS * EF_AUX_LANES];
    __shared__ int cs[EF_MAX_BINS * EF_AUX_LANES];
    const MtgLsArgs &a = g.a;
    const int nb = g.nbins, lane = threadIdx.x;
    const int64_t l = a.l0 + blockIdx.y, k = (int64_t)blockIdx.x * EF_AUX_LANES + lane;
    const double f = a.freqs[k < a.F ? k : a.F - 1];
    const double2 *dxt = a.dxt + l * a.t_stride, *yv = a.yv + l * a.N;
    for (int b = 0; b < nb; ++b) { vs[b * EF_AUX_LANES + lane] = 0.0; cs[b * EF_AUX_LANES + lane] = 0; }
    for (int64_t n = 0; n < a.N; ++n) {
        const int at = mtg_cycles_bin(f, dxt[n].y - g.time_0, nb) * EF_AUX_LANES + lane;
        vs[at] += yv[n].y;
        cs[at] += 1;
    }
    if (k >= a.F) return;
    const int64_t row = ((l - a.l0) * a.F + k) * nb;
    for (int b = 0; b < nb; ++b) {
        if (count) count[row + b] = cs[b * EF_AUX_LANES + lane];
        if (varsum) varsum[row + b] = vs[b * EF_AUX_LANES + lane];
    }
}

template <int R, bool WEIGHTED>
hipError_t ef_launch(const MtgEfArgs &g, const MtgEfPlan &plan, int64_t blocks, hipStream_t s)
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mtg_epoch_fold_kernel<R, WEIGHTED>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)MTG_EF_LDS_BUDGET);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mtg_epoch_fold_kernel<R, WEIGHTED>), dim3((unsigned)blocks), dim3(plan.lanes), (size_t)plan.acc_bytes, s, g);
    return hipGetLastError();
}

}  // namespace

hipError_t mtg_launch_epoch_fold(const MtgEpochFoldArgs &q, const MtgEfPlan &plan, int64_t l0, int64_t Ls, hipStream_t s)
{
    const MtgLombScargleArgs &ls = q.ls;
    if (q.nbins < 2 || q.nbins > EF_MAX_BINS || plan.lanes > EF_MAX_LANES || plan.lds_bytes > MTG_EF_LDS_BUDGET) return hipErrorInvalidValue;
    const int R = plan.tile;
    const int64_t nfb = (ls.F + plan.lanes - 1) / plan.lanes, tiles = (Ls + R - 1) / R;
    if (nfb > 0x7fffffff / tiles) return hipErrorInvalidValue;
    MtgEfArgs g;
    g.a = mtg_ls_args(ls, l0, Ls, nfb);
    g.nbins = q.nbins; g.time_0 = q.time_0; g.wsum = q.wsum; g.wrsum = q.wrsum;
    hipError_t e = hipSuccess;
    if (ls.power || q.wsum || q.wrsum) {
        const int64_t blocks = nfb * tiles;
        if (ls.weighted) e = R == 1 ? ef_launch<1, true>(g, plan, blocks, s) : R == 2 ? ef_launch<2, true>(g, plan, blocks, s) : ef_launch<4, true>(g, plan, blocks, s);
        else e = R == 1 ? ef_launch<1, false>(g, plan, blocks, s) : R == 2 ? ef_launch<2, false>(g, plan, blocks, s) : ef_launch<4, false>(g, plan, blocks, s);
        if (e != hipSuccess) return e;
    }
    if (q.count || q.varsum) {
        const int64_t cols = (ls.F + EF_AUX_LANES - 1) / EF_AUX_LANES;
        if (cols > 0x7fffffff || Ls > 65535) return hipErrorInvalidValue;
        hipLaunchKernelGGL(mtg_phase_fold_counts_kernel, dim3((unsigned)cols, (unsigned)Ls), dim3(EF_AUX_LANES), 0, s, g, q.count, q.varsum);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (ls.power) {   // (the Lomb-Scargle launcher's reduction of a slab's rows)
        mtg_launch_lomb_scargle_peaks(ls, l0, Ls, s);
        e = hipGetLastError();
    }
    return e;
}
