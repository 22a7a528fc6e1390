// mtg_device.h -- data structures shared by the host side of the C-ABI and the
// gfx950 kernels.  Written for MI355X (CDNA4, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/mtg.h"

// Measurement knobs (kernel A/B experiments: scripts/build_variant.sh compiles with -DMTG_MEASURE).  The shipped library
// reads NO environment variable: every switch a user may touch is an mtg_set_* entry of include/mtg.h, and nothing that
// can change the bits of a result (the rank-10 chunk count, ...) hangs on the environment of the process.
#ifdef MTG_MEASURE
#include <stdlib.h>
static inline const char *mtg_measure_env(const char *name) { return getenv(name); }
#else
static inline const char *mtg_measure_env(const char *) { return nullptr; }
#endif

// What celerite.GP(kernel, mean, fit_mean) holds (reference gpmodelling.py:51),
// flattened so that it travels as a kernel argument (scalar loads only).
struct MtgModel {
    int nterms;
    int mean_kind;
    int PF;      // full parameter vector length (kernel + mean)
    int P;       // free parameters = length of one theta row
    int nk;      // kernel parameters (mean parameters start here)
    int nsho;    // SHOTerm count: each may expand to 1 complex or 2 real terms
    int nr0, nc0;        // structure with every SHO under-damped (Q >= 1/2)
    int nr_max, nc_max;  // widest real / complex expansion (workspace layout)
    int last_b0;         // the last complex slot always holds a term with b = 0 (Lorentzian, ComplexTerm3, Cosinus)
    int kinds[MTG_MAX_TERMS];
    int poff[MTG_MAX_TERMS];
    int src[MTG_MAX_PARAMS];  // theta column feeding full[k], or -1 = frozen
    double defaults[MTG_MAX_PARAMS];
    double lo[MTG_MAX_PARAMS];
    double hi[MTG_MAX_PARAMS];
    double extra[MTG_MAX_TERMS];
};

// Coefficient workspace: structure-of-arrays, one column per evaluation so that
// lane e reads/writes coef[slot * stride + e] (coalesced).  Slots:
//   a_real[nr_max] c_real[nr_max] a_comp[nc_max] b_comp[nc_max] c_comp[nc_max]
//   d_comp[nc_max] asum(= sum a + jitter) mean_slope mean_intercept jitter
// and, for a model with a profile mean only (mtg_mean.h), that mean's further per-row constants after them
struct MtgCoefLayout {
    int nr_max, nc_max;
    __host__ __device__ int ar(int j) const { return j; }
    __host__ __device__ int cr(int j) const { return nr_max + j; }
    __host__ __device__ int ac(int k) const { return 2 * nr_max + k; }
    __host__ __device__ int bc(int k) const { return 2 * nr_max + nc_max + k; }
    __host__ __device__ int cc(int k) const { return 2 * nr_max + 2 * nc_max + k; }
    __host__ __device__ int dc(int k) const { return 2 * nr_max + 3 * nc_max + k; }
    __host__ __device__ int asum() const { return 2 * nr_max + 4 * nc_max; }
    __host__ __device__ int mean(int i) const { return 2 * nr_max + 4 * nc_max + 1 + i; }
    __host__ __device__ int jit() const { return 2 * nr_max + 4 * nc_max + 3; }
    __host__ __device__ int nslots() const { return 2 * nr_max + 4 * nc_max + 4; }
    // profile means (MTG_MEAN_SINE, _TWOSINE, _GAUSSIAN): constant i of mtg_mean_derive, behind every slot above
    __host__ __device__ int mean_extra(int i) const { return nslots() + i; }
};

struct MtgPrepArgs {
    MtgModel model;
    const double *theta;  // [B][P]
    int64_t B;
    int add_prior;
    double *coef;
    int64_t cstride;
    int nsig;       // number of structure signatures (nsho + 1); 1 = identity mapping
    int *lists;     // [nsig][cstride] evaluation indices grouped by signature
    int *counts;    // [nsig]
    double *out;    // [B]
    int32_t *status;  // [B]
    int32_t *sig;   // [B] number of over-damped SHO terms per evaluation, or NULL
    // a walker-sharded ensemble expands and solves only rows [row_lo, row_hi); the others get MTG_ST_REMOTE
    // (skipped by every solver like a prior rejection) until the all-gather brings the owner's result
    int64_t row_lo = 0, row_hi = INT64_MAX;
};

// status of a row another rank evaluates (internal: never visible after the exchange)
#define MTG_ST_REMOTE 4

struct MtgSolveArgs {
    const double *coef;
    int64_t cstride;
    MtgCoefLayout lay;
    const int *list;       // NULL = identity mapping
    const int *count_ptr;  // NULL = B
    int64_t B;
    const int32_t *lc_index;  // NULL = light curve 0
    int32_t *status;
    double *out;
    const double2 *dxt;  // [N] or [L][N] pairs (dx_n, t_n), dx_0 = 0
    const double2 *yv;   // [L][N] pairs (y_n, sigma_n^2 = yerr_n^2)
    int64_t N;
    int64_t t_stride;    // 0 (shared sampling) or N
    uint64_t yv_bytes;   // L * N * 16: may exceed 4 GiB (the sweep windows its 32-bit offsets per wave)
    uint64_t dxt_bytes;
    uint64_t window_bytes;  // reach of one buffer descriptor, <= 2^32 - 1 (smaller only in tests)
    // resident sets beyond the window: evaluations a wave cannot reach from its first light curve are
    // appended to left_list (count in *left_count) and swept by a second launch with solo = 1, one
    // evaluation per wave; NULL when the whole set lies inside one window
    int *left_list;
    int *left_count;
    int solo;
    const double *dxmax;  // [1] max_n dx_n (device): decides table vs OCML sincos per wave
    int mean_kind;
    int has_mean;  // 0: the mean is identically zero for every evaluation of this launch and the model has no jitter term
    // time-parallel path of the rank-10 structures only (mtg_tp_big.h): workspace laid out by
    // mtg_tp_big_plan(J, B, tp_chunks) and the number of chunks per evaluation; NULL / 0 otherwise
    double *tp_ws;
    int tp_chunks;
    int tp_gsize;   // elements per scan group (mtg_tp_big_gsize)
    int tp_direct;  // likelihood without the filter pass (mtg_tp_big.h)
    int tp_nr0, tp_nc0;    // structure with no over-damped SHO term; evaluation ev has (tp_nr0 + 2 sig[ev], tp_nc0 - sig[ev])
    const int32_t *sig;    // [B] over-damped SHO terms per evaluation (mtg_prepare_one), or NULL = 0
    // serial sweep in sorted order (mtg_sort.hip): `list` is the whole batch sorted by (structure, light curve) and
    // this launch takes the seg_k-th segment of it, which starts after seg_counts[0 .. seg_k); NULL: list starts at 0
    const int *seg_counts = nullptr;
    int seg_k = 0;
    // the context's resident copy of the exp2 / (cos, sin) tables (struct MtgMathTablesT<true> of mtg_math.h, made once by
    // mtg_launch_tables): the time-parallel kernels copy it into LDS instead of computing it per workgroup; NULL: computed
    const void *tables = nullptr;
};

// fills `tables` (sizeof(MtgMathTablesT<true>) bytes of device memory) -- mtg_timeparallel.hip
void mtg_launch_tables(void *tables, hipStream_t stream);
size_t mtg_tables_bytes();

// doubles per filtering element (A | b | eta | C | Jm | five likelihood scalars) of the time-parallel kernel,
// rounded up to an odd number: lane l's element starts l * MTG_TP_ELEM doubles into LDS, and an even stride
// puts many lanes on the same bank (rank 3 would be 32 doubles: all 64 lanes on ONE bank, every access
// serialised 64-fold -- measured as 5.6 us per scan round instead of ~1)
#define MTG_TP_ELEM(J) (((J) * (J) + 2 * (J) + (J) * ((J) + 1) + 5) | 1)

// What every per-row entry (mtg_predict, mtg_predict_at, mtg_gp_draw, mtg_loglike_grad, mtg_apply_inverse) hands its
// kernels: the expanded coefficients of the whole batch and the resident light curves (RowCall::expand of mtg_capi.hip
// fills it)
struct MtgRowArgs {
    const double *coef;     // SoA coefficient workspace (mtg_prepare_kernel), indexed by the row of the batch
    int64_t cstride;
    MtgCoefLayout lay;
    int nr0, nc0;           // structure with no over-damped SHO term
    const int32_t *sig;     // [batch] over-damped SHO terms of each evaluation
    int64_t row0, B;        // this launch takes rows [row0, row0 + B) of the batch (a slab)
    const int32_t *lc_index;
    int32_t *status;        // [batch] prior verdict from prepare on entry; MTG_ST_NOTPD added by the factorisation
    const double2 *dxt, *yv;
    int64_t N, t_stride;
};

struct MtgPredictArgs : MtgRowArgs {   // the whole batch in one launch: row0 = 0
    double *work;           // [B][N][3 J + 2]: U, W, phi (per slot), D, z
    double *mu, *var;       // [B][N]
};
void mtg_launch_predict(const MtgPredictArgs &, hipStream_t);

// samples between two checkpoints of the new-time prediction (mtg_predict_at.hip): a new time replays at most this
// many stored steps in each direction; the checkpoints take N J^2 / C doubles per row
#ifndef MTG_PAT_C
#define MTG_PAT_C 64
#endif

struct MtgPredictAtArgs : MtgRowArgs {
    double *work;           // [B][N][3 J + 3]: U, W, phi (per slot), D, z, x = (K^-1 r)_n
    int64_t nck;            // checkpoints per row: ceil(N / MTG_PAT_C)
    double *ckf, *ckb;      // [B][nck][J (J + 1) / 2 + J]: (S_n, f_n) and (G_n, g_n) at n = k MTG_PAT_C
    double *ckr;            // [B][J (J + 1) / 2]: S + D W W^T after the first sample of the time-reversed factorisation
    int want_var;           // 0: mean only (G is neither swept nor stored)
    int64_t M;
    const double *ts;       // [M] new times
    const int64_t *order;   // [M] ts in ascending order (indices into ts), or NULL: ts is ascending as given
    double *mu, *var;       // [B][M]
    const double *data;     // [B][N] of this slab: read in place of the resident data y (mtg_gp_cond_draw), or NULL
};
// both stages of the new-time prediction for one slab; 0 = rank outside 0 .. MTG_MAX_J
int mtg_launch_predict_at(const MtgPredictAtArgs &, hipStream_t);
// the first stage alone (factorisation, checkpoints, reversed sweep), for an evaluation stage of the caller's own
int mtg_launch_predict_at_factor(const MtgPredictAtArgs &, hipStream_t);

// Per-term conditional mean / variance at new times (mtg_predict_terms.hip): mtg_predict_at's workspace and first stage,
// then an evaluation stage that restricts the generators at t* to the slots of each mask's terms
struct MtgPredictTermsArgs : MtgPredictAtArgs {   // mu, var: [B][T][M] of this slab
    int T;                      // masks, 1 .. 32
    const uint32_t *masks;      // [T]: bit k = term k of the model, MTG_TERMS_MEAN = add the mean
    const int32_t *owner;       // [nr_max + nc_max][cstride]: the term of every slot of every row (mtg_launch_prepare)
};
// the evaluation stage for one slab, after mtg_launch_predict_at_factor; 0 = rank outside 0 .. MTG_MAX_J
int mtg_launch_predict_terms_eval(const MtgPredictTermsArgs &, hipStream_t);

// The joint prior draw of the conditional draw (mtg_gp_cond_draw.hip) on the light curve's epochs merged with the
// unique new times tu, and the last step of Matheron's rule.  The sweep leaves y - y~ in `data` for mtg_launch_predict_at
// and the latent f* in `fs`; the scatter adds the two at every entry of the caller's ts.
struct MtgGpCondDrawArgs : MtgRowArgs {
    int64_t Mu;             // unique new times
    const double *tu;       // [Mu] ascending
    const int64_t *first;   // [Mu] index in the caller's ts of the first entry with this time (the caller's normals only)
    int64_t M;              // entries of the caller's ts
    const int64_t *inv;     // [M] index into tu of each of them
    const double *normals;  // [B][N + M] of this slab, or NULL: Philox on the device
    uint32_t seed_lo, seed_hi;
    int64_t draw0;          // global index of row 0 of the batch (mtg_set_stream_base): random counters only
    double *data;           // [B][N]  y_n - y~_n
    double *fs;             // [B][Mu] f*_u
    const double *mu;       // [B][Mu] of mtg_launch_predict_at with `data`
    double *y;              // [B][M]
};
// one slab: the sweep (0 = rank outside 0 .. MTG_MAX_J), and after mtg_launch_predict_at the scatter
int mtg_launch_gp_cond_draw(const MtgGpCondDrawArgs &, hipStream_t);
void mtg_launch_gp_cond_scatter(const MtgGpCondDrawArgs &, hipStream_t);

// samples per LDS tile of the GP draw (mtg_gp_draw.hip): 64 rows x MTG_DRAW_T samples, row stride MTG_DRAW_T + 1 doubles
#ifndef MTG_DRAW_T
#define MTG_DRAW_T 32
#endif
#define MTG_DRAW_TS (MTG_DRAW_T + 1)
static_assert(MTG_DRAW_T % 16 == 0 && 64 % MTG_DRAW_T == 0, "the tile's conflict-free stride and its transposed form");

// The tile of a 64-lane workgroup that owns rows [r0, r0 + 64) of g [B][N] (mtg_gp_draw.hip, mtg_whiten.hip): samples
// [n0, n0 + nt), nt <= MTG_DRAW_T, between global memory and lane-major rows of `tile` [64][MTG_DRAW_TS], transposed on
// the way -- one load or store instruction covers 64 / MTG_DRAW_T rows x MTG_DRAW_T consecutive samples.  No barrier in
// either: the kernel places its own around them.
__device__ __forceinline__ void mtg_tile_load(double *tile, const double *g, int64_t r0, int64_t B, int64_t N, int64_t n0, int nt)
{
    constexpr int RPI = 64 / MTG_DRAW_T;              // rows per transposed instruction
    const int tr = (int)threadIdx.x / MTG_DRAW_T, tc = (int)threadIdx.x % MTG_DRAW_T;
#pragma unroll 4
    for (int i = 0; i < 64; i += RPI) {
        const int rr = i + tr;
        if (r0 + rr < B && tc < nt) tile[rr * MTG_DRAW_TS + tc] = g[(r0 + rr) * N + n0 + tc];
    }
}

__device__ __forceinline__ void mtg_tile_store(double *g, const double *tile, int64_t r0, int64_t B, int64_t N, int64_t n0, int nt)
{
    constexpr int RPI = 64 / MTG_DRAW_T;
    const int tr = (int)threadIdx.x / MTG_DRAW_T, tc = (int)threadIdx.x % MTG_DRAW_T;
#pragma unroll 4
    for (int i = 0; i < 64; i += RPI) {
        const int rr = i + tr;
        if (r0 + rr < B && tc < nt) g[(r0 + rr) * N + n0 + tc] = tile[rr * MTG_DRAW_TS + tc];
    }
}

struct MtgGpDrawArgs : MtgRowArgs {     // of yv only the sigma^2 half is read
    const double *normals;  // [B][N] standard normals of this slab, or NULL: Philox on the device
    uint32_t seed_lo, seed_hi;
    int64_t draw0;          // global index of row 0 of the batch (mtg_set_stream_base): random counters only
    double *y;              // [B][N] of this slab
};
// one slab of draws; 0 = rank outside 0 .. MTG_MAX_J
int mtg_launch_gp_draw(const MtgGpDrawArgs &, hipStream_t);

// samples per chunk of the autocorrelation's lag sums (mtg_whiten.hip): wave w of four takes the chunks w, w + 4, ...
#ifndef MTG_WHITEN_ACF_CHUNK
#define MTG_WHITEN_ACF_CHUNK 256
#endif

struct MtgWhitenArgs : MtgRowArgs {     // the inverse of the draw (mtg_whiten.hip)
    const double *y;        // [B][N] data of this slab without the y_offset, or NULL: the resident data
    double *q;              // [B][N] of this slab, or NULL: the sums alone
    double *stats;          // [batch][MTG_WHITEN_NSTATS], indexed by the row of the batch
};
// one slab of the sweep; 0 = rank outside 0 .. MTG_MAX_J
int mtg_launch_whiten(const MtgWhitenArgs &, hipStream_t);
// the diagnostics of one slab from its q: KS distances into stats (q sorted into `sorted`, [B][N]), lag sums into acf [B][K]
size_t mtg_whiten_sort_temp_bytes(int64_t rows, int64_t N);
hipError_t mtg_launch_whiten_ks(const MtgWhitenArgs &, double *sorted, void *temp, size_t temp_bytes, hipStream_t);
hipError_t mtg_launch_whiten_acf(const MtgWhitenArgs &, int K, double *acf, hipStream_t);

// highest rank the gradient's tangent sweep is compiled for (mtg_loglike_grad.hip): primal and tangent state of a
// lane live in registers, and beyond this rank they no longer fit without scratch
#ifndef MTG_GRAD_MAX_J
#define MTG_GRAD_MAX_J 6
#endif

struct MtgGradArgs : MtgRowArgs {       // the whole batch in one launch: row0 = 0; lane l = e P + p
    MtgModel model;         // the coefficient tangents are expanded from it (mtg_prepare_tangent.h)
    const double *theta;    // [B][P]
    int P;                  // free parameters (>= 1)
    double *dcoef;          // [nslots][dstride]: d coef[slot] / d theta[p] of row e at column e P + p
    int64_t dstride;
    double *out;            // [B] lnL (written by the lane p = 0 of a row; -inf from the expansion for a rejected row)
    double *grad;           // [B][P]
    int32_t *verdict;       // [B] the expansion's status, copied by the tangent kernel: what the sweep reads (it writes `status`)
};
// coefficient tangents, then the tangent sweep; 0 = rank outside 0 .. MTG_GRAD_MAX_J
int mtg_launch_loglike_grad(const MtgGradArgs &, hipStream_t);
static_assert(std::is_trivially_copyable<MtgPredictArgs>::value && std::is_trivially_copyable<MtgPredictAtArgs>::value &&
              std::is_trivially_copyable<MtgGpDrawArgs>::value && std::is_trivially_copyable<MtgGradArgs>::value &&
              std::is_trivially_copyable<MtgGpCondDrawArgs>::value && std::is_trivially_copyable<MtgPredictTermsArgs>::value &&
              std::is_trivially_copyable<MtgWhitenArgs>::value,
              "passed by value as kernel arguments");

struct MtgLombScargleArgs {
    const double2 *dxt, *yv;
    int64_t N, t_stride, L;   // the resident set: t_stride 0 (shared sampling) or N
    int weighted, normalization;
    int nterms;               // harmonics K: 1 (mtg_lomb_scargle_kernel) or 2 .. MTG_LS_MAX_TERMS (mtg_lomb_scargle_multi_kernel)
    double *stats;            // [L][4]: ybar, YY, sum sigma^-2 (or N), 0
    int64_t F;
    const double *freqs;      // [F] on the device
    double *power;            // [slab][F]: the slab being worked on
    double *peak_power;       // [L] or NULL
    int64_t *peak_index;      // [L] or NULL
};
// the pre-pass over all L light curves; then one slab [l0, l0 + Ls) of powers and, where asked for, its peaks
// (0 = more workgroups than a grid holds)
void mtg_launch_lomb_scargle_stats(const MtgLombScargleArgs &, hipStream_t);
int mtg_launch_lomb_scargle(const MtgLombScargleArgs &, int64_t l0, int64_t Ls, hipStream_t);
// the peaks of the rows of power[Ls][F] into peak_power / peak_index at l0, where asked for (mtg_launch_lomb_scargle ends
// with it; mtg_launch_epoch_fold reduces its own powers by it)
void mtg_launch_lomb_scargle_peaks(const MtgLombScargleArgs &, int64_t l0, int64_t Ls, hipStream_t);
// light curves per lane for a set of L: mtg_ls_tile(nterms, L, shared_sampling, weighted)
#include "mtg_ls_plan.h"
// the powers of one slab with nterms >= 2 (mtg_lomb_scargle_multi.hip; mtg_launch_lomb_scargle dispatches to it and adds
// the peaks; 0 = more workgroups than a grid holds)
int mtg_launch_lomb_scargle_multi_powers(const MtgLombScargleArgs &, int64_t l0, int64_t Ls, hipStream_t);

// One slab of mtg_lomb_scargle_envelope (mtg_lomb_scargle_envelope.hip; the cutting rules: mtg_ls_envelope_plan.h): the
// powers of all L light curves at the Fs frequencies from k0 on, as mtg_launch_lomb_scargle left them
struct MtgLsEnvelopeArgs {
    const double *slab;            // [L][Fs]
    int64_t L, Fs, k0;
    int Q;
    const int64_t *ranks;          // [Q] on the device, each in [0, L)
    double *order_stat;            // [Q][Fs]: the slab's
    int64_t *valid;                // [F] or NULL: the call's, written at k0 + k
    const double *reference;       // [F] or NULL
    int64_t *exceed;               // [F] or NULL (needs reference)
    const double *scale;           // [F]: ratio peaks only
    double *peak_ratio;            // [L]: the running maximum of power / scale over the slabs so far, ascending k0
    int64_t *peak_ratio_index;     // [L]
    void *keys_a, *keys_b;         // [Fs][L] 64-bit keys each, and rocPRIM's temporary storage: L > MTG_LSE_LDS_KEYS only
    void *temp;
    size_t temp_bytes;
};
static_assert(std::is_trivially_copyable<MtgLsEnvelopeArgs>::value, "plain data");
// order statistics, valid and exceed of every column of the slab (in LDS, or by segmented sort: mtg_lse_in_lds)
hipError_t mtg_launch_ls_envelope_columns(const MtgLsEnvelopeArgs &, hipStream_t);
// the slab folded into the running ratio peaks
hipError_t mtg_launch_ls_envelope_ratio_peaks(const MtgLsEnvelopeArgs &, hipStream_t);
// rocPRIM's temporary storage for a slab of Fs columns (0 on the LDS path)
size_t mtg_ls_envelope_temp_bytes(int64_t L, int64_t Fs);

// One slab [l0, l0 + Ls) of mtg_epoch_fold / mtg_phase_fold (mtg_epoch_fold.hip; tile and lanes: mtg_ef_plan.h).  `ls`
// is the resident set, the frequencies and the pre-pass statistics as the Lomb-Scargle launcher takes them, its power and
// peaks the slab's and the call's (NULL with the bins alone).  The bins of the slab, each NULL or [Ls][F][nbins]: wsum
// and wrsum from the sweep itself, count and varsum from a pass of their own over the same bins.
#include "mtg_ef_plan.h"
struct MtgEpochFoldArgs {
    MtgLombScargleArgs ls;
    int nbins;
    double time_0;
    double *wsum, *wrsum, *varsum;
    int64_t *count;
};
// (hipErrorInvalidValue: more workgroups than a grid holds)
hipError_t mtg_launch_epoch_fold(const MtgEpochFoldArgs &, const MtgEfPlan &, int64_t l0, int64_t Ls, hipStream_t);

// One slab [l0, l0 + Ls) of mtg_wwz (mtg_wwz.hip; tile, lanes, slab and grid: mtg_wwz_plan.h).  `ls` is the resident set,
// the frequencies and the pre-pass statistics as the Lomb-Scargle launcher takes them; its power is the slab's values
// [Ls][T][F] (NULL: N_eff alone) and its peaks are the call's, reduced over a light curve's whole map.
#include "mtg_wwz_plan.h"
struct MtgWwzArgs {
    MtgLombScargleArgs ls;
    int64_t T;
    const double *taus;    // [T] on the device
    double kc;             // 4 pi^2 decay
    int statistic;         // MTG_WWZ_*
    double *neff;          // NULL or [Ls][T][F] of the slab
    double *nearest;       // workspace [Ls][T] (shared sampling: [T]): the squared distance of tau to its nearest sample
};
// (hipErrorInvalidValue: more workgroups than a grid holds, or a plan that is not mtg_wwz_plan's)
hipError_t mtg_launch_wwz(const MtgWwzArgs &, const MtgWwzPlan &, int64_t l0, int64_t Ls, hipStream_t);

// One slab [l0, l0 + Ls) of mtg_lag_sums (mtg_lag.hip; tile, workspace and slab: mtg_lag_plan.h).  `ls` is the resident
// set and the pre-pass statistics (unweighted) as the Lomb-Scargle launcher takes them; the frequencies, power and peaks
// are not read.  The outputs are the call's, each NULL or [L][nbins] on the device, written at l0.
#include "mtg_lag_plan.h"
struct MtgLagArgs {
    MtgLombScargleArgs ls;
    int nbins;
    const double *edges;   // [nbins + 1] on the device
    double *ws;            // plan.ws_bytes
    int64_t *count;
    double *lag, *sf, *cf, *cf2, *noise;
};
// (hipErrorInvalidValue: more workgroups than a grid holds, a slab outside the set, or a plan that is not mtg_lag_plan's for
// these sizes and outputs: mtg_lag_launch_blocks)
hipError_t mtg_launch_lag(const MtgLagArgs &, const MtgLagPlan &, int64_t l0, int64_t Ls, hipStream_t);

// One slab [l0, l0 + Ls) of mtg_cross_sums (mtg_cross.hip; instantiation, workspace and slab: mtg_cross_plan.h).  `ls` is
// the resident set and its pre-pass statistics (unweighted); the companion is its times, its values as (y2, anything)
// pairs, [1][M] or [L][M] as plan.per says, and the same pre-pass's statistics of those rows.  The outputs are the
// call's, each NULL or [L][nbins] on the device, written at l0.
#include "mtg_cross_plan.h"
struct MtgCrossArgs {
    MtgLombScargleArgs ls;
    int64_t M;
    const double *t2;        // [M] on the device
    const double2 *yv2;      // [L2][M]
    const double *stats2;    // [L2][4]
    int nbins;
    const double *edges;     // [nbins + 1] on the device
    double *ws;              // plan.ws_bytes
    int64_t *count;
    double *lag, *cf, *cf2, *sa, *sb, *saa, *sbb;
};
// (hipErrorInvalidValue: more workgroups than a grid holds, a slab outside the set, or a plan that is not mtg_cross_plan's for
// these sizes and outputs: mtg_lag_launch_blocks)
hipError_t mtg_launch_cross(const MtgCrossArgs &, const MtgCrossPlan &, int64_t l0, int64_t Ls, hipStream_t);

// One slab [l0, l0 + Ls) of mtg_iccf (mtg_iccf.hip; instantiation, grid and slab: mtg_iccf_plan.h).  `ls` and the companion
// as in MtgCrossArgs.  The lags as the caller gave them, and the order the grid's lanes take them in (ascending tau).
// ccf, n_a and n_b are the SLAB's, each NULL or [Ls][K]; peak, peak_index and centroid are the call's, each NULL or [L],
// written at l0 (they need ccf).
#include "mtg_iccf_plan.h"
struct MtgIccfArgs {
    MtgLombScargleArgs ls;
    int64_t M;
    const double *t2;        // [M] on the device
    const double2 *yv2;      // [L2][M]
    const double *stats2;    // [L2][4]
    int64_t K;
    const double *tau;       // [K] on the device
    const int32_t *order;    // [K] on the device: a permutation of 0 .. K - 1
    int mode;                // MTG_ICCF_*
    double threshold;
    double *ccf;
    int64_t *n_a, *n_b;
    double *peak;
    int64_t *peak_index;
    double *centroid;
};
// (hipErrorInvalidValue: more workgroups than a grid holds, a slab outside the set or beyond the plan's, sizes out of
// range, or a plan that is not mtg_iccf_plan's for these sizes and this mode)
hipError_t mtg_launch_iccf(const MtgIccfArgs &, const MtgIccfPlan &, int64_t l0, int64_t Ls, hipStream_t);

typedef void (*mtg_solve_launcher)(const MtgSolveArgs &, int64_t nlanes, hipStream_t);
// Table lookup of the compiled <NR, NC> instantiations (mtg_kernels.hip).
mtg_solve_launcher mtg_find_solver(int nr, int nc, int last_b0 = 0);
// The same sweep with a profile mean subtracted inside the step (mtg_kernels_mean.hip): one table per mean kind
mtg_solve_launcher mtg_find_mean_solver(int mean_kind, int nr, int nc, int last_b0 = 0);
// Time-parallel (one wave per evaluation) instantiations, J <= 6 (mtg_timeparallel.hip); the
// launcher's second argument is the number of evaluations.
mtg_solve_launcher mtg_find_tp_solver(int nr, int nc);
// Same with 256 chunks (four waves) per evaluation, J <= 5: for batches of at most a few hundred.
mtg_solve_launcher mtg_find_tp_wide_solver(int nr, int nc);
// All nsig = (SHO terms + 1) structures (nr0 + 2k, nc0 - k) of a model in one launch: the launcher
// takes list = base of the per-structure lists, count_ptr = base of the counts; lanes 64 or 256.
mtg_solve_launcher mtg_find_tp_fused_solver(int nr0, int nc0, int nsig, int lanes);
// owner: NULL, or [nr_max + nc_max][cstride] int32 receiving the term of every slot of every accepted row (mtg_prepare.h)
void mtg_launch_prepare(const MtgPrepArgs &, hipStream_t, int32_t *owner = nullptr);
// mtg_sort.hip: evaluation indices sorted (stable) by key = structure * L + light curve, rejected rows last
int mtg_sort_key_bits(int64_t L, int nsig);
size_t mtg_sort_temp_bytes(int64_t B, int bits);
hipError_t mtg_launch_sort_by_lightcurve(int64_t B, const int32_t *status, const int32_t *sig, const int32_t *lc, int64_t L,
                                         int nsig, uint32_t *keys_in, uint32_t *keys_out, int *order, void *temp,
                                         size_t temp_bytes, hipStream_t stream);
// every structure of a sorted batch in one launch (mtg_kernels_multi.hip): a.list = the sorted order, a.seg_counts =
// the rows per structure; nullptr when the combination is not compiled
mtg_solve_launcher mtg_find_multi_solver(int nr0, int nc0, int nsig, int last_b0);
// the serial sweep as a producer / consumer pipeline of two waves per 64 rows (mtg_kernels_pipe.hip), for batches that
// leave the one-lane-per-evaluation launch a single wave on half of the SIMDs; nsig = 1: list / count_ptr as for
// mtg_find_solver's kernels, nsig > 1: the sorted order and seg_counts as for mtg_find_multi_solver's
mtg_solve_launcher mtg_find_pipe_solver(int nr0, int nc0, int nsig, int last_b0);
// two models' pipelined sweeps in ONE launch (mtg_kernels_pipe_pair.hip): a workgroup of eight waves runs a quartet of
// each, two waves per SIMD sharing one table set; shapes as for mtg_find_pipe_solver; NULL = this pair is not compiled
struct MtgPipeShapeId { int nr0, nc0, nsig, last_b0; };
typedef void (*mtg_pipe_pair_launcher)(const MtgSolveArgs &a, int64_t nlanes_a, const MtgSolveArgs &b, int64_t nlanes_b, hipStream_t);
mtg_pipe_pair_launcher mtg_find_pipe_pair_solver(const MtgPipeShapeId &a, const MtgPipeShapeId &b);
// does mtg_find_solver(nr, nc, last_b0) return the b = 0 specialisation?
int mtg_solver_uses_b0(int nr, int nc, int last_b0);
void mtg_launch_lc_setup(int64_t N, int64_t L, int64_t t_rows, const double *t, const double *y,
                         const double *yerr, const double *y_offset, double2 *dxt, double2 *yv,
                         double *dxmax, hipStream_t);
// device-resident ensemble sampler (mtg_sampler.hip)
struct MtgEnsembleArgs {
    int E, W, P;
    uint32_t e_base;      // index of ensemble 0 in the caller's global numbering: random counters only (mtg_set_stream_base)
    uint32_t seed_lo, seed_hi;
    double a;             // stretch scale
    int32_t *perm;        // [E][W] red/blue split of the current iteration
    const int32_t *perm_next = nullptr;   // [E][W] split of the iteration about to be proposed, made beforehand (or NULL: made in place)
    double *coords;       // [E][W][P]
    double *lnp;          // [E][W]
    double *factor;       // [E][W/2] (P - 1) ln z of the current proposals ([2][E][W/2] for a speculative iteration)
    int32_t *naccept;     // [E][W]
    double *best_lnp;     // [E]
    double *best_coords;  // [E][P]
    int32_t *n_notpd;
};
// One launch between two solves: accept of half-step (iteration, half) -- proposals in pa.theta, results in
// new_lnp / status -- then the proposals of (next_iteration, next_half) expanded through pa (either part optional).
// The defaults are the priming launch of a run: nothing to accept, the first proposals.
struct MtgSamplerLaunch {
    int do_accept = 0, half = 0;
    uint32_t iteration = 0;
    const double *new_lnp = nullptr;
    const int32_t *status = nullptr;
    int *clear_counts = nullptr;                           // counters of the bank the solve has just used
    double *chain_row = nullptr, *lnp_chain_row = nullptr;  // [E][W][P], [E][W] of the iteration this accept completes, or NULL
    int do_propose = 1, next_half = 0;
    uint32_t next_iteration = 0;
};
void mtg_launch_sampler_step(const MtgEnsembleArgs &g, const MtgSamplerLaunch &l, const MtgPrepArgs &pa, hipStream_t);
// A whole iteration speculatively (mtg_sampler.hip): accept of both half-steps of `iteration` from the 3 E W/2 rows
// in new_lnp / status, then the 3 E W/2 proposals of next_iteration (g.factor holds 2 E W/2 entries; half and next_half
// have no meaning here).
void mtg_launch_sampler_spec(const MtgEnsembleArgs &g, const MtgSamplerLaunch &l, const MtgPrepArgs &pa, hipStream_t);
// the splits of `steps` iterations from iteration0 on, perm_all[steps][E][W] (mtg_sampler.hip)
void mtg_launch_split_all(const MtgEnsembleArgs &g, uint32_t iteration0, int steps, int32_t *perm_all, hipStream_t);
void mtg_launch_initial_best(int E, int W, int P, const double *coords, const double *lnp, double *best_lnp,
                             double *best_coords, hipStream_t);
// TK95 light-curve simulation (mtg_simulate.hip)
// The launchers take their arguments by name: first what a whole call shares (filled once), then what changes from one
// chunk of S series, global indices s0 .. s0 + S, to the next.
struct MtgTk95Spectrum {   // random spectra X[S][nfft / 2 + 1] of the model's (or a tabulated) power spectrum
    int64_t sbase = 0, nfft = 0;
    double dt = 1.0;
    const double *coef = nullptr;   // the expanded model (no table): [slot][cstride], structure of series i in sig[i]
    int64_t cstride = 0;
    MtgCoefLayout lay = {0, 0};
    int nr0 = 0, nc0 = 0;
    const int32_t *sig = nullptr;
    const double *psd_table = nullptr;   // [psd_rows][nfft / 2 + 1], psd_rows = 1 or one per series
    int64_t psd_rows = 0;
    uint64_t seed = 0;
    const double *given = nullptr;       // standard normals handed in instead of drawn
    int64_t S = 0, s0 = 0;
    double2 *X = nullptr;
};
void mtg_launch_tk95_spectrum(const MtgTk95Spectrum &, hipStream_t);
struct MtgTk95Segment {    // the cut segment of every series as rates: out[s0 - out_first + i][seg_len]
    int64_t sbase = 0, nfft = 0, seg_len = 0;
    double dt = 1.0, scale = 1.0, mean_rate = 0.0;
    uint64_t seed = 0;
    const int64_t *given_start = nullptr;   // starts handed in instead of drawn
    int64_t S = 0, s0 = 0;
    const double *series = nullptr;         // [S][nfft]
    double *out = nullptr;
    int64_t out_first = 0;
};
void mtg_launch_tk95_segment(const MtgTk95Segment &, hipStream_t);
// KraftNoise (noise_models.py:81-150) for noise_kind 3: background counts and rate errors per epoch, and the posterior
// median / half-width of the 68 % interval of the source counts for total counts 0 .. K - 1 (< threshold), [N][K]
struct MtgKraftTables {
    const double *bkg_counts = nullptr, *bkg_rate_err = nullptr, *median = nullptr, *half = nullptr;
    int K = 0;
    double threshold = 0.0;
};
// the E13 flux-PDF adjustment of the cut segments (mtg_e13.hip)
size_t mtg_e13_sort_temp_bytes(int64_t S, int64_t n);
void mtg_launch_e13_std(int64_t S, int64_t n, const double *seg, double *stdv, hipStream_t);
void mtg_launch_e13_draw(int64_t S, int64_t s0, int64_t sbase, int64_t n, int kind, double mean, const double *stdv, uint64_t seed,
                         double *x, hipStream_t);
void mtg_launch_e13_iota(int64_t S, int64_t n, int32_t *idx, int32_t *done, hipStream_t);
void mtg_launch_e13_abs(int64_t total, const double2 *spec, double *amp, hipStream_t);
void mtg_launch_e13_phase(int64_t total, const double *amp, double2 *spec, hipStream_t);
hipError_t mtg_launch_e13_sort_values(int64_t S, int64_t n, const double *x, double *keys_out, const int32_t *idx, int32_t *order_tmp,
                                      uint32_t *segment, uint32_t *segment_out, int32_t *order, double *values, void *temp,
                                      size_t temp_bytes, hipStream_t);
hipError_t mtg_launch_e13_rank(int64_t S, int64_t n, const double *keys, double *keys_out, const int32_t *idx, int32_t *order_tmp,
                               uint32_t *segment, uint32_t *segment_out, int32_t *order, void *temp, size_t temp_bytes, hipStream_t);
void mtg_launch_e13_step(int64_t S, int64_t n, const int32_t *order, const double *values, double *x, double *fresh, int32_t *done,
                         int32_t *notconv, int32_t *running, hipStream_t);
struct MtgTk95Observe {    // window averages of the cut segments at the N epochs, with noise: rates / dy [.][N] by global index
    int64_t sbase = 0, N = 0, nfft = 0, seg_len = 0;
    double dt = 1.0, scale = 1.0, mean_rate = 0.0;   // (all neutral: the plain window average of the series)
    const int32_t *win_lo = nullptr, *win_hi = nullptr;
    int noise_kind = 0;
    double sigma_noise = 0.0;
    const double *exposures = nullptr;
    MtgKraftTables kraft;
    int64_t fixed_start = -1;               // >= 0: every segment starts here; -1: drawn from the seed
    uint64_t seed = 0;
    const int64_t *given_start = nullptr;   // starts handed in: they go before either
    double *clean = nullptr, *rates = nullptr, *dy = nullptr;
    int64_t S = 0, s0 = 0;
    const double *series = nullptr;         // [S][nfft]
};
void mtg_launch_tk95_observe(const MtgTk95Observe &, hipStream_t);
void mtg_launch_tk95_resident(int64_t L, int64_t N, const double *rates, const double *dy, double2 *yv, double *means,
                              hipStream_t);
// inverse real transform of a length with large prime factors on power-of-two transforms (chirp-z; mtg_simulate.hip)
void mtg_launch_czt_tables(int64_t n, int64_t m, double2 *chirp, double2 *b, hipStream_t);
void mtg_launch_czt_pack(int64_t S, int per, int64_t n, int64_t m, const double2 *X, const double2 *chirp, double2 *a, hipStream_t);
void mtg_launch_czt_mul(int64_t pairs, int64_t m, const double2 *bhat, double2 *a, hipStream_t);
void mtg_launch_czt_unpack(int64_t S, int per, int64_t n, int64_t m, const double2 *c, const double2 *chirp, double *series, hipStream_t);
void mtg_launch_apply_inverse(const double *work, int64_t N, int J, int64_t M, double *x, hipStream_t);
void mtg_launch_math_probe(int64_t n, const double *x, double *e, double *s, double *c, double *rcp,
                           hipStream_t);

// walker-averaged autocorrelation function of a chain (mtg_simulate.hip)
void mtg_launch_acf_center(int64_t n_t, int64_t n2, int64_t S, const double *chain, double *x, double *sumsq, double *scratch,
                           hipStream_t s);
void mtg_launch_acf_power(int64_t nk, int64_t E, int W, int P, const double2 *f, const double *sumsq, double2 *g, hipStream_t s);
void mtg_launch_acf_transpose(int64_t rows, int64_t cols, const double *in, double *out, hipStream_t s);
void mtg_launch_acf_out(int64_t n_t, int64_t n2, int64_t EP, double scale, const double *r, double *rho, hipStream_t s);
