/*
 * include/mtg.h -- C-ABI of libmtg_hip.so, the MI355X (gfx950) engine behind
 * mind_the_gaps' GP log-likelihood hot path.
 *
 * Every entry point replaces a piece of the reference's Python -> celerite
 * interface (paths relative to /root/reference); the reference has no FFI of
 * its own (celerite is a pybind11 dependency), so these are the functions a
 * ctypes binding inside mind_the_gaps/gpmodelling.py would bind
 * (INTEGRATION.md shows that stub).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative MTG_E_* code and never throws; the caller owns every
 * pointer it passes, the library borrows it for the duration of the call;
 * device buffers created by the library belong to the context.  One in-flight
 * call per context; any number of contexts (one per process per GPU is the
 * intended use).  All arithmetic is IEEE float64.
 */
#ifndef MTG_H
#define MTG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTG_API __attribute__((visibility("default")))

/* ---- error codes -------------------------------------------------------- */
#define MTG_OK 0
#define MTG_E_ARG (-1)       /* bad argument (message in mtg_last_error)        */
#define MTG_E_NODEVICE (-2)  /* no usable gfx950 device / HIP runtime failure   */
#define MTG_E_HIP (-3)       /* a HIP call failed                               */
#define MTG_E_STATE (-4)     /* light curves or model not set yet               */
#define MTG_E_UNSUPPORTED (-5) /* kernel structure outside the compiled table  */

/* ---- per-evaluation status (status[b]) ----------------------------------- */
#define MTG_ST_OK 0        /* lnP finite                                        */
#define MTG_ST_PRIOR 1     /* log_prior = -inf: lnP = -inf, likelihood skipped
                              (gpmodelling.py:149-151)                           */
#define MTG_ST_NOTPD 2     /* non-positive pivot D_n: celerite raises
                              LinAlgError here; lnP is written as -inf           */
#define MTG_ST_NONFINITE 3 /* lnL or ln det not finite: celerite returns -inf   */

/* ---- term kinds: celerite coefficient builders, evaluated on the device --- */
#define MTG_TERM_REAL 0       /* celerite.terms.RealTerm(log_a, log_c)                  */
#define MTG_TERM_COMPLEX3 1   /* celerite.terms.ComplexTerm(log_a, log_c, log_d), b = 0 */
#define MTG_TERM_COMPLEX4 2   /* celerite.terms.ComplexTerm(log_a, log_b, log_c, log_d) */
#define MTG_TERM_SHO 3        /* celerite.terms.SHOTerm(log_S0, log_Q, log_omega0)      */
#define MTG_TERM_MATERN32 4   /* celerite.terms.Matern32Term(log_sigma, log_rho; eps)   */
#define MTG_TERM_JITTER 5     /* celerite.terms.JitterTerm(log_sigma)                   */
#define MTG_TERM_DRW 6        /* mind_the_gaps/models/celerite_models.py:55-68          */
#define MTG_TERM_LORENTZIAN 7 /* mind_the_gaps/models/celerite_models.py:7-34           */
#define MTG_TERM_COSINUS 8    /* mind_the_gaps/models/celerite_models.py:36-52          */
#define MTG_TERM_BPL 9        /* mind_the_gaps/models/celerite_models.py:71-90          */
#define MTG_N_TERM_KINDS 10

#define MTG_MEAN_CONSTANT 0   /* celerite.modeling.ConstantModel(value)                 */
#define MTG_MEAN_LINEAR 1     /* mind_the_gaps/models/mean_models.py:24-31 (slope, intercept) */
/* The reference's profile means, parameters in the order of their parameter_names, values at the absolute time t:     */
#define MTG_MEAN_SINE 2       /* mean_models.py:12-16 (constant, amplitude, frequency, phase):
                                 constant + amplitude sin(frequency t + phase)                                          */
#define MTG_MEAN_TWOSINE 3    /* mean_models.py:18-22 (constant, amplitude0, phase0, amplitude1, phase1, frequency):
                                 constant + amplitude0 sin(frequency t + phase0) + amplitude1 sin(2 frequency t + phase1) */
#define MTG_MEAN_GAUSSIAN 4   /* mean_models.py:6-10 (mean, sigma, amplitude, constant):
                                 amplitude / (2 pi sigma) exp(-(t - mean)^2 / (2 sigma^2)) + constant -- the
                                 normalisation is 2 pi sigma, NOT sqrt(2 pi) sigma: the reference's own, kept as is     */
#define MTG_N_MEAN_KINDS 5

#define MTG_MAX_TERMS 12
#define MTG_MAX_PARAMS 40     /* full parameter vector: kernel + mean parameters        */
#define MTG_MAX_J 10          /* celerite rank J = n_real + 2 n_complex                 */
#define MTG_MAX_WALKERS 4096  /* walkers per ensemble of the device sampler             */

typedef struct mtg_ctx mtg_ctx;

/* Library / device discovery.  mtg_device_count() < 0 means no HIP runtime. */
MTG_API int mtg_device_count(void);
MTG_API const char *mtg_version(void);
MTG_API int mtg_term_nparams(int kind);
/* Parameters of a mean kind (1, 2, 4, 6, 4 for MTG_MEAN_CONSTANT .. MTG_MEAN_GAUSSIAN); -1 for an unknown kind. */
MTG_API int mtg_mean_nparams(int kind);

/*
 * Context = one GPU + its light curves + its model + workspaces.
 * Replaces the per-process state the reference keeps in `self.gp`
 * (gpmodelling.py:51-55) and copies into every multiprocessing.Pool worker
 * (gpmodelling.py:245).  Returns NULL when `device` is not a usable GPU.
 */
MTG_API mtg_ctx *mtg_create(int device);
/*
 * A context whose kernels run on one of `parts` (1 to 8) equal, disjoint slices of the device's compute units (CU i is
 * in slice i mod parts; the context's stream carries the CU mask).  Two contexts on the two halves of a GPU run their
 * launches side by side whatever order they arrive in: the null and the alternative model's refits of the Protassov
 * loop (docs/notebooks/tutorial_ppp.ipynb:334-340, one after the other in the reference), each a half-step of
 * ~32 000 rows at 8 GPUs -- one wave per SIMD on its half -- take max(t_null, t_alt) together instead of
 * t_null + t_alt (ppp.protassov_test(concurrent_refits=True)).  Calls on a caller's stream
 * (mtg_loglike_batch_device with a stream of the caller's) run wherever that stream runs.
 */
MTG_API mtg_ctx *mtg_create_on_slice(int device, int part, int parts);
MTG_API void mtg_destroy(mtg_ctx *ctx);
/* Message for the last non-zero return on this context (ctx may be NULL for
 * mtg_create failures). */
MTG_API const char *mtg_last_error(const mtg_ctx *ctx);
/*
 * Testing aid.  The sweep reads samples through buffer descriptors with 32-bit byte
 * offsets; for resident sets beyond 4 GiB every wave places its descriptor at the
 * first light curve its 64 evaluations need and reaches the others within a window
 * of `bytes` (default and maximum 2^32 - 1).  Evaluations further away (never, when
 * a batch is grouped by light curve) are collected and swept one per wave by a
 * second launch.  A small window lets a test exercise that logic on a small set.
 */
MTG_API int mtg_set_window_bytes(mtg_ctx *ctx, uint64_t bytes);

/*
 * celerite.GP.compute(t, yerr) for L light curves at once; the reference calls
 * it with yerr = dy + 1e-12 (gpmodelling.py:54) and the host layer above this
 * ABI does the same.  t: [N] when t_per_lc == 0 (shared sampling, the PPP case
 * of gpmodelling.py:538) or [L][N]; y, yerr: [L][N], host pointers.  The
 * library checks that every t row is sorted (celerite raises ValueError
 * otherwise -> MTG_E_ARG), forms sigma^2 = yerr^2 (celerite squares yerr) and
 * dx_n = t_n - t_{n-1} on the device and keeps everything resident until the
 * next call / mtg_destroy.
 * y_offset: [L] or NULL.  The reference freezes the mean of every light curve at
 * ITS OWN average, ConstantModel(lightcurve.mean) with fit_mean=False
 * (gpmodelling.py:83-87): pass those L values here (they are subtracted from y
 * once, at upload) and give the model a frozen mean of 0.  The set may be as
 * large as the HBM allows (L * N * 32 bytes resident; the upload is staged in
 * blocks); one light curve must stay below 2^28 samples.
 */
MTG_API int mtg_set_lightcurves(mtg_ctx *ctx, int64_t N, int64_t L, const double *t, int t_per_lc,
                                const double *y, const double *yerr, const double *y_offset);
/* Same with DEVICE pointers (light curves born on the GPU); no sortedness
 * check, the data are copied device-to-device on the context's stream. */
MTG_API int mtg_set_lightcurves_device(mtg_ctx *ctx, int64_t N, int64_t L, const double *d_t,
                                       int t_per_lc, const double *d_y, const double *d_yerr,
                                       const double *d_y_offset);

/*
 * The model: what `celerite.GP(kernel, mean=..., fit_mean=...)`
 * (gpmodelling.py:51) holds.  The FULL parameter vector is the kernel
 * parameters of every term in `+` order followed by the mean parameters
 * (mtg_mean_nparams(mean_kind) of them: 1 for MTG_MEAN_CONSTANT, 2 for
 * MTG_MEAN_LINEAR, 4 / 6 / 4 for MTG_MEAN_SINE / _TWOSINE / _GAUSSIAN), PF
 * entries in all.  free_index and bounds cover the mean parameters like any
 * other, so part of a mean can be frozen.
 * The profile means (MTG_MEAN_SINE, _TWOSINE, _GAUSSIAN) are evaluated by the
 * one-lane sweep alone (mtg_kernels_mean.hip): mtg_loglike_batch[_device],
 * mtg_loglike_coeffs, mtg_ensemble_* (sharded or not) and mtg_apply_inverse
 * (which does not read the mean) work with them; mtg_predict, mtg_predict_at, mtg_predict_terms,
 * mtg_gp_draw, mtg_gp_cond_draw and mtg_loglike_grad return MTG_E_UNSUPPORTED (the host layer
 * binds y - mean(t) with a zero mean for those, one theta at a time), and a
 * context paired with mtg_pair_contexts launches alone.  A row whose mean is
 * not finite at some sample (sigma = 0) gets MTG_ST_NONFINITE.
 *   kinds[nterms]      MTG_TERM_* tags
 *   term_extra[nterms] per-term constant (Matern32Term eps), may be NULL
 *   full_values[PF]    current value of every parameter (used for frozen ones)
 *   free_index[P]      position in the full vector of each entry of theta,
 *                      i.e. celerite's unfrozen-parameter order
 *                      (get_parameter_vector, gpmodelling.py:55)
 *   bounds[PF][2]      (lo, hi) of every parameter, +-inf for None
 *                      (get_parameter_bounds(include_frozen=True))
 */
MTG_API int mtg_set_model(mtg_ctx *ctx, int nterms, const int32_t *kinds, const double *term_extra,
                          int mean_kind, int PF, const double *full_values, int P,
                          const int32_t *free_index, const double *bounds);

/*
 * GPModelling._log_probability (gpmodelling.py:127-152; add_prior = 1) and
 * -GPModelling._neg_log_like (gpmodelling.py:155-169; add_prior = 0) for B
 * parameter vectors in one launch.  theta: [B][P] host; lc_index: [B] light
 * curve of each row (NULL = all 0); out: [B] lnP; status: [B] MTG_ST_*.
 * Replaces emcee's `pool.map(self._log_probability, coords)` (gpmodelling.py:247-248)
 * and scipy's serial finite-difference calls (gpmodelling.py:192).
 */
MTG_API int mtg_loglike_batch(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index,
                              int add_prior, double *out, int32_t *status);
/*
 * Same with DEVICE pointers, enqueued on `stream` (a hipStream_t passed as void*) without
 * synchronising: inputs stay resident in HBM, results are valid once the stream reaches this point.
 * NULL is what it is everywhere in HIP: the (legacy) default stream -- PyTorch's
 * torch.cuda.current_stream().cuda_stream is 0 for its default stream, and work the caller has
 * queued there (the producer of d_theta, the consumer of d_out) is ordered with the launch.
 * MTG_STREAM_CONTEXT selects the context's own non-blocking stream, which is NOT ordered against the
 * default stream as far as the CALLER's work goes.  The library's own calls are always ordered one after
 * the other whatever streams they run on (they share the context's workspaces): a call that follows one on
 * a different stream waits for it through an event, and mtg_synchronize waits for the last call on a
 * caller's stream as well as for the context's stream.
 *
 * Order of evaluation: the throughput kernel gives every evaluation a lane and each lane reads its own
 * light curve, so it wants the lanes of a wave on one or two light curves.  Large batches are therefore
 * swept in the order of a stable sort by (structure, light curve) of the library's own making, whatever
 * order the caller's rows have (results are per row and do not depend on it); mtg_set_sort: 0 = keep the
 * caller's order, 1 = always sort, 2 (default) = sort unless the host-pointer entry point sees that the
 * rows are grouped by light curve already.  A model whose rows fall into more than one structure (an SHO
 * term on either side of Q = 1/2) is always swept in sorted order under 1 and 2: the per-structure lists
 * are filled with atomics, and only the sort makes the assignment of rows to waves -- on which the last
 * bits of a row can depend, see MTG_TRIG_FAST_MAX -- the same in every run, as a seeded chain needs it.
 */
#define MTG_STREAM_CONTEXT ((void *)(intptr_t)-1)
MTG_API int mtg_loglike_batch_device(mtg_ctx *ctx, int64_t B, const double *d_theta,
                                     const int32_t *d_lc_index, int add_prior, double *d_out,
                                     int32_t *d_status, void *stream);

/*
 * celerite solver entry `compute(jitter, a_real, c_real, a_comp, b_comp, c_comp,
 * d_comp, ...)` + log_likelihood for user-defined Python terms whose
 * coefficients are evaluated on the host (celerite_models.py:9,17 override
 * points).  All evaluations share one structure (jr real, jc complex terms).
 * a_real..d_comp: [B][jr] / [B][jc] host, jitter: [B] (NULL = 0),
 * mean_params: [B][mtg_mean_nparams(mean_kind)] (NULL = 0; a profile mean needs them).
 */
MTG_API int mtg_loglike_coeffs(mtg_ctx *ctx, int64_t B, int jr, int jc, const double *a_real,
                               const double *c_real, const double *a_comp, const double *b_comp,
                               const double *c_comp, const double *d_comp, const double *jitter,
                               int mean_kind, const double *mean_params, const int32_t *lc_index,
                               double *out, int32_t *status);

/*
 * Kernel choice for mtg_loglike_batch[_device] / mtg_ensemble_*: 0 = always one lane per
 * evaluation (throughput kernel), 1 = one wave per evaluation, parallel in time, whenever the
 * structure has that kernel (J <= 6, and the J = 10 structures of five SHO terms), 2 = automatic
 * (default): time-parallel for light curves of at least 256 samples and batches of at most 1024
 * evaluations (J <= 6: 4-10x faster there); J = 10: at least 1024 samples and at most 8192 evaluations
 * (the light curve is cut into as many chunks as fill the GPU: 40-100x faster than the serial sweep for
 * the 32-256 evaluations of an ensemble half-step).  3 = as 1, restricted to the one-wave-per-evaluation kernel
 * (J <= 6): under 1 and 2 the number of rows in a batch picks between kernels whose sums differ in the last bits;
 * under 0 (one-lane sweep and its pipelined form, bit-identical to each other) and under 3 a row's result does not
 * depend on what else is in the batch -- what a job that splits its rows over several GPUs needs to reproduce the
 * one-GPU result exactly (ppp.protassov_test(reproducible=True)).
 * A model with a profile mean (MTG_MEAN_SINE, _TWOSINE, _GAUSSIAN) runs on the one-lane sweep under every mode: a row's
 * result does not depend on the batch it travels in, whatever this is set to.
 */
MTG_API int mtg_set_time_parallel(mtg_ctx *ctx, int mode);
/*
 * Index of this context's first resident ensemble (mtg_ensemble_*) and first simulated series
 * (mtg_simulate_tk95) in the caller's global numbering, default 0.  The counter-based random streams are keyed by
 * (seed, ..., first_index + local index): a job that splits E ensembles or S series over several contexts (GPUs)
 * with the same seed draws, for every one of them, exactly the numbers ONE context holding them all would draw --
 * the result of the reference's loop over simulated light curves (docs/notebooks/tutorial_ppp.ipynb:326-343,
 * gpmodelling.py:505-513) no longer depends on how many GPUs share it.  Read at mtg_ensemble_init / at every
 * mtg_simulate_tk95; enters random counters only, never an address.
 */
MTG_API int mtg_set_stream_base(mtg_ctx *ctx, int64_t first_index);
/*
 * mtg_simulate_tk95 transforms a grid length with large prime factors (the reference's grid arithmetic, simulator.py:259-262,
 * gives BASELINE configs[3] 1 087 853 = 13^2 x 41 x 157 points) on power-of-two transforms by hand (chirp-z), two real
 * series per complex transform: hipFFT's own plan for such a length takes 0.9 s to build.  on = 0: one series per
 * transform, so that a series' values do not depend on which other series the call holds -- what a set simulated in
 * blocks over several GPUs needs to be the set of one call, bit for bit (with mtg_set_stream_base); default 1.
 */
MTG_API int mtg_set_simulate_pairs(mtg_ctx *ctx, int on);
/*
 * The flux PDF of the light curves mtg_simulate_tk95 makes (Simulator(..., pdf=...), simulator.py:149-150): kind 0 (default)
 * Gaussian = the TK95 series as it is; 1 lognormal, 2 uniform = every cut segment goes through the amplitude / rank
 * adjustment of Emmanoulopoulos et al. 2013 as the reference runs it (simulator.py:65-140 E13Simulator; the distributions
 * of stats.py:116-146 with the simulator's mean and the segment's standard deviation), at most max_iter + 1 iterations
 * (the reference's `max_iter`), ON THE DEVICE (csrc/mtg_e13.hip: batched hipFFT transforms, one segmented radix sort per
 * iteration) before the segment is averaged into the epochs; everything after it -- noise, make_resident -- as for the
 * Gaussian case, so a posterior-predictive run with a non-Gaussian PDF never leaves the GPU.  The white series is drawn
 * from the context's Philox stream (keyed by seed and global series index), or taken from the caller for the NEXT call:
 * mtg_set_simulate_pdf_draws(ctx, S, n, draws[S][n]) with n = seg_len (tests hold the device against the host with it).
 * mtg_simulate_pdf_report: segments of the last call that used all their iterations without converging (the reference
 * warns), and the largest iteration count.
 */
MTG_API int mtg_set_simulate_pdf(mtg_ctx *ctx, int kind, int max_iter);
/*
 * KraftNoise (noise_models.py:81-150) for mtg_simulate_tk95(noise_kind = 3), on the device: total counts ~ Poisson(rate x
 * exposure + bkg_counts[n]); net rate = (total - bkg) / exposure, dy = sqrt((sqrt(total) / exposure)^2 + bkg_rate_err[n]^2);
 * epochs with total < threshold (the reference's kraft_counts, 15) take the median of the Kraft, Burrows & Nousek (1991)
 * posterior of the source counts and half the width of its 68 % interval instead -- functions of (total, background)
 * alone, tabulated by the caller for total = 0 .. K - 1 and every epoch: median[N][K], half[N][K] (counts; K >= threshold).
 * N must be the number of epochs of the resident sampling; N = 0 forgets the tables.
 */
MTG_API int mtg_set_simulate_kraft(mtg_ctx *ctx, int64_t N, int K, double threshold, const double *bkg_counts, const double *bkg_rate_err,
                                   const double *median, const double *half);
MTG_API int mtg_set_simulate_pdf_draws(mtg_ctx *ctx, int64_t S, int64_t n, const double *draws);
MTG_API int mtg_simulate_pdf_report(const mtg_ctx *ctx, int64_t *not_converged, int *iterations);
/* Which transform mtg_simulate_tk95 takes: 0 (default) = by grid length (hipFFT's plan for lengths of radices 2-13, the
 * hand-written chirp-z otherwise), 1 = always hipFFT's plan, 2 = always chirp-z (tests compare the two). */
MTG_API int mtg_set_simulate_transform(mtg_ctx *ctx, int mode);
/*
 * The reference's simulator draws from numpy's GLOBAL generator -- get_fft (simulator.py:468-501): real, im =
 * np.random.normal(0, size=(2, N // 2 + 1)); cut_random_segment (simulator.py:536-539): np.random.uniform -- so a user who
 * calls np.random.seed() gets the same light curve every time.  For that user the host draws those numbers in the
 * reference's order and hands them to the NEXT mtg_simulate_tk95 of this context in place of its own Philox streams:
 * normals [S][2][nk] (per series the row of real parts, then the row of imaginary parts, nk = nfft / 2 + 1; entry 0 of
 * either is unused as in the reference) and starts [S], the index of the first fine-grid sample of each series' cut.
 * The spectrum scaling, the inverse transform, the cut, the window averages stay on the device.  Consumed by one call
 * (which must have the same S and nfft; every start + seg_len <= nfft); S = 0 clears.  `Simulator(..., stream="numpy")`.
 */
MTG_API int mtg_set_simulate_draws(mtg_ctx *ctx, int64_t S, int64_t nk, const double *normals, const int64_t *starts);
MTG_API int mtg_set_sort(mtg_ctx *ctx, int mode);
/*
 * The serial sweep as a two-wave pipeline (csrc/mtg_kernels_pipe.hip): 0 = never, 1 = whenever the model has the
 * kernel (ranks 3-6 with a complex term; light curves of at least 64 samples; measurements and tests), 2 (default) =
 * for batches beyond the time-parallel kernels' range that still fit one workgroup of 128 rows per compute unit
 * (32 768 rows on an MI355X), where the one-lane-per-evaluation launch would leave a lone wave on half of the SIMDs:
 * e.g. one GPU's share of the Protassov refits at 8 GPUs -- 250 light curves x 128 walkers per half-step of the
 * reference's loop (docs/notebooks/tutorial_ppp.ipynb:326-343, gpmodelling.py:247-248).  A row's result is the
 * same to the last bit as from the one-lane kernel.
 */
MTG_API int mtg_set_pipeline(mtg_ctx *ctx, int mode);
/*
 * Two contexts on one device whose pipelined half-steps go out in ONE launch (csrc/mtg_kernels_pipe_pair.hip): the null
 * and the alternative kernel of the posterior-predictive test, which the reference fits to every simulated light curve
 * one after the other (docs/notebooks/tutorial_ppp.ipynb:326-343) and which here advance side by side, each context
 * driven by a host thread of its own.  A pipelined sweep takes a whole compute unit (its tables and rings fill the LDS),
 * so two contexts' launches alternate on the compute units and leave every SIMD one wave that issues ~60 % of the time;
 * paired, a workgroup of eight waves runs 128 rows of each model on one table set, two waves per SIMD.  Each call that
 * would dispatch mtg_pipe_kernel meets its partner's (on the host, bounded wait: mtg_set_pair_patience, default 250 ms);
 * a partner that does not come in time means "alone this time" (the next wait is half as long); four misses in a row,
 * another sampling or a pair of model shapes without a compiled kernel break the pair for good and both go on alone.
 * Results are those of the unpaired kernels to the last bit.  mtg_pair_stats: launches that were shared / made alone
 * since pairing, and whether the pair is broken.  mtg_destroy unpairs; unpairing (or destroying) one context while the
 * partner's thread is inside a call is safe: the rendezvous is reference-counted and the partner launches alone.
 */
MTG_API int mtg_pair_contexts(mtg_ctx *a, mtg_ctx *b);
MTG_API int mtg_unpair_contexts(mtg_ctx *ctx);
/* Longest host-side wait (ms >= 1) of a paired context for its partner's half-step; the context must be paired. */
MTG_API int mtg_set_pair_patience(mtg_ctx *ctx, int milliseconds);
MTG_API int mtg_pair_stats(const mtg_ctx *ctx, int64_t *paired_launches, int64_t *solo_launches, int *broken);
/*
 * Speculative iterations of mtg_ensemble_run (default 1 = where they pay, 0 = never).  The time-parallel solve of a
 * small batch takes as long for three times the rows -- most of the GPU is idle -- and the second half-step of a
 * stretch-move iteration depends on the first only through each partner's coordinates: where it is, or where its own
 * proposal would put it.  Both candidates are then evaluated beside the first half-step's proposals, one solve and one
 * sampler launch per iteration instead of two and two (1.9 x the iterations per second for BASELINE configs[0] and
 * [1]).  Taken when all 3 E W/2 rows get a workgroup of their own in one occupancy round (light curves of >= 4096
 * samples: <= 512 rows up to rank 5, <= 256 at rank 6; <= 1024 rows below), J <= 6, not walker-sharded.  The random numbers, hence the chain, are those of
 * the sequential form -- to the last bit where both forms run the same kernel (the batch size picks it: e.g. rank 5,
 * 256 walkers: four waves per evaluation for the 128 rows of a half-step, two for the 384 of a speculative iteration).
 * Mode 2 is mode 1 with every iteration's split ranked inside its sampler launch instead of all of a run's splits in
 * one launch up front (what mode 1 itself does once steps * E * W * 4 bytes pass 64 MiB): same chain, bit for bit.
 */
MTG_API int mtg_set_speculation(mtg_ctx *ctx, int mode);
/* Name of the kernel the last batch was dispatched to, e.g. "mtg_solve_kernel<1,2,1>" (first structure of the
 * model when several were launched); "" before the first call.  For measurements (bench.py roofline.kernel). */
MTG_API const char *mtg_last_solver(const mtg_ctx *ctx);
/*
 * J = 10 time-parallel path: enabled != 0 (default) takes the likelihood from the chunk-composition pass
 * and the scan alone and sends only evaluations whose terms cancel badly (or meet a non-positive pivot)
 * through the filter pass; 0 runs the filter pass for every evaluation.  Same results to ~1e-13; a
 * switch for tests and measurements.
 */
MTG_API int mtg_set_tp_direct(mtg_ctx *ctx, int enabled);
/* Block until everything enqueued on the context's stream has finished, and the last
 * mtg_loglike_batch_device call made on a caller's stream. */
MTG_API int mtg_synchronize(mtg_ctx *ctx);
/* Device time (ms, HIP events on the launch stream) of the last
 * mtg_loglike_batch / mtg_loglike_coeffs call: kernels only, no copies. */
MTG_API double mtg_last_kernel_ms(const mtg_ctx *ctx);
/*
 * Per-call kernel timing for the next `capacity` mtg_loglike_batch[_device]
 * calls: HIP events are recorded on the launch stream before the prepare
 * kernel, between prepare and the solve kernel(s), and after them.
 * mtg_profile_read waits for the recorded calls, writes their durations (ms)
 * and returns how many were recorded (<= capacity), ending the session.
 */
MTG_API int mtg_profile_begin(mtg_ctx *ctx, int capacity);
MTG_API int mtg_profile_read(mtg_ctx *ctx, int capacity, double *prepare_ms, double *solve_ms);
/*
 * Device-resident lock-step ensembles: emcee's stretch move (a = 2, random red/blue
 * split) as `derive_posteriors` drives it (gpmodelling.py:245-248), for E independent
 * ensembles of W walkers with state, random numbers (Philox4x32-10 keyed by `seed`)
 * and accept/reject on the GPU; one iteration = 2 x W/2 evaluations per ensemble, no
 * host synchronisation inside mtg_ensemble_run.
 *   coords          [E][W][P] initial walkers (host), e.g. from spread_walkers; W even,
 *                   2 P <= W <= MTG_MAX_WALKERS
 *   lc_of_ensemble  [E] light curve of every ensemble; NULL = ensemble e -> light
 *                   curve e (E == L), or all -> 0 when one light curve is resident
 *   chain/lnp_chain [steps][E][W][P] / [steps][E][W] host buffers or NULL (emcee's
 *                   get_chain / get_log_prob layout per ensemble)
 * mtg_ensemble_get copies out the current state, the best sample seen per ensemble
 * (max_loglikelihood / max_parameters, gpmodelling.py:431-443), acceptance counts,
 * the iteration count and the number of proposals whose covariance was not positive
 * definite (celerite would have raised LinAlgError; they are rejected here).
 */
MTG_API int mtg_ensemble_init(mtg_ctx *ctx, int64_t E, int W, uint64_t seed, const double *coords,
                              const int32_t *lc_of_ensemble);
MTG_API int mtg_ensemble_run(mtg_ctx *ctx, int steps, double *chain, double *lnp_chain);
/* Resume: after mtg_ensemble_init with the coordinates and the seed of a saved state (mtg_ensemble_get), put the
 * iteration counter -- every random number is a function of (seed, iteration, ...) --, the saved
 * log-probabilities lnp [E][W] and, optionally, the acceptance counts and the running best back;
 * mtg_ensemble_run then continues the chain bit for bit.  lnp = NULL keeps the values mtg_ensemble_init has
 * just computed for the saved coordinates: the same numbers to rounding, but from ONE batch of E W rows where
 * the run evaluated half-ensembles -- another row count may mean another kernel and summation order, and a
 * last-bit difference can flip an accept decision; pass the saved values for a bit-for-bit continuation. */
MTG_API int mtg_ensemble_restore(mtg_ctx *ctx, int64_t iteration, const double *lnp, const int32_t *naccept,
                                 const double *best_lnp, const double *best_coords);
MTG_API int mtg_ensemble_get(mtg_ctx *ctx, double *coords, double *lnp, double *best_lnp, double *best_coords,
                             int32_t *naccept, int64_t *iteration, int32_t *n_notpd);

/*
 * Walker-averaged, normalised autocorrelation function of a chain -- the inner loop of the convergence
 * check of mind_the_gaps/gpmodelling.py:260-272 (emcee.autocorr.integrated_time: function_1d of every
 * walker and dimension by zero-padded FFT, each normalised by its lag-0 value, averaged over the walkers).
 * chain: host [n_t][E][W][P] for E independent ensembles (E = 1: one chain); rho: host out [n_t][E][P].  On
 * the device: E * W * P batched forward transforms, power spectra normalised and averaged over each ensemble's
 * walkers, E * P inverse transforms (hipFFT, the only library call).  A walker that never moved yields NaN in
 * its dimension, as emcee does.
 */
MTG_API int mtg_chain_autocorr(mtg_ctx *ctx, int64_t n_t, int64_t E, int W, int P, const double *chain, double *rho);
/* Pairs of hipFFT plans mtg_chain_autocorr has built on this context so far (it keeps the four most recently used
 * shapes): a call on a cached shape leaves the count alone. */
MTG_API int64_t mtg_chain_autocorr_plans_built(const mtg_ctx *ctx);
/* hipFFT's one-time start-up (~1.4 s: the first plan of a process) paid now, on the context's device; safe to call
 * from a helper thread (HIP's current device is per thread: the call selects ctx's; NULL = the thread's current). */
MTG_API int mtg_fft_warmup(mtg_ctx *ctx);
/* The inverse-transform plan mtg_simulate_tk95 needs for series of nfft points, made now and kept by the context
 * (one plan per length, whatever the number of simulations).  A Bluestein plan -- 1 087 853 points in BASELINE
 * configs[3] -- takes 0.9 s to build: from a helper thread, while the context samples the observed light curve, it
 * costs nothing.  Safe beside any other call on the context; mtg_simulate_tk95 waits for it. */
MTG_API int mtg_simulate_plan(mtg_ctx *ctx, int64_t nfft);

/*
 * Walker sharding of the resident ensembles across the GPUs of a job (one process per GPU; the
 * reference's counterpart is the multiprocessing.Pool.map over the half-ensemble of
 * mind_the_gaps/gpmodelling.py:245-248).  Every process calls mtg_ensemble_init with the SAME
 * coordinates and seed, then one of the two calls below with its rank: from then on
 * mtg_ensemble_run evaluates only rows [rank * chunk, (rank + 1) * chunk), chunk = ceil(E * W/2 /
 * world), of every half-step's proposals and gets the others' log-probabilities (8 bytes per
 * walker and a status word) before the accept step, which every rank then takes identically:
 * all ranks hold the same chain.  A row is evaluated by the same kernel whatever the rank, but the
 * kernel is chosen by the number of rows a rank evaluates: chains agree bit for bit with the
 * one-process chain when that choice is the same (always with mtg_set_time_parallel(ctx, 0)).
 *
 *  mtg_ensemble_shard_rccl   one ncclAllGather of doubles and one of int32 per half-step, grouped,
 *                            on the context's stream: no host synchronisation in the run.  id128:
 *                            the 128-byte ncclUniqueId made by ONE process with
 *                            mtg_rccl_unique_id and handed to the others by the caller (any
 *                            channel: torch.distributed.broadcast, MPI, a file).  Collective:
 *                            returns when every rank of `world` has called it.  librccl.so.1 is
 *                            looked up at run time, the copy already loaded in the process first
 *                            (mtg_rccl_load(path) names one explicitly before anything else loads it).
 *  mtg_ensemble_shard_host   the exchange is a callback of the caller (another transport: gloo,
 *                            MPI ...; or processes that share one GPU, which RCCL refuses): after
 *                            each half-step's solve the library hands it host arrays lnp[count],
 *                            status[count] with rows [lo, hi) filled in; it must fill in all others
 *                            (the chunk layout above) and return 0.  Synchronises the stream twice per
 *                            half-step.
 *  mtg_ensemble_unshard      back to every row on this process.  mtg_ensemble_init also resets it.
 */
typedef int (*mtg_exchange_fn)(void *user, double *lnp, int32_t *status, int64_t count, int64_t lo, int64_t hi);
MTG_API int mtg_rccl_load(const char *path);
MTG_API int mtg_rccl_unique_id(void *id128);
MTG_API int mtg_ensemble_shard_rccl(mtg_ctx *ctx, const void *id128, int rank, int world);
MTG_API int mtg_ensemble_shard_host(mtg_ctx *ctx, int rank, int world, mtg_exchange_fn fn, void *user);
MTG_API int mtg_ensemble_unshard(mtg_ctx *ctx);
/* How the resident ensembles are sharded: kind 0 none / 1 RCCL / 2 host callback, this process's rank and the
 * world it was given, and -- RCCL -- the communicator's own idea of its size (ncclCommCount).  Any pointer may
 * be NULL. */
MTG_API int mtg_ensemble_shard_info(const mtg_ctx *ctx, int *kind, int *rank, int *world, int *comm_ranks);
/* Time the RCCL exchange: HIP events on the launch stream around the first `capacity` all-gather pairs of the
 * following mtg_ensemble_run calls; mtg_ensemble_shard_profile_read waits for them, writes their durations (ms)
 * and returns how many were recorded, ending the session.  (What an exchange costs on the stream -- including
 * the wait for the slowest rank's solve -- not the wire time alone.) */
MTG_API int mtg_ensemble_shard_profile(mtg_ctx *ctx, int capacity);
MTG_API int mtg_ensemble_shard_profile_read(mtg_ctx *ctx, int capacity, double *exchange_ms);

/*
 * Posterior-predictive light-curve simulation, the step before the hot path in the
 * Protassov loop: GPModelling.generate_from_posteriors (gpmodelling.py:478-539) ->
 * Simulator.generate_lightcurve + add_noise (simulator.py:300-420, get_fft :468-501),
 * Gaussian flux PDF (Timmer & Koenig 1995), for S posterior samples theta[S][P] of the
 * context's model on the context's (shared) sampling of N epochs.
 *   nfft, sim_dt   length and step of the fine regular grid (len(sim_timestamps), sim_dt)
 *   seg_len        fine samples in the randomly cut segment (sim_duration / sim_dt)
 *   win_lo/win_hi  [N] fine-sample ranges [lo, hi) of the segment averaged into every
 *                  epoch (the `strategy` windows of simulator.py:266-267, 340-367)
 *   noise_kind     0 none, 1 Gaussian(sigma_noise), 2 Poisson over exposures[N], 3 Kraft (Poisson with background and the
 *                  Bayesian estimates of the faint epochs: mtg_set_simulate_kraft first)
 *   clean          [S][N] noise-free rates or NULL; rates, dy [S][N]: noisy rates and
 *                  their 1-sigma errors (host buffers); lc_means [S] or NULL
 *   make_resident  != 0: the simulated set becomes the context's light curves (frozen mean
 *                  = each curve's average, yerr = dy + 1e-12), ready for
 *                  mtg_loglike_batch / mtg_ensemble_* with no host round trip
 *   psd_table      NULL: the PSD is celerite's Term.get_psd of the context's model at theta[S][P].  Otherwise
 *                  (any callable PSD, simulator.py:149,272-280) the spectrum tabulated by the caller at the
 *                  angular frequencies 2 pi k / (nfft sim_dt), k = 0 .. nfft/2: [psd_rows][nfft/2 + 1] with
 *                  psd_rows = 1 (shared) or S; theta and the model are then not used
 *   segments       NULL, or [S][seg_len]: the cut segments themselves as rates on the fine grid (what the
 *                  reference hands to its E13 flux-PDF adjustment before down-sampling)
 * The inverse FFTs are one batched hipFFT plan; random numbers are Philox4x32-10 keyed by `seed`.
 */
MTG_API int mtg_simulate_tk95(mtg_ctx *ctx, int64_t S, const double *theta, const double *psd_table, int64_t psd_rows,
                              uint64_t seed, int64_t nfft, double sim_dt, double mean_rate, int64_t seg_len,
                              const int32_t *win_lo, const int32_t *win_hi, int noise_kind, double sigma_noise,
                              const double *exposures, double *clean, double *rates, double *dy, double *lc_means,
                              double *segments, int make_resident);
/*
 * Test entry: the down-sampling step of mtg_simulate_tk95 alone on caller-provided fine-grid series
 * [S][nfft] with the segment starting at fine sample `start`: rates[S][N] = plain average of
 * series[s][start + lo .. start + hi) per epoch (simulator.py:340-367).
 */
MTG_API int mtg_tk95_observe_series(mtg_ctx *ctx, int64_t S, int64_t nfft, int64_t seg_len, int64_t start,
                                    const double *series, const int32_t *win_lo, const int32_t *win_hi, double *rates);

/*
 * celerite.GP.predict(y, return_var=True) at the training times, as
 * GPModelling.standarized_residuals calls it (gpmodelling.py:366): conditional mean
 * mu[b][n] (WITHOUT the per-light-curve y_offset, which the caller adds back) and
 * variance var[b][n] (without jitter; the caller adds kernel.jitter when
 * include_noise) for B parameter vectors, in O(N J^2) per vector through the
 * factorisation instead of celerite's dense N x N cross-covariance.  Rows outside
 * the prior or with a non positive-definite covariance get their status and no
 * output.
 */
MTG_API int mtg_predict(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, double *mu,
                        double *var, int32_t *status);

/*
 * celerite.GP.apply_inverse(y) / CholeskySolver.solve: x <- K^-1 x for M right-hand sides,
 * x[N][M] (row n = sample n of every right-hand side), K the covariance of light curve
 * `lc_index` at parameter vector `theta`, in O(N J^2 + N J M) from the same factorisation
 * mtg_predict uses.  It is what the full covariance of celerite's predict at NEW times is
 * made of (K_** - K_* K^-1 K_*^T, a dense M x M object by definition; the host side assembles
 * it); the mean and the variance at new times come from mtg_predict_at without K_*.
 * *status: MTG_ST_* of the parameter vector (nothing is written to x unless MTG_ST_OK).
 */
MTG_API int mtg_apply_inverse(mtg_ctx *ctx, const double *theta, int32_t lc_index, int64_t M, double *x,
                              int32_t *status);

/*
 * celerite.GP.predict(y, t=ts, return_var=True) at M new times ts[M] (any order, duplicates
 * allowed, shared by all rows; a non-finite one is MTG_E_ARG) for B parameter vectors:
 * conditional mean mu[b][m] (WITHOUT the per-light-curve y_offset, as mtg_predict; a fitted
 * linear mean is included) and celerite's noise-free variance var[b][m] = k(0) - k_*^T K^-1 k_*
 * (var == NULL: mean only).  celerite forms the dense cross-covariance K_* [M][N] and solves
 * with it; here the factorisation's forward and backward recurrences are checkpointed every
 * 64 samples and each new time replays at most 64 stored steps on either side:
 * O((N + 64 M) J^2) per vector, device memory O(B (N J + N J^2 / 64 + M)), nothing of size
 * N x M on either side.  Large batches are processed in slabs of rows.  Rows outside the prior
 * or with a non positive-definite covariance get their status and read back NaN.
 */
MTG_API int mtg_predict_at(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index,
                           int64_t M, const double *ts, double *mu, double *var, int32_t *status);

/*
 * celerite.GP.predict(y, t=ts, return_var=True, kernel=k_c): the conditional mean and variance of ONE COMPONENT of the
 * sum kernel given the data, for T components in one call ("the QPO and the red noise separately").  Component c is
 * the sum k_c of the terms whose bit is set in term_mask[c] -- bit k = term k of the model in the `+` order of
 * mtg_set_model; 1 <= T <= 32; a bit at or beyond nterms other than MTG_TERMS_MEAN is MTG_E_ARG; a mask of 0 is
 * allowed.  With r = y - mean and K the covariance of the WHOLE model (never of the component),
 *   mu[b][c][m]  = k_c(t*_m, t) K^-1 r          (+ the constant or linear mean at t*_m with MTG_TERMS_MEAN in the mask;
 *                                                the per-light-curve y_offset is excluded, as in mtg_predict_at)
 *   var[b][c][m] = k_c(0) - k_c,*^T K^-1 k_c,*  (var == NULL: means only)
 * both noise-free, like mtg_predict_at: a MTG_TERM_JITTER term contributes nothing to either, and a mask of 0 or of
 * jitter terms alone gives mu = 0 (or the mean) and var = 0.  The means of single-term masks add up to the all-terms
 * mean; the variances do not (the components are correlated given the data).
 * celerite forms the dense M x N cross-covariance of the sub-kernel.  Here the factorisation, its checkpoints and the
 * replay to t* are mtg_predict_at's and are done once per (row, time); only the generators at t* and k(0) are
 * restricted to the slots of the selected terms, J^2 operations per mask: T components cost little more than one
 * mtg_predict_at plus the T times larger copy back.  Which slots a term owns is decided per row where the slots are
 * handed out (an SHO term owns two real slots when over-damped, a complex pair otherwise).  With every term selected
 * and MTG_TERMS_MEAN, mu and var are bit for bit mtg_predict_at's; every (row, time, mask) result is independent of B,
 * M, T, the order of ts and the order of the masks.
 * Everything else as mtg_predict_at: ts in any order, duplicates allowed, a non-finite one is MTG_E_ARG; rows in
 * slabs; rows outside the prior or not positive definite keep their status and read back NaN; ranks above MTG_MAX_J
 * and profile means return MTG_E_UNSUPPORTED.  mtg_last_solver names "mtg_predict_terms_eval_kernel<J>".
 */
#define MTG_TERMS_MEAN (1u << 31)
MTG_API int mtg_predict_terms(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int T,
                              const uint32_t *term_mask /* [T] */, int64_t M, const double *ts,
                              double *mu /* [B][T][M] */, double *var /* [B][T][M] or NULL */, int32_t *status);

/*
 * celerite.GP.sample(size) -> solver.dot_L: B realisations of the process itself, y[b] ~ N(mean, K(theta[b])) on the
 * sampling and error bars of light curve lc_index[b] (NULL = all 0), K = k(t_i - t_j) + diag(sigma^2 + jitter) as in
 * the likelihood -- a draw is a noisy light curve, as celerite's is.  With the factorisation K = L diag(D) L^T the
 * draw is y = mean + L sqrt(D) q, q ~ N(0, I): the forward sweep of mtg_predict driven by one normal per sample,
 * O(N J^2) per draw, exact for any sampling (no FFT, no regular grid: what mtg_simulate_tk95 approximates).  The data
 * y of the resident light curves are not read.  y[b][n] includes a fitted constant or linear mean and EXCLUDES the
 * per-light-curve y_offset, which the caller adds back (as for mtg_predict).
 *   normals  [B][N] standard normals of the caller (host), or NULL: drawn on the device from Philox4x32-10 keyed by
 *            `seed`, counter (n / 2, 12, low word, high word of first_index + b) with first_index that of
 *            mtg_set_stream_base; one block gives the Box-Muller pair q[2k], q[2k + 1].  Draw b therefore depends on
 *            (seed, first_index + b, theta[b], its light curve) alone: not on B, nor on how a job is cut over calls
 *            or GPUs.  seed is not used with the caller's normals.
 * Large batches are processed in slabs of rows (device memory O(slab N)).  Rows outside the prior or with a non
 * positive-definite covariance get their status and read back NaN.
 */
MTG_API int mtg_gp_draw(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, uint64_t seed,
                        const double *normals /* [B][N] or NULL: Philox */, double *y /* [B][N] */, int32_t *status);

/*
 * The whitened (one-step-ahead) residuals of B rows and their goodness-of-fit diagnostics: the inverse of mtg_gp_draw.
 * With K = L diag(D) L^T and r = y - mean(t) (the fitted constant or linear mean),
 *     q = D^-1/2 L^-1 r,    q[b][n] = (y_n - E[y_n | y_1 .. y_n-1]) / sqrt(Var[y_n | y_1 .. y_n-1]):
 * under the model the q_n are i.i.d. N(0, 1) -- what a KS test against the normal and an autocorrelation band of
 * +-1.96 / sqrt(N) assume (the smoothing residual of mtg_predict is neither independent nor of unit variance) -- and
 * lnL = -1/2 (stats[1] + stats[2] + N ln 2 pi).  O(N J^2) per row: the forward sweep of mtg_gp_draw with the
 * innovation taken from the data.
 *   y      [B][N] data (host) WITHOUT the per-light-curve y_offset, as mtg_gp_draw returns them; NULL: the resident
 *          data of light curve lc_index[b].  The same data give the same bits either way.
 *   q      [B][N] or NULL.
 *   acf    [B][K] or NULL (then K must be 0): acf[b][k - 1] = sum_{n < N - k} q_n q_{n+k} / sum_n q_n^2, k = 1 .. K,
 *          1 <= K <= N - 1 (matplotlib's acorr: no mean subtracted, normalised by lag 0).  O(N K) per row.
 *   stats  [B][MTG_WHITEN_NSTATS] or NULL:
 *          0 sum q   1 sum q^2   2 sum ln D   3 sum q^3   4 sum q^4   7 max |q|      (summed in sample order)
 *          5 D+ = max_i (i / N - Phi(q_(i)))   6 D- = max_i (Phi(q_(i)) - (i - 1) / N)   (the one-sample KS distances
 *          of the sorted row against the standard normal, Phi(x) = erfc(-x / sqrt 2) / 2).  D+ and D- are formed
 *          where the residuals are on the device anyway, that is when q or acf is asked for; a call for stats alone
 *          stores nothing of size N, costs one sweep and returns NaN in slots 5 and 6.
 * K outside its range, K != 0 without acf, and q, acf and stats all NULL are MTG_E_ARG; B == 0 is MTG_OK.  Rows outside
 * the prior or with a non-positive pivot keep their status and read back NaN in every output.  A row's outputs do not
 * depend on the batch it travels in.  Large batches go in slabs of rows (device memory O(slab N): up to 256 MiB each
 * for the given y, q, its sorted copy and the lags; what exceeds 64 MiB is freed when the call returns); where D+ and
 * D- are formed a slab holds fewer than 2^31 samples (the sort's item count), down to one row, and N >= 2^31 is
 * MTG_E_ARG.  Ranks above MTG_MAX_J and profile means return MTG_E_UNSUPPORTED.  mtg_last_solver names
 * "mtg_whiten_kernel<J>".
 */
#define MTG_WHITEN_NSTATS 8
MTG_API int mtg_whiten(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index,
                       const double *y      /* [B][N] host, or NULL: the resident data of lc_index[b] */,
                       double *q            /* [B][N] or NULL */,
                       int K, double *acf   /* [B][K] or NULL (then K must be 0) */,
                       double *stats        /* [B][MTG_WHITEN_NSTATS] or NULL */,
                       int32_t *status);

/*
 * celerite.GP.sample_conditional(y, t): B draws of the process GIVEN the resident data, at M new times ts[M] (any
 * order, duplicates allowed, shared by all rows; a non-finite one is MTG_E_ARG; M == 0 is MTG_OK and writes nothing).
 * celerite forms the dense M x N cross-covariance and factors the dense M x M conditional covariance; here Matheron's
 * rule makes it two linear sweeps.  A joint prior draw (y~, f*) at the light curve's epochs (noisy: sigma^2 + jitter on
 * the diagonal) and at the unique new times (latent: diagonal 0) comes from the factor step of mtg_gp_draw on the merged
 * series, a new time equal to an epoch after it; then y*[b][m] = f* + mu, mu the conditional mean of mtg_predict_at
 * for the light curve y - y~.  O((N + 64 M) J^2) per draw, device memory O(slab (N J + N J^2 / 64 + N + M)), nothing of
 * size N x M or M x M.  y*[b][m] includes a fitted constant or linear mean and EXCLUDES the per-light-curve y_offset
 * (as mtg_predict_at); entries of ts with the same time receive the same value.
 *   normals  [B][N + M] standard normals of the caller (host): row b holds those of the N epochs in epoch order, then
 *            one per entry of ts; a time given more than once takes the normal of its first entry and the others are
 *            not read.  NULL: drawn on the device from Philox4x32-10 keyed by `seed`, counter (k, purpose, low word,
 *            high word of first_index + b), first_index that of mtg_set_stream_base: block k of purpose
 *            MTG_PURPOSE_GP_COND_EPOCH gives the Box-Muller pair of epochs 2k, 2k + 1, block k of
 *            MTG_PURPOSE_GP_COND_NEW that of the unique new times of rank 2k, 2k + 1 in ascending order.  Draw b
 *            therefore depends on (seed, first_index + b, theta[b], its light curve, the set of new times) alone: not
 *            on B, on slabs, or on the order of ts.
 * Statuses as mtg_predict_at: rows outside the prior or with a non-positive pivot (of K, or of the merged series) get
 * their status and read back NaN.  mtg_last_solver names the sweep, "mtg_gp_cond_draw_kernel<J>".
 */
#define MTG_PURPOSE_GP_COND_EPOCH 13 /* Philox counter word c1; 12 is mtg_gp_draw's */
#define MTG_PURPOSE_GP_COND_NEW 14
MTG_API int mtg_gp_cond_draw(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int64_t M,
                             const double *ts, uint64_t seed, const double *normals /* [B][N + M] or NULL: Philox */,
                             double *y /* [B][M] */, int32_t *status);

/*
 * celerite.GP.grad_log_likelihood for B parameter vectors at once: out[b] = lnL(theta[b]) of light curve lc_index[b]
 * (NULL = all 0) and grad[b][p] = d lnL / d theta[b][p] for the model's P free parameters, the derivative of the
 * float64 recurrence itself (no finite differences).  Against a quad-precision truth every component is within
 * 70 sqrt(N) u G_p (u = 2^-53, G_p the sum of the magnitudes of the terms that make the component up) on ordinary rows;
 * where the float64 formulation is itself ill-conditioned the gradient is, like lnL, as good as that formulation and no
 * better: an SHO term within 1e-3 of Q = 1/2 in ln Q (3e4 in those units: 1e-8 relative in the ln Q component),
 * amplitudes of e^10 to e^20 over the noise with c dx down to 1e-9 (1e6: 1e-8 relative), and frequencies beyond 1e4 rad
 * per step, where rounding d to a double already moves the phases (tests/test_loglike_grad_gpu.py).  One lane per (row, free parameter) sweeps the factorisation together with its directional
 * derivative, state in registers: O(N J^2) per lane, no workspace that grows with N; the coefficient tangents
 * ([coefficient slots][B P] doubles) belong to the context and grow on demand.  The box prior is flat, so add_prior
 * only decides which rows are rejected: a row outside the prior gets MTG_ST_PRIOR, out = -inf and a gradient of
 * NaN; a row with a non-positive pivot MTG_ST_NOTPD, -inf and NaN.  A row's values do not depend on the batch it
 * travels in.  An SHO term is differentiated on the side of Q = 1/2 the row is on.  Models of rank
 * J = n_real + 2 n_complex > 6 return MTG_E_UNSUPPORTED (the tangent state no longer fits the register file);
 * mtg_last_solver names the kernel, "mtg_loglike_grad_kernel<J>".
 */
MTG_API int mtg_loglike_grad(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int add_prior,
                             double *out /* [B] */, double *grad /* [B][P] */, int32_t *status);

/*
 * astropy's LombScargle(t, y, dy, fit_mean=True, center_data=True, nterms=1, normalization=...).power(freqs): the
 * generalised (floating-mean) Lomb-Scargle periodogram of EVERY resident light curve l at every freqs[k] (host, cycles
 * per unit of time) -- the set of mtg_set_lightcurves or the simulated one mtg_simulate_tk95(make_resident) left.  A
 * model need not be set.
 *   weighted != 0: w_n = sigma_n^-2 / sum sigma^-2 from the resident error bars; weighted == 0: w_n = 1 / N (dy = None).
 *   ybar = sum w y, r = y - ybar, YY = sum w r^2, and with c_n, s_n = cos, sin(2 pi f (t_n - t_0))
 *     C = sum w c,  S = sum w s,  YC = sum w r c,  YS = sum w r s,
 *     CC = sum w c^2 - C^2,  SS = sum w s^2 - S^2,  CS = sum w c s - C S,
 *     p = (SS YC^2 + CC YS^2 - 2 CS YC YS) / (CC SS - CS^2)
 * the tau-free form of Zechmeister & Kuerster (2009), algebraically astropy's YC_tau^2 / CC_tau + YS_tau^2 / SS_tau and
 * invariant under a shift of the times and of y: the elapsed time t - t_0 is used, and the y_offset of the resident set
 * does not matter.  normalization:
 */
#define MTG_LS_STANDARD 0   /* p / YY, in [0, 1]                                  */
#define MTG_LS_MODEL    1   /* p / (YY - p)                                       */
#define MTG_LS_LOG      2   /* -log(1 - p / YY)                                   */
#define MTG_LS_PSD      3   /* p * 0.5 * sum(1 / sigma_n^2)  (unweighted: 0.5 N)  */
/*
 * The phase is formed in cycles: f (t_n - t_0) is taken exactly (product and fma remainder), its integer part is
 * dropped before anything is rounded, and the fraction goes through the (cos, sin) table of the sweep; what is left is
 * the rounding of t_n - t_0 itself (exact for times within a factor of two of each other).  Against a 50-digit
 * evaluation of astropy's form the standard power is within max(10 rho, 64 sqrt(N) u), u = 2^-53, rho the error of the
 * same formula in plain float64 (tests/test_lomb_scargle_gpu.py), also with f T ~ 1e6 cycles.
 * One lane owns a frequency; the samples are walked in ascending order, in chunks of 256 whose partial sums are added
 * to a running total; on shared sampling a lane carries a tile of light curves, so that one (cos, sin) pair serves the
 * whole tile.  power[l][k] depends on (light curve l, freqs[k], normalization, weighted) alone, bit for bit: not on L,
 * on which light curves share the tile, on F, on the order of freqs, or on whether the sampling is stored shared or per
 * light curve.
 *   power       [L][F] (host) or NULL
 *   peak_power  [L] or NULL: the maximum of row l;  peak_index [L] or NULL: the first k that attains it.  Both are
 *               reduced on the device: with power == NULL nothing of size L F comes back, and the device workspace is
 *               bounded -- the light curves are processed in slabs.
 * A frequency at which CC SS - CS^2 is not positive gives NaN in that entry; the peak passes NaN entries over (a row of
 * nothing else: NaN and -1).
 * MTG_E_STATE without light curves; MTG_E_ARG for F < 1, a frequency that is not finite or <= 0, an unknown
 * normalization, N < 4 (three points are fitted exactly: the denominator is 0), and all three outputs NULL.  Runs on
 * the context's stream, ordered with its other calls; the resident set is only read.  mtg_last_solver names
 * "mtg_lomb_scargle_kernel<R>" (R light curves per lane), mtg_last_kernel_ms runs from the pre-pass to the last slab's
 * powers and peaks (with one slab: kernels only; the copies of earlier slabs lie inside it).
 */
MTG_API int mtg_lomb_scargle(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host, cycles per unit time */,
                             int normalization, int weighted,
                             double *power /* [L][F] host, or NULL */,
                             double *peak_power /* [L] or NULL */, int64_t *peak_index /* [L] or NULL */);

/*
 * mtg_lomb_scargle with nterms = K phase-tied harmonics per frequency: astropy's LombScargle(fit_mean=True,
 * center_data=True, nterms=K).power(freqs, method="chi2"), the batched form of fitting a profile that is not a sinusoid
 * (eclipses, pulses, QPO harmonics).  Weights, ybar, r and YY as above; with phi_n = 2 pi f (t_n - t_0) and the design row
 *   x_n = (1, sin phi_n, cos phi_n, ..., sin K phi_n, cos K phi_n),   A = sum w x x^T,   b = sum w r x,   p = b^T A^-1 b
 * and the four normalizations applied to p as above.  b_0 = sum w r is zero, so the bias column is eliminated first (the
 * Schur complement A_hh - h h^T, the step CC = sum w c^2 - C^2 above) and the 2K x 2K rest is factored by Cholesky;
 * for K = 1 this is algebraically the formula above.  Every entry of A is half a sum or difference of
 * C_m = sum w cos m phi and S_m = sum w sin m phi, m <= 2 K: a lane accumulates those 4 K sums and 2 K data sums per light
 * curve.  The base pair (cos phi, sin phi) is mtg_lomb_scargle's bit for bit; harmonic m follows from harmonic m - 1 by
 * one complex multiplication by it.  Against a 50-digit evaluation the standard power is within
 * max(10 rho, 64 sqrt(N) u kappa), kappa the 2-norm condition number of A (tests/test_lomb_scargle_multi_gpu.py).
 *   nterms == 1 runs mtg_lomb_scargle's kernel: the result is mtg_lomb_scargle's bit for bit.
 * Outputs, slabs, peak reduction and invariance as for mtg_lomb_scargle: power[l][k] depends on (light curve l, freqs[k],
 * nterms, normalization, weighted) alone, bit for bit.  A frequency at which a pivot of the factorisation is not positive
 * gives NaN in that entry.  Errors as for mtg_lomb_scargle, and MTG_E_ARG for nterms outside 1 .. MTG_LS_MAX_TERMS and for
 * N < 2 nterms + 2 (2 nterms + 1 samples are fitted exactly).  mtg_last_solver names "mtg_lomb_scargle_multi_kernel<K,R>"
 * (R light curves per lane: csrc/mtg_ls_plan.h), or mtg_lomb_scargle's kernel for nterms == 1.
 */
enum { MTG_LS_MAX_TERMS = 5 };   /* (not one of the MTG_LS_* normalization macros) */
MTG_API int mtg_lomb_scargle_multi(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host, cycles per unit time */,
                                   int nterms /* 1 .. MTG_LS_MAX_TERMS */, int normalization, int weighted,
                                   double *power /* [L][F] host, or NULL */,
                                   double *peak_power /* [L] or NULL */, int64_t *peak_index /* [L] or NULL */);

/*
 * Epoch folding (Leahy et al. 1983) of every resident light curve at freqs [F]: fold at the trial frequency, bin by
 * phase, and ask how much of the variance the binned profile explains -- the statistic for eclipses, dips and narrow
 * pulses, where a few harmonics are a poor basis.  Weights w_n, ybar, r_n = y_n - ybar, YY = sum w r^2 and sw exactly as
 * in mtg_lomb_scargle (weighted: sigma_n^-2 / sum sigma^-2, else 1 / N).  With te_n = fl(t_n - time_0) (one IEEE
 * subtraction) the bin of sample n at frequency f is
 *   b_n = floor(nbins frac(f te_n)),   the product f te_n taken EXACTLY, frac(x) = x - floor(x) in [0, 1) also for te < 0
 * -- a function of the stored doubles alone: a sample whose rounded product crosses a bin edge still lands in the bin of
 * the exact one (csrc/mtg_ls_phase.h, mtg_cycles_bin: |f te| < 2^47, and what it takes to miss).  Per bin
 *   W_b = sum_{n in b} w_n,   S_b = sum_{n in b} w_n r_n,   c_b = #{n in b}        (samples ascending, one addition each)
 *   p = sum_{b : c_b > 0} S_b^2 / W_b                                              (bins ascending, as (S_b S_b) / W_b)
 * (the kernel skips a bin by W_b > 0, the same unless a weight underflows), and
 *   power = p / YY (standard), p / (YY - p) (model), -log(1 - p / YY) (log), p sw / 2 (psd)
 * with the MTG_LS_* constants: p = YY - chi^2 of the best piecewise-constant profile, the quantity mtg_lomb_scargle
 * normalises.  Leahy's chi^2 is 2 x psd.  YY = 0 behaves as in mtg_lomb_scargle (0 / 0).
 * Outputs, slabs, stream, the read-only resident set and the peak reduction (NaN passed over; a row of nothing else:
 * NaN and -1) as for mtg_lomb_scargle.  power[l][k] depends on (light curve l, freqs[k], nbins, time_0, normalization,
 * weighted) alone, bit for bit: not on L, the tile, F, the order of freqs, or how the sampling is stored.
 * mtg_last_solver names "mtg_epoch_fold_kernel<R,weighted> lanes T" (R light curves per lane, T lanes per workgroup:
 * csrc/mtg_ef_plan.h), mtg_last_kernel_ms times the pre-pass and the sweeps.
 * MTG_E_STATE without light curves; MTG_E_ARG for F < 1, a frequency that is not finite or <= 0, nbins outside
 * 2 .. MTG_EF_MAX_BINS, a time_0 that is not finite, an unknown normalization, N < 2, or all outputs NULL; the context
 * works as before after an error.
 */
enum { MTG_EF_MAX_BINS = 32 };
MTG_API int mtg_epoch_fold(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host, cycles per unit time */,
                           int nbins /* 2 .. MTG_EF_MAX_BINS */, double time_0, int normalization, int weighted,
                           double *power /* [L][F] host, or NULL */,
                           double *peak_power /* [L] or NULL */, int64_t *peak_index /* [L] or NULL */);

/*
 * The folded profiles themselves: mtg_epoch_fold's sweep storing the bins instead of reducing them.  Each output NULL or
 * [L][F][nbins] on the host: count = c_b, wsum = W_b, wrsum = S_b as above (the weighted mean of bin b is
 * ybar + S_b / W_b), varsum = sum_{n in b} sigma_n^2 (the error of an unweighted bin mean is sqrt(varsum) / count).
 * mtg_epoch_fold's p is, bit for bit, what the formula above gives from wsum and wrsum in that order.
 * Meant for the few frequencies one looks at: every output stays whole on the device, and a call with
 * L F nbins > MTG_PF_MAX_ENTRIES (256 MiB of workspace with all four asked for) is refused with MTG_E_ARG.  Other errors
 * as for mtg_epoch_fold.
 */
#define MTG_PF_MAX_ENTRIES ((int64_t)1 << 23)
MTG_API int mtg_phase_fold(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host */, int nbins, double time_0, int weighted,
                           int64_t *count /* [L][F][nbins] or NULL */, double *wsum /* W_b */, double *wrsum /* S_b */,
                           double *varsum /* sum of sigma^2 per bin */);

/*
 * Foster's weighted wavelet Z-transform (Foster 1996, AJ 112, 1709) of every resident light curve: the time-frequency
 * view of a periodicity that comes, goes or drifts.  At one (tau, f) it is mtg_lomb_scargle's floating-mean fit with
 * every sample also weighted by a Gaussian window centred on tau whose width is a fixed number of cycles.
 * Inputs: freqs [F] > 0 (cycles per unit time), the window centres taus [T] (finite, any order, inside or outside the
 * time span), a decay constant c >= 0 (Foster's 1 / (8 pi^2) = MTG_WWZ_DECAY) and the weighting: statistical weights
 * s_n = sigma_n^-2 (weighted != 0) or 1.  For one (light curve, tau, f):
 *   te_n = fl(t_n - tau) (one IEEE subtraction),  z_n = f te_n (cycles),
 *   g_n = exp(-4 pi^2 c z_n^2)  (exp(-z^2 / 2) at the default c),  w_n = s_n g_n,
 *   r_n = y_n - ybar, ybar the weighted mean of mtg_lomb_scargle's pre-pass (the statistic does not depend on it
 *   mathematically; it is there for the rounding).
 * With the weighted means <a> = sum w a / sum w:
 *   C = <cos 2 pi z>, S = <sin 2 pi z>, CC = <cos^2>, CS = <cos sin>, SS = 1 - CC,
 *   X = <r>, XX = <r^2>, XC = <r cos>, XS = <r sin>,   N_eff = (sum w)^2 / sum w^2,   V_x = XX - X^2,
 * centred (CC - C^2, SS - S^2, CS - C S, XC - X C, XS - X S) and put through the 2 x 2 formula of mtg_lomb_scargle, they
 * give V_y, the variance of the fitted local sinusoid, and its coefficients (a, b).  `statistic` selects what is written:
 */
#define MTG_WWZ_POWER     0   /* P = V_y / V_x, in [0, 1]: the local generalised Lomb-Scargle power */
#define MTG_WWZ_Z         1   /* Z = (N_eff - 3) V_y / (2 (V_x - V_y)): Foster's Z                  */
#define MTG_WWZ_AMPLITUDE 2   /* sqrt(a^2 + b^2): Foster's WWA                                      */
#define MTG_WWZ_DECAY 0.012665147955292222   /* 1 / (8 pi^2) */
/*
 * A determinant that is not positive gives NaN in that entry, and so does a denominator that is not positive: V_x for
 * P, V_x - V_y for Z (a window that holds no more than the three fitted parameters, or a fit exact to the last bit; the
 * peaks pass NaN over, an infinity would be every map's peak).  Otherwise N_eff <= 3 gives whatever the formula gives.
 * With c = 0, P is mtg_lomb_scargle's standard power -- the same quantity, not the same bits: the phase origin is tau --
 * and N_eff = (sum s)^2 / sum s^2: N unweighted, less than N with error bars that differ.
 * Supported range: |f|, |t_n - tau| and their products below about 1e150.  Beyond, (4 pi^2 c f) f or te_n te_n
 * overflows, the exponent becomes inf - inf or 0 inf = NaN, nothing is cut and the entry is NaN: no error is raised.
 * Range.  Every quantity above is invariant under a common factor on the weights, so g_n is taken relative to the
 * largest weight of its (tau, f): the exponent is E_n = ((4 pi^2 c f) f) (te_n te_n - te_* te_*), te_* the te_n of
 * smallest magnitude (found once per (sampling, tau)), every operation rounded.  The largest weight is then 1 and
 * sum w >= min s: a centre in the middle of a gap at high frequency gives finite numbers, not 0 / 0 from underflow.
 * Cut.  A weight whose exponent E_n, as the device forms it, exceeds 80 ln 2 is exactly 0: a decision that depends on
 * (tau, f, sample) alone and drops less than N 2^-80 of sum w.  A cut sample adds exact zeros, so a workgroup skips
 * every chunk of 256 samples in which all its lanes' weights are cut -- the samples ascend in time, so the kept chunks are
 * one range that follows from tau and the workgroup's lowest frequency -- without changing one bit of any lane's result.
 * One lane owns a frequency, a workgroup one tau and a tile of light curves on shared sampling (csrc/mtg_wwz_plan.h);
 * samples ascending, a chunk's partial sums from zero, folded into running totals.  out[l][j][k] depends on (light
 * curve l, freqs[k], taus[j], c, statistic, weighted) alone, bit for bit: not on L, the tile, F or T, the order of freqs
 * or taus, which frequencies share a workgroup, the slabs, or whether the sampling is stored shared or per light curve.
 * Against a 50-digit evaluation of Foster's formulas as written (no cut, no rescaling) P is within
 * max(10 rho, 64 sqrt(N) u kappa), kappa the 2-norm condition number of the normalised 3 x 3 normal matrix, and N_eff
 * within 64 sqrt(N) u relative (tests/test_wwz_gpu.py).
 *   out         [L][T][F] (host) or NULL: the statistic
 *   neff        [L][T][F] (host) or NULL: N_eff
 *   peak        [L] or NULL: the maximum of light curve l's map;  peak_index [L] or NULL: the first j F + k attaining
 *               it.  Reduced on the device, NaN entries passed over (a map of nothing else: NaN and -1); with out and
 *               neff NULL nothing of size L T F comes back.  The device workspace is bounded: slabs of light curves.
 * MTG_E_STATE without light curves; MTG_E_ARG for F < 1 or T < 1, a frequency that is not finite or <= 0, a tau that is
 * not finite, a decay that is negative or not finite, an unknown statistic, N < 4, L T F beyond int64, or all outputs
 * NULL; the context works as before after an error.  mtg_last_solver names "mtg_wwz_kernel<R,weighted> lanes T",
 * mtg_last_kernel_ms runs from the pre-pass to the last slab's kernels.
 */
MTG_API int mtg_wwz(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host, cycles per unit time */,
                    int64_t T, const double *taus /* [T] host */, double decay, int statistic, int weighted,
                    double *out /* [L][T][F] host, or NULL */, double *neff /* [L][T][F] host, or NULL */,
                    double *peak /* [L] or NULL */, int64_t *peak_index /* [L] or NULL */);

/*
 * The time-lag view: sums over the pairs of samples of every resident light curve in bins of the lag, from which the
 * caller normalises the structure function SF^2(tau) = <(y_j - y_i)^2> - <sigma_i^2 + sigma_j^2> and the discrete
 * correlation function of Edelson & Krolik (1988, ApJ 333, 646) with its error.  Defined on the pairs: gaps cost
 * nothing, nothing is interpolated.  For light curve l and every pair i < j of its samples:
 *   lag and bin   tau_ij = fl(t_j - t_i), one IEEE subtraction of the stored times.  The pair belongs to bin b iff
 *                 edges[b] <= tau_ij < edges[b + 1] (plain double comparisons); pairs below edges[0] or at or above
 *                 edges[nbins] belong to no bin.  Equal times give tau = 0, which lands in bin 0 when edges[0] == 0.
 *   residuals     r_n = y_n - ybar_l, ybar_l the unweighted mean mtg_lomb_scargle's pre-pass gives with weighted = 0;
 *                 sigma_n^2 the stored variance.
 *   per bin       count = #pairs, lag = sum tau_ij, sf = sum (y_j - y_i)^2, cf = sum r_i r_j, cf2 = sum (r_i r_j)^2,
 *                 noise = sum (sigma_i^2 + sigma_j^2)
 * Raw sums only: one sweep serves SF, DCF and their errors.  count and lag depend on the sampling alone but are written
 * per light curve.  Each output is NULL or [L][nbins] on the host.
 * Operations.  With d = y_j - y_i and p = r_i r_j (rounded): sf = fma(d, d, sf), cf = cf + p, cf2 = fma(p, p, cf2),
 * noise = noise + (sigma_i^2 + sigma_j^2), lag = lag + tau.  The direct sums: the prefix-sum identity
 * sum_j (r_j - r_i)^2 = Q - 2 r_i S + n r_i^2 cancels by var / SF(tau) at the short lags where a red-noise structure
 * function is read, and is not used.
 * Order.  A row i forms its partial sum for a bin from zero with j ascending (the times ascend, so for a fixed row the
 * lag does not decrease and the bin only moves up).  The rows' partials of one (light curve, bin) are then added in an
 * order fixed by N: lane q of 256 takes the rows q, q + 256, ... ascending, then a binary tree over the lanes.  Every
 * output entry therefore depends on (light curve l, edges) alone, bit for bit: not on L, which light curves share a
 * tile, whether the sampling is stored shared or per light curve, the slabs, or which other outputs were asked for.
 * An empty bin reads exactly 0 in every sum.  No floating-point atomics.
 * The call runs on the context's stream and only reads the resident set.  A row's partials go through a device
 * workspace of at most 1 GiB -- slabs of light curves -- unless 8 light curves' alone are larger (csrc/mtg_lag_plan.h).
 * mtg_last_solver names "mtg_lag_kernel<R,all> lanes 256" (R light curves per lane; all = 0: the kernel that forms sf
 * alone, taken when nothing else is asked for), mtg_last_kernel_ms runs from the pre-pass through the last reduction.
 * Against a 50-digit evaluation every sum of c pairs is within max(10 rho, 64 sqrt(c) u) of the sum of its terms'
 * magnitudes and count is exact (tests/test_lag_gpu.py).
 * MTG_E_STATE without light curves; MTG_E_ARG for nbins outside 1 .. MTG_LAG_MAX_BINS, an edge that is not finite,
 * edges[0] < 0, edges not strictly ascending, N < 2, or all six outputs NULL; the context works as before after an error.
 */
enum { MTG_LAG_MAX_BINS = 128 };
MTG_API int mtg_lag_sums(mtg_ctx *ctx, int nbins, const double *edges /* [nbins + 1] host */,
                         int64_t *count /* [L][nbins] or NULL */, double *lag /* [L][nbins] or NULL */,
                         double *sf     /* [L][nbins] or NULL */, double *cf  /* [L][nbins] or NULL */,
                         double *cf2    /* [L][nbins] or NULL */, double *noise /* [L][nbins] or NULL */);

/*
 * The lag between TWO series on different irregular samplings -- what Edelson & Krolik (1988) wrote the discrete
 * correlation function for: sums over the pairs (resident sample i, companion sample j) of every resident light curve l
 * and a companion series given with the call, in bins of the signed lag.  The companion has M samples at the ascending
 * times t2 (equal times allowed) and the values y2: one row for every light curve (L2 == 1) or a row per light curve
 * (L2 == L; row l goes with light curve l).  It is uploaded for the call and not kept.
 *   lag and bin   tau_ij = fl(t2_j - t_i), one IEEE subtraction; positive when the companion lags the resident series.
 *                 The pair belongs to bin b iff edges[b] <= tau_ij < edges[b + 1]; edges may be negative; a pair outside
 *                 [edges[0], edges[nbins]) belongs to no bin.  Every (i, j) is a pair: there is no i < j.
 *   residuals     r_i = y_i - ybar_l as in mtg_lag_sums; s_j = y2_j - ybar2, with ybar2 what the same unweighted
 *                 pre-pass gives for the companion row taken as a light curve of M samples.
 *   per bin       count = #pairs, lag = sum tau_ij, cf = sum r_i s_j, cf2 = sum (r_i s_j)^2, and the local moments
 *                 sa = sum r_i, sb = sum s_j, saa = sum r_i^2, sbb = sum s_j^2 over the pairs of the bin, from which
 *                 the host forms the locally normalised correlation of Lehar et al. (1992) and Welsh (1999).
 * Operations.  With p = r_i s_j (rounded): cf = cf + p, cf2 = fma(p, p, cf2), sb = sb + s_j, sbb = fma(s_j, s_j, sbb),
 * lag = lag + tau.  A row i contributes fl(r_i c) to sa and fl(fl(r_i^2) c) to saa, c its pair count in the bin: this is
 * the definition.
 * Order.  A row i forms its partial for a bin from zero with j ascending (for a fixed row the lag does not decrease, so
 * the bin only moves up).  The rows' partials of one (light curve, bin) are added as in mtg_lag_sums: lane q of 256 takes
 * the rows q, q + 256, ... ascending, then a binary tree over the lanes.  Every output entry depends on (resident light
 * curve l, its companion row, t2, edges) alone, bit for bit: not on L, which light curves share a tile, L2 == 1 or
 * L2 == L with identical rows, whether the resident sampling is stored shared or per light curve, the slabs, or which
 * other outputs were asked for.  An empty bin reads exactly 0 in every sum.  No floating-point atomics.
 * With edges[0] > 0 and the companion equal to the resident light curve (M == N, the same times and values), count, lag,
 * cf and cf2 equal mtg_lag_sums' bit for bit.
 * The call runs on the context's stream and only reads the resident set.  Workspace and slabs as mtg_lag_sums
 * (csrc/mtg_cross_plan.h).  mtg_last_solver names "mtg_cross_kernel<R,per,all> lanes 256" (R light curves per lane;
 * per = 1: a companion row per light curve, taken when L2 == L > 1; all = 0: the kernel that forms count, lag, cf and cf2
 * alone, taken when no local moment is asked for), mtg_last_kernel_ms runs from the pre-pass through the last reduction.
 * Against an exact evaluation every sum of c pairs is within max(10 rho, 64 sqrt(c) u) of the sum of its terms'
 * magnitudes and count is exact (tests/test_cross_gpu.py).
 * MTG_E_STATE without light curves; MTG_E_ARG for M < 1 or M >= 2^28, L2 not 1 or L, a t2 or y2 entry that is not
 * finite, t2 descending, nbins outside 1 .. MTG_LAG_MAX_BINS, an edge that is not finite, edges not strictly ascending,
 * or all eight outputs NULL -- the message names the offending index; the context works as before after an error.
 */
MTG_API int mtg_cross_sums(mtg_ctx *ctx, int64_t M, const double *t2 /* [M] host, ascending */,
                           int64_t L2 /* 1 or L */, const double *y2 /* [L2][M] host */,
                           int nbins, const double *edges /* [nbins + 1] host, may be negative */,
                           int64_t *count /* [L][nbins] or NULL */, double *lag /* [L][nbins] or NULL */,
                           double *cf     /* [L][nbins] or NULL */, double *cf2 /* [L][nbins] or NULL */,
                           double *sa     /* [L][nbins] or NULL */, double *sb  /* [L][nbins] or NULL */,
                           double *saa    /* [L][nbins] or NULL */, double *sbb /* [L][nbins] or NULL */);

/*
 * The interpolated cross-correlation function (ICCF) of Gaskell & Peterson (1987, ApJS 65, 1) and White & Peterson (1994,
 * PASP 106, 879) of every resident light curve l and a companion series given with the call, on a grid of K lags: the
 * measure whose peak and centroid above 0.8 of the peak reverberation mapping quotes as the lag (Peterson et al. 1998,
 * PASP 110, 660).  It is the opposite trade to mtg_cross_sums: the resolution is the lag grid's, not a bin's, and the
 * price is that one series is LINEARLY INTERPOLATED at the other's shifted times.  Interpolation across a gap invents
 * data: n_a and n_b tell how many samples each half used, and the statistic is to be calibrated against simulated light
 * curves on the same sampling (ppp.iccf_significance), not read against a textbook distribution.
 * The companion has M samples at the ascending times t2 (equal times allowed) and the values y2: one row for every light
 * curve (L2 == 1) or a row per light curve (L2 == L); it is uploaded for the call and not kept.  The resident times t_i
 * ascend (equal times allowed, as they are stored).  The lags tau_k are finite, in any order, duplicates allowed; a
 * positive lag means the companion lags the resident series, as in mtg_cross_sums.
 *   residuals     r_i = y_i - ybar_l and s_j = y2_j - ybar2, the unweighted pre-pass means of mtg_cross_sums.
 *                 (Interpolation is linear: interpolating residuals is interpolating values.)
 *   interpolant   I(series, x) of a series (u_n, z_n), n < P, at u_0 <= x <= u_{P-1}: p = the largest index with u_p <= x
 *                 (plain double comparisons); p == P - 1: z_p; otherwise w = (x - u_p) / (u_{p+1} - u_p) and the value
 *                 fma(w, z_{p+1} - z_p, z_p), every operation rounded.  The denominator is positive by construction; at
 *                 a repeated time the LAST of the group is the left node -- this is the definition.  Outside
 *                 [u_0, u_{P-1}] there is no value: nothing is extrapolated.
 *   half A        (the companion interpolated) for every i with x = fl(t_i + tau_k) inside [t2_0, t2_{M-1}]:
 *                 a_i = r_i, b_i = I(companion residuals, x); i ascending.
 *   half B        (the resident series interpolated) for every j with x = fl(t2_j - tau_k) inside [t_0, t_{N-1}]:
 *                 a_j = I(resident residuals, x), b_j = s_j; j ascending.
 *   sums          over the samples of a half in that order, sequentially from zero: n += 1, Sa = Sa + a, Sb = Sb + b,
 *                 Saa = fma(a, a, Saa), Sbb = fma(b, b, Sbb), Sab = fma(a, b, Sab).
 *   r of a half   C = Sab - (Sa Sb) / n, Va = Saa - (Sa Sa) / n, Vb = Sbb - (Sb Sb) / n, r = C / sqrt(Va Vb): each
 *                 product, quotient, difference and the square root one IEEE operation, n converted exactly.
 *   NaN rule      n < 2, Va or Vb not positive, or a quotient that is not finite (Va Vb underflowed): NaN.  Never an
 *                 infinity -- it would be every row's peak (mtg_wwz's rule).  A NaN half makes r NaN.
 *   mode          MTG_ICCF_BOTH: r = 0.5 (r_A + r_B); MTG_ICCF_COMPANION: r = r_A; MTG_ICCF_RESIDENT: r = r_B.
 *   ccf           [L][K] or NULL: r.   n_a, n_b [L][K] or NULL: the samples of half A and half B; 0 for a half the
 *                 mode does not form.
 *   peak          [L] or NULL: the largest finite ccf[l][k];  peak_index [L] or NULL: the first k attaining it; a row
 *                 without a finite value: NaN and -1.
 *   centroid      [L] or NULL: num / den with num = fma(tau_k, r_k, num) and den = den + r_k over the k, ascending, with
 *                 r_k finite and r_k >= fl(threshold peak); NaN when the row has no finite value or den is not positive.
 *                 timedomain.lag_peak_and_centroid with lag = tau.  Reduced on the device: with ccf, n_a and n_b NULL
 *                 nothing of size L K comes back.
 * Invariance.  Every ccf, n_a, n_b entry depends on (light curve l, its companion row, t2, tau_k, mode) alone, bit for
 * bit: not on L, K, the order of tau, which light curves share a tile, the slabs, L2 == 1 or L2 == L with identical rows,
 * whether the resident sampling is stored shared or per light curve, or which outputs were asked for.  peak[l] and
 * centroid[l] depend on row l of ccf and on tau in the given order.  No floating-point atomics.
 * One lane owns a lag and walks the samples of a half in ascending order; for a fixed lag x does not decrease, so the
 * samples inside the other series' span are one run, found by binary search on the rounded x, and the bracket only moves
 * up: O(N + M) per lag, light curve tile and half.  On shared resident sampling a tile of light curves shares the walk
 * (csrc/mtg_iccf_plan.h); the device copies of the [L][K] outputs stay within 256 MiB: slabs of light curves.
 * mtg_last_solver names "mtg_iccf_kernel<R,per,all> lanes 256" (R light curves per lane; per = 1: a companion row per
 * light curve, taken when L2 == L > 1; all = 0: the kernel that walks half A alone, taken for MTG_ICCF_COMPANION),
 * mtg_last_kernel_ms runs from the pre-pass through the last reduction.
 * Against an exact rational evaluation (the square root at 50 digits) each half is within max(10 rho, 64 sqrt(n) u S) with
 * S = Cabs / sqrt(Va Vb) + |r| (Vaabs / Va + Vbabs / Vb) / 2 what the one-pass formulas' rounding scales with, and the
 * counts are exact (tests/test_iccf_gpu.py).
 * MTG_E_STATE without light curves; MTG_E_ARG for M < 2 or M >= 2^28, N < 2, L2 not 1 or L, K outside
 * 1 .. MTG_ICCF_MAX_LAGS, an unknown mode, a threshold outside (0, 1], all six outputs NULL, a t2 entry that is not finite,
 * t2 descending, a y2 or tau entry that is not finite -- the message names the offending index; the context works as
 * before after an error.
 */
enum { MTG_ICCF_BOTH = 0, MTG_ICCF_COMPANION = 1, MTG_ICCF_RESIDENT = 2, MTG_ICCF_MAX_LAGS = 65536 };
MTG_API int mtg_iccf(mtg_ctx *ctx, int64_t M, const double *t2 /* [M] host, ascending */,
                     int64_t L2 /* 1 or L */, const double *y2 /* [L2][M] host */,
                     int64_t K, const double *tau /* [K] host */, int mode, double threshold,
                     double *ccf /* [L][K] or NULL */, int64_t *n_a /* [L][K] or NULL */, int64_t *n_b /* [L][K] or NULL */,
                     double *peak /* [L] or NULL */, int64_t *peak_index /* [L] or NULL */, double *centroid /* [L] or NULL */);

/*
 * What the periodograms of the resident set say about every frequency: reductions of power[l][k] ACROSS the light
 * curves, without the [L][F] array ever leaving the device.  power[l][k] is, by definition and bit for bit, what
 * mtg_lomb_scargle returns for the same resident set, frequency, normalization and weighting (its launcher computes it).
 *   order_stat[q][k]    the element of rank ranks[q] of column k sorted ascending with NaN last (numpy's sort order);
 *                       ranks at or beyond valid[k] read NaN.  Equal values are one value: -0 and +0 may come in either sign.
 *   valid[k]            #{l : power[l][k] is not NaN}
 *   exceed[k]           #{l : power[l][k] >= reference[k]} (a NaN never counts)
 *   peak_ratio[l]       max_k power[l][k] / scale[k] (the IEEE quotient), NaN entries passed over;
 *   peak_ratio_index[l] the first k attaining it; a row of nothing but NaN: NaN and -1.
 * The frequencies are walked in slabs (at most 64 MiB of device workspace whatever L F is; a column of up to 16384
 * light curves is sorted in LDS, a longer one by a segmented radix sort).  Invariance: every output for column k depends
 * on the resident set as a SET, freqs[k], normalization, weighted and reference[k] / scale[k] alone, bit for bit -- not on
 * F, the order of freqs, the slabs, or (order_stat, valid, exceed) the order of the light curves; peak_ratio[l] depends
 * on light curve l, the frequencies and scale alone.
 * MTG_E_STATE without light curves; MTG_E_ARG for what mtg_lomb_scargle refuses (F < 1, a bad frequency, an unknown
 * normalization, N < 4) and for Q < 0, a rank outside [0, L), Q > 0 with order_stat NULL, exceed without reference, a
 * ratio output without scale, a reference entry that is not finite, a scale entry that is not finite and positive, and
 * a call that asks for no output; the message names the offending index.  The resident set is only read; after an
 * error the context works as before.  mtg_last_solver names "mtg_ls_envelope_column_kernel<C>" (C columns per
 * workgroup) or "mtg_ls_envelope_select_kernel" (segmented sort), or the ratio-peak kernel where nothing else was asked
 * for; mtg_last_kernel_ms runs from the pre-pass to the last slab's kernels.
 */
MTG_API int mtg_lomb_scargle_envelope(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host */, int normalization, int weighted,
                                      int Q, const int64_t *ranks /* [Q] host, each in [0, L), any order, duplicates allowed */,
                                      double *order_stat /* [Q][F] host */,
                                      int64_t *valid /* [F] or NULL */,
                                      const double *reference /* [F] host, finite, or NULL */,
                                      int64_t *exceed /* [F] or NULL, needs reference */,
                                      const double *scale /* [F] host, finite and > 0, or NULL */,
                                      double *peak_ratio /* [L] or NULL, needs scale */,
                                      int64_t *peak_ratio_index /* [L] or NULL, needs scale */);
/*
 * mtg_lomb_scargle_envelope of the periodogram with nterms harmonics: power[l][k] is mtg_lomb_scargle_multi's bit for bit,
 * everything after the powers (slabs, column sort, exceedance, ratio peaks) is mtg_lomb_scargle_envelope's; nterms and N
 * are checked as mtg_lomb_scargle_multi checks them.
 */
MTG_API int mtg_lomb_scargle_envelope_multi(mtg_ctx *ctx, int64_t F, const double *freqs /* [F] host */,
                                            int nterms /* 1 .. MTG_LS_MAX_TERMS */, int normalization, int weighted,
                                            int Q, const int64_t *ranks /* [Q] host */, double *order_stat /* [Q][F] host */,
                                            int64_t *valid /* [F] or NULL */, const double *reference /* [F] host, or NULL */,
                                            int64_t *exceed /* [F] or NULL, needs reference */,
                                            const double *scale /* [F] host, or NULL */,
                                            double *peak_ratio /* [L] or NULL, needs scale */,
                                            int64_t *peak_ratio_index /* [L] or NULL, needs scale */);

/*
 * Accuracy probe of the device elementary functions the recurrence uses
 * (tests only): exp_neg[i] = exp(-x[i]), sin/cos(x[i]), rcp_x[i] = 1 / x[i] for
 * n host values x >= 0.
 */
MTG_API int mtg_math_probe(mtg_ctx *ctx, int64_t n, const double *x, double *exp_neg, double *sin_x,
                           double *cos_x, double *rcp_x);
/* 1 if (jr, jc) has a compiled kernel. */
MTG_API int mtg_structure_supported(int jr, int jc);

#ifdef __cplusplus
}
#endif
#endif /* MTG_H */
