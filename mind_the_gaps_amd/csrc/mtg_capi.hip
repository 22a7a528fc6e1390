// mtg_capi.hip -- host side of the C-ABI declared in include/mtg.h.
// One context = one MI355X + resident light curves + model + workspaces.
#include "mtg_device.h"
#include "mtg_ls_envelope_plan.h"
#include "mtg_mean.h"
#include "mtg_sim_plan.h"
#include "mtg_solve_plan.h"
#include "mtg_tp_scan.h"
#include "mtg_trace.h"

#include <dlfcn.h>
#include <hipfft/hipfft.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <initializer_list>
#include <memory>
#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local std::string g_create_error;

// hipFFT plans are made from helper threads too (mtg_fft_warmup, mtg_simulate_plan) while another thread may be making
// or destroying one for a convergence check: plan creation and destruction go through one process-wide lock
// (executions do not).  FftPlan below is the only code that takes it.
std::mutex g_fft_plan_mu;

// what a 1-D hipFFT plan is made for; idist = odist = 0: hipfftPlan1d, otherwise hipfftPlanMany over contiguous transforms
// that lie idist / odist elements apart
struct FftKey {
    hipfftType type = HIPFFT_Z2Z;
    int64_t len = 0;
    int batch = 0;
    int64_t idist = 0, odist = 0;
    bool operator==(const FftKey &o) const { return type == o.type && len == o.len && batch == o.batch && idist == o.idist && odist == o.odist; }
};

struct FftPlan {  // owning hipFFT plan and the key it was made for; every cached and throw-away plan of the library is one
    FftPlan() = default;
    FftPlan(FftPlan &&o) noexcept : h(o.h), made(o.made), key(o.key) { o.made = false; }
    FftPlan &operator=(FftPlan &&o) noexcept
    {
        if (this != &o) { reset(); h = o.h; made = o.made; key = o.key; o.made = false; }
        return *this;
    }
    ~FftPlan() { reset(); }
    bool holds(const FftKey &k) const { return made && key == k; }
    const FftKey *held() const { return made ? &key : nullptr; }
    // the plan for `k`: the one held if it was made for k, else made now in its place; 0 when hipFFT refuses (nothing is
    // held then).  The caller sets the stream and executes.
    hipfftHandle get(const FftKey &k)
    {
        if (holds(k)) return h;
        std::lock_guard<std::mutex> plans(g_fft_plan_mu);
        drop();
        int len = (int)k.len;
        const hipfftResult r = k.idist ? hipfftPlanMany(&h, 1, &len, nullptr, 1, (int)k.idist, nullptr, 1, (int)k.odist, k.type, k.batch)
                                       : hipfftPlan1d(&h, len, k.type, k.batch);
        if (r != HIPFFT_SUCCESS) return 0;
        made = true;
        key = k;
        return h;
    }
    void reset()
    {
        if (!made) return;
        std::lock_guard<std::mutex> plans(g_fft_plan_mu);
        drop();
    }

private:
    void drop() { if (made) (void)hipfftDestroy(h); made = false; }   // under g_fft_plan_mu
    hipfftHandle h = 0;
    bool made = false;
    FftKey key;
};

// A forward / inverse pair (convergence check, E13 adjustment) is two plans, both made or neither: 0, or which creation
// failed (1 forward, 2 inverse) with both plans empty.
int fft_pair_get(FftPlan &fwd, const FftKey &kf, FftPlan &inv, const FftKey &ki, hipfftHandle *hf, hipfftHandle *hi)
{
    *hf = fwd.get(kf);
    *hi = *hf ? inv.get(ki) : 0;
    if (*hf && *hi) return 0;
    fwd.reset();
    inv.reset();
    return *hf ? 2 : 1;
}

struct DevBuf {  // owning device allocation; locals free themselves on every return path
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 4;  // grow with slack: batches vary between calls
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    template <class T> hipError_t reserve_n(int64_t n) { return reserve((size_t)n * sizeof(T)); }   // room for n elements
    template <class T> T *as() const { return static_cast<T *>(p); }
};

}  // namespace

struct mtg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    std::string err;

    // light curves (resident)
    int64_t N = 0, L = 0;
    int t_per_lc = 0;
    uint64_t window_bytes = 0xffffffffull;  // reach of one buffer descriptor of the sweep (mtg_set_window_bytes)
    DevBuf dxt, yv, dxmax;  // interleaved (dx, t) and (y, sigma^2) pairs
    DevBuf t_tmp, y_tmp, dy_tmp, off_tmp;  // upload staging

    // model
    bool has_model = false;
    MtgModel model;

    // workspaces
    DevBuf coef, lists, counts, tp_ws, sig;
    DevBuf tables;            // resident exp2 / (cos, sin) tables for the time-parallel kernels (mtg_launch_tables)
    bool tables_ready = false;
    int64_t cstride = 0;
    int nsig_ws = 1;  // signature lists the workspace was laid out for
    int bank = 0;     // which of the two banks of structure lists / counters the next expansion and solve use (the device
                      // sampler alternates: the proposals of a half-step are expanded while the other bank is cleared)
    // staging for the host-pointer entry points
    DevBuf theta, lc, out, status;
    DevBuf grad_dcoef, grad, grad_verdict;  // mtg_loglike_grad: coefficient tangents [nslots][B P], the gradient [B][P], the expansion's status [B]; grown on demand
    // mtg_whiten: one slab of given data, residuals, their sorted copy and lag sums, the sort's scratch; [B][8] sums; grown on demand
    DevBuf whiten_y, whiten_q, whiten_sorted, whiten_acf, whiten_temp, whiten_stats;

    // small batches: one wave per evaluation, parallel in time (0 never, 1 whenever compiled, 2 auto)
    int tp_mode = 2;   // (3: as 1, but the one-wave-per-evaluation kernel only -- results independent of the batch size)
    int tp_direct = 1;  // rank-10 time-parallel path: likelihood without the filter pass (mtg_set_tp_direct)
    int pipe_mode = 2;  // two-wave pipeline of the serial sweep (mtg_set_pipeline): 0 never, 1 whenever compiled, 2 auto
    int cus = 0;        // compute units of the device

    int64_t stream_base = 0;      // mtg_set_stream_base: global index of the context's first ensemble / simulated series
    // device-resident ensembles (mtg_ensemble_*)
    struct Ensembles {
        int64_t E = 0, L = 0, N = 0;  // ensembles; shape of the resident set they index into
        int W = 0, P = 0;
        uint64_t seed = 0;
        int64_t base = 0;             // stream_base as it was when the ensembles were made
        uint32_t iteration = 0;
        DevBuf coords, lnp, perm, naccept, best_lnp, best_coords, notpd;   // the state: [E][W][P], [E][W] ..., one counter
        // the rows of a solve -- proposals, their factors, log-probabilities, statuses, light curves --: room for the
        // 3 E W/2 of a speculative iteration, a half-step uses the first E W/2; lc_full: the light curve of every walker
        DevBuf q, factor, new_lnp, st, lc_spec, lc_full;
        DevBuf chain, lnp_chain;      // a run's [steps][E][W][P] and [steps][E][W]
        DevBuf perm_all;              // the splits of a whole speculative run, made before it ([steps][E][W])
        // the bytes each buffer holds for E ensembles of W walkers in P dimensions
        struct Sizes { size_t coords, lnp, perm, naccept, best_lnp, best_coords, notpd, q, factor, new_lnp, st, lc_spec, lc_full; };
        static Sizes sizes(int64_t E, int W, int P)
        {
            const size_t EW = (size_t)E * W, EH = (size_t)E * (W / 2), d = sizeof(double), i = sizeof(int32_t);
            Sizes z;
            z.coords = EW * P * d; z.lnp = EW * d; z.best_lnp = (size_t)E * d; z.best_coords = (size_t)E * P * d;
            z.perm = z.naccept = z.lc_full = EW * i; z.notpd = i;
            z.q = 3 * EH * P * d; z.factor = 2 * EH * d; z.new_lnp = 3 * EH * d; z.st = z.lc_spec = 3 * EH * i;
            return z;
        }
        Sizes sizes() const { return sizes(E, W, P); }
        hipError_t reserve(const Sizes &z)
        {
            const struct { DevBuf &buf; size_t bytes; } rooms[] = {
                {coords, z.coords}, {lnp, z.lnp}, {perm, z.perm}, {q, z.q}, {factor, z.factor}, {new_lnp, z.new_lnp}, {st, z.st},
                {lc_spec, z.lc_spec}, {lc_full, z.lc_full}, {naccept, z.naccept}, {best_lnp, z.best_lnp},
                {best_coords, z.best_coords}, {notpd, z.notpd}};
            hipError_t e = hipSuccess;
            for (const auto &r : rooms) e = e == hipSuccess ? r.buf.reserve(r.bytes) : e;
            return e;
        }

        // walker sharding (mtg_ensemble_shard_*): this rank evaluates rows [lo, hi) of every half-step's proposals; the
        // exchange brings everybody's log-probabilities before the accept step.  What shard_release resets; the generation
        // counter and the profile's events after it stay
        struct Shard {
            int kind = 0;  // 0 none, 1 RCCL all-gather on the stream, 2 host callback
            int rank = 0, world = 1;
            int64_t chunk = 0, lo = 0, hi = 0;
            void *comm = nullptr;         // ncclComm_t
            mtg_exchange_fn fn = nullptr;
            void *user = nullptr;
            double *h_lnp = nullptr;      // pinned staging of the host exchange: h_rows rows
            int32_t *h_st = nullptr;
            int64_t h_rows = 0;
        } shard;
        std::atomic<int> shard_generation{0};   // bumped by every (un)sharding: a communicator that comes up late is dropped
        std::vector<hipEvent_t> shard_ev;       // mtg_ensemble_shard_profile: event pairs around the first exchanges of a run
        int shard_ev_cap = 0, shard_ev_n = 0;
    } ens;
    int64_t live_rows = 0;              // rows the next solve really evaluates (0: all) -- kernel choice only
    bool no_prior_batch = false;        // the batch being solved was expanded WITHOUT the prior (run_model_batch): kernel choice only

    // mtg_chain_autocorr: the convergence check is repeated on a growing chain, so plans and buffers stay.  Four plan
    // pairs, the least recently used one making room: the tutorial's loop checks the null and the alternative model's
    // chains in turn (two shapes), and a single slot was rebuilt at every check -- 9 ms each, a third of that loop
    // (scripts/tutorial_loop_probe.py)
    struct AcfPlans { FftPlan fwd, inv; uint64_t used = 0; } acf_slots[MTG_ACF_SLOTS];   // (slot choice: mtg_sim_plan.h)
    uint64_t acf_clock = 0;
    DevBuf acf_chain, acf_x, acf_f, acf_g, acf_r, acf_ss, acf_tmp;
    int64_t acf_plans_built = 0;   // plan pairs made so far (mtg_chain_autocorr_plans_built: a cached shape must not add to it)

    // mtg_simulate_tk95: the inverse transform's plan (made once per length: a Bluestein plan for the 1 087 853 points
    // of BASELINE configs[3] takes 0.9 s to build, as long as the 2000 simulations it then runs) and its buffers.
    // mtg_simulate_plan may build it from a helper thread while the context is busy elsewhere: sim_mu.
    std::mutex sim_mu;
    // C2R plans of the simulator: [0] the bulk plan (the batch of a full call at the length), [1] a short call's (fewer
    // series than that batch: a single light curve runs ONE transform); each remade when its (length, batch) changes.
    // Which slot a call takes: MtgSimLayout::slot (mtg_sim_plan.h)
    FftPlan sim_plans[2];
    DevBuf sim_spec, sim_series;
    // ... and the hand-made chirp-z transform for lengths hipFFT would take through a Bluestein plan (0.9 s to build
    // against 15 ms for the power-of-two plans this needs; mtg_simulate.hip): chirp w [nfft], transform of the wrapped
    // conjugate chirp [m], work area [pairs][m], Z2Z plans of length m ([0] the bulk batch, [1] a short call's)
    struct SimCzt {
        bool tables = false;
        bool pairs_on = true;   // two series per complex transform (mtg_set_simulate_pairs)
        int64_t nfft = 0, m = 0;
        DevBuf chirp, bhat, work;
        FftPlan plans[2];
    } czt;
    // draws handed in by the caller for the NEXT mtg_simulate_tk95 (mtg_set_simulate_draws): standard normals
    // [S][2][nfft / 2 + 1] and segment starts [S]
    struct { DevBuf normals, starts; std::vector<int64_t> starts_host; int64_t S = 0, nk = 0; } given;
    // KraftNoise for noise_kind 3 (mtg_set_simulate_kraft): per-epoch background and the faint epochs' tables
    struct { DevBuf bkg, err, med, half; int K = 0; double threshold = 0.0; int64_t N = 0; } kraft;
    // the flux PDF of the simulated light curves (mtg_set_simulate_pdf): 0 Gaussian = TK95 as it is, 1 lognormal, 2 uniform
    // = the E13 adjustment of every cut segment on the device (mtg_e13.hip); its buffers, plans and last run's report
    struct E13 {
        int kind = 0, max_iter = 400;
        DevBuf seg, x, fresh, values, adj, keys, amp, spec, idx, order, order_tmp, segment, segment_out, flags, stdv, temp;
        FftPlan fwd, inv;   // D2Z / Z2D over [batch][n], remade together when n or the batch changes
        // the scratch of one chunk, all of it (what the simulator's epilogue weighs and releases; not `given`)
        template <class F> void each_scratch(F f)
        {
            for (DevBuf *b : {&seg, &x, &fresh, &values, &adj, &keys, &amp, &spec, &idx, &order, &order_tmp, &segment, &segment_out,
                              &flags, &stdv, &temp})
                f(*b);
        }
        int64_t not_converged = 0;
        int iterations = 0;
        DevBuf given;            // caller's draws for the next simulation (mtg_set_simulate_pdf_draws): [S][n]
        int64_t given_S = 0, given_n = 0;
    } e13;

    // side streams: the structures (signatures) of a small batch run next to each other
    hipStream_t side[MTG_MAX_J / 2] = {};
    hipEvent_t side_done[MTG_MAX_J / 2] = {};
    hipEvent_t fork = nullptr;

    // per-call kernel timing (mtg_profile_*): event triples start / solve / end
    std::vector<hipEvent_t> prof_ev;
    int prof_cap = 0, prof_n = 0;

    // order of the serial sweep (mtg_sort.hip): 0 the caller's order, 1 always sorted by (structure, light curve),
    // 2 sorted unless the caller's order is known to be grouped already (host entry points look at lc_index)
    int sort_mode = 2;
    int spec_mode = 1;                  // speculative iterations of small ensembles: 0 never, 1 where they pay, 2 = 1 without the splits up front (mtg_ensemble_run)
    int lc_grouped_hint = 0;   // set by the host-pointer entry points for the call in flight
    DevBuf sort_keys, sort_keys_out, sort_order, sort_tmp;
    char last_solver[96] = "";   // what the last solve dispatched (mtg_last_solver)

    // Calls may come on the caller's streams (mtg_loglike_batch_device) and on the context's own; they share the
    // workspaces, so consecutive calls on different streams are chained with events: every call on a foreign
    // stream ends by recording `foreign_done` on it, every call begins by waiting for whatever ran last elsewhere.
    hipEvent_t foreign_done = nullptr, own_done = nullptr;
    bool foreign_pending = false;   // work recorded in foreign_done that the context's stream has not waited for
    bool own_dirty = false;         // the context's stream has had work since the last foreign call waited for it
    hipStream_t last_foreign = nullptr;

    // mtg_pair_contexts: the partner whose pipelined half-steps share a launch with this context's (MtgPair below)
    // Shared ownership: a thread inside pair_launch holds a reference of its own, so that mtg_unpair_contexts /
    // mtg_destroy on the partner's thread cannot free the rendezvous under it.  Read and written with
    // std::atomic_load / std::atomic_store only.
    std::shared_ptr<struct MtgPair> pair;

    // mtg_set_simulate_transform: 0 = by grid length (default), 1 = hipFFT's own plan, 2 = chirp-z
    int sim_transform = 0;

    // every hipFFT plan of the context (mtg_destroy: before the stream they run on goes)
    void reset_plans()
    {
        for (AcfPlans &sl : acf_slots) { sl.fwd.reset(); sl.inv.reset(); }
        for (FftPlan *pl : {&sim_plans[0], &sim_plans[1], &czt.plans[0], &czt.plans[1], &e13.fwd, &e13.inv}) pl->reset();
    }
};

// Two contexts whose pipelined sweeps go out in ONE launch (mtg_kernels_pipe_pair.hip): the two models of the Protassov
// test, each driven by a host thread of its own (mtg_ensemble_run: a loop of asynchronous launches).  Whoever reaches
// a pipelined half-step first leaves its arguments here, records `ready` on its stream and waits -- on the HOST, for as
// long as the partner takes to get to its own half-step, microseconds in steady state --; the second one makes its
// stream wait for `ready`, launches both models' rows in one grid, records `done`, and the first one's stream waits
// for that.  Nothing waits without a bound: a partner that does not come within `patience_ms` (stalled between two C
// calls, its run over, its batch on another kernel) means "alone this time"; MTG_PAIR_MAX_MISSES consecutive misses
// (each waited for half as long as the one before) break the pair for good and everybody launches alone from then on.
enum { MTG_PAIR_MAX_MISSES = 4 };
struct MtgPair {
    ~MtgPair()
    {
        for (hipEvent_t e : {ready[0], ready[1], done})
            if (e) (void)hipEventDestroy(e);
    }
    std::mutex mu;
    std::condition_variable cv;
    mtg_ctx *members[2] = {nullptr, nullptr};
    hipEvent_t ready[2] = {nullptr, nullptr}, done = nullptr;
    bool waiting = false;     // the slot holds a half-step
    int who = 0;              // ... of this member
    MtgSolveArgs sa;
    int64_t rows = 0;
    MtgPipeShapeId shape{};
    uint64_t launched = 0;    // pair launches so far (a waiter leaves when it moves)
    bool broken = false;
    int patience_ms = 250;
    int misses = 0;           // consecutive half-steps whose partner did not come
    int64_t n_pair = 0, n_solo = 0;
};

namespace {

// the current bank of structure lists ([nsig] signature lists, then [nsig] left-over lists) and counters (64)
inline int *bank_lists(const mtg_ctx *ctx) { return ctx->lists.as<int>() + (int64_t)ctx->bank * 2 * ctx->nsig_ws * ctx->cstride; }
inline int *bank_counts(const mtg_ctx *ctx) { return ctx->counts.as<int>() + ctx->bank * 64; }

void shard_release(mtg_ctx *ctx);

int fail(mtg_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail((ctx), MTG_E_HIP, "%s failed: %s", #call, hipGetErrorString(e__));   \
    } while (0)

int nparams(int kind)
{
    switch (kind) {
    case MTG_TERM_REAL: return 2;
    case MTG_TERM_COMPLEX3: return 3;
    case MTG_TERM_COMPLEX4: return 4;
    case MTG_TERM_SHO: return 3;
    case MTG_TERM_MATERN32: return 2;
    case MTG_TERM_JITTER: return 1;
    case MTG_TERM_DRW: return 2;
    case MTG_TERM_LORENTZIAN: return 3;
    case MTG_TERM_COSINUS: return 2;
    case MTG_TERM_BPL: return 3;
    default: return -1;
    }
}

int use_device(mtg_ctx *ctx)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return MTG_OK;
}

// Begin a call that launches on stream `s`: wait for what the previous calls left running on other streams.
int enter_stream(mtg_ctx *ctx, hipStream_t s)
{
    if (s == ctx->stream) {
        if (ctx->foreign_pending) {
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->foreign_done, 0));
            ctx->foreign_pending = false;
        }
        ctx->own_dirty = true;
        return MTG_OK;
    }
    if (ctx->own_dirty) {
        HIP_TRY(ctx, hipEventRecord(ctx->own_done, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->own_done, 0));
        ctx->own_dirty = false;
    }
    if (ctx->foreign_pending && ctx->last_foreign != s) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->foreign_done, 0));
    return MTG_OK;
}

// End of a call on a foreign stream: later calls (and mtg_synchronize) wait for this point.
int leave_stream(mtg_ctx *ctx, hipStream_t s)
{
    if (s == ctx->stream) return MTG_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->foreign_done, s));
    ctx->foreign_pending = true;
    ctx->last_foreign = s;
    return MTG_OK;
}

// the context's own stream, ordered after whatever ran last on a caller's stream
#define CTX_STREAM(ctx, s)                         \
    hipStream_t s = (ctx)->stream;                 \
    do {                                           \
        int rc__ = enter_stream((ctx), s);         \
        if (rc__) return rc__;                     \
    } while (0)

int reserve_workspace(mtg_ctx *ctx, int64_t B, int nslots, int nsig)
{
    // stride padded to a multiple of 64 so that every column starts 512-B aligned
    int64_t stride = (B + 63) / 64 * 64;
    if (stride < 64) stride = 64;
    HIP_TRY(ctx, ctx->coef.reserve((size_t)stride * nslots * sizeof(double)));
    // [nsig] signature lists, then [nsig] left-over lists of the windowed sweep (sweep_launch)
    HIP_TRY(ctx, ctx->lists.reserve((size_t)stride * (nsig > 1 ? nsig : 1) * 2 * 2 * sizeof(int)));   // two banks
    ctx->nsig_ws = nsig > 1 ? nsig : 1;
    HIP_TRY(ctx, ctx->counts.reserve(2 * 64 * sizeof(int)));
    HIP_TRY(ctx, ctx->sig.reserve((size_t)stride * sizeof(int32_t)));
    ctx->cstride = stride;
    return MTG_OK;
}

// coefficient slots of a row of model m: the layout's, and a profile mean's further constants behind them (mtg_mean.h)
int model_nslots(const MtgModel &m)
{
    return MtgCoefLayout{m.nr_max, m.nc_max}.nslots() + mtg_mean_extra_slots(m.mean_kind);
}

// the sweep of structure (nr, nc) for a model's mean kind
mtg_solve_launcher find_sweep(int mean_kind, int nr, int nc, int last_b0 = 0)
{
    return mtg_mean_is_profile(mean_kind) ? mtg_find_mean_solver(mean_kind, nr, nc, last_b0) : mtg_find_solver(nr, nc, last_b0);
}

// the entries that read the mean on the device (predict, draw, gradient) know the constant and the linear mean only
int refuse_profile_mean(mtg_ctx *ctx, const char *who)
{
    const int kind = ctx->model.mean_kind;
    if (!mtg_mean_is_profile(kind)) return MTG_OK;
    return fail(ctx, MTG_E_UNSUPPORTED, "%s: not available with mean kind %d (%s): bind y - mean(t) with a zero mean instead", who,
                kind, mtg_mean_name(kind));
}

// every structure of the model (nr0 + 2k, nc0 - k) must have a compiled kernel; reserves the
// coefficient workspace for B evaluations
int check_model_workspace(mtg_ctx *ctx, int64_t B)
{
    const MtgModel &m = ctx->model;
    const int nsig = m.nsho + 1;
    for (int k = 0; k < nsig; ++k) {
        const int nr = m.nr0 + 2 * k, nc = m.nc0 - k;
        if (nr + nc == 0) continue;
        if (!mtg_find_solver(nr, nc))
            return fail(ctx, MTG_E_UNSUPPORTED,
                        "no compiled kernel for %d real + %d complex terms (J=%d)", nr, nc,
                        nr + 2 * nc);
    }
    return reserve_workspace(ctx, B, model_nslots(m), nsig);
}

// arguments of the theta -> coefficients expansion into the context's workspace; nsig: structure lists to fill
// (the model's nsho + 1 for the likelihood's solvers; 1 = none: the per-row entries and the simulator, which read the
// structure of a row from ctx->sig and, like everybody but mtg_ensemble_run, find the context on bank 0)
MtgPrepArgs make_prep_args(mtg_ctx *ctx, int64_t B, const double *d_theta, int add_prior, double *d_out,
                           int32_t *d_status, int nsig)
{
    MtgPrepArgs pa;
    pa.model = ctx->model;
    pa.theta = d_theta;
    pa.B = B;
    pa.add_prior = add_prior;
    pa.coef = ctx->coef.as<double>();
    pa.cstride = ctx->cstride;
    pa.nsig = nsig;
    pa.lists = bank_lists(ctx);
    pa.counts = bank_counts(ctx);
    pa.out = d_out;
    pa.status = d_status;
    pa.sig = ctx->sig.as<int32_t>();  // structure of every evaluation: the rank-10 time-parallel path dispatches on it
    pa.row_lo = 0;
    pa.row_hi = INT64_MAX;
    return pa;
}

int check_lc_index(mtg_ctx *ctx, int64_t B, const int32_t *lc_index)
{
    if (lc_index)
        for (int64_t b = 0; b < B; ++b)
            if (lc_index[b] < 0 || lc_index[b] >= ctx->L)
                return fail(ctx, MTG_E_ARG, "lc_index[%lld] = %d outside [0, %lld)", (long long)b, lc_index[b],
                            (long long)ctx->L);
    return MTG_OK;
}

// fn(row0, rows) for the slabs [row0, row0 + rows) of a batch of B rows, Bs at a time, until one fails
template <class F>
hipError_t for_each_slab(int64_t B, int64_t Bs, F fn)
{
    hipError_t e = hipSuccess;
    for (int64_t row0 = 0; e == hipSuccess && row0 < B; row0 += Bs) e = fn(row0, B - row0 < Bs ? B - row0 : Bs);
    return e;
}

// One launch of the serial sweep for structure k of the model.  When the resident set is larger than
// the reach of a buffer descriptor the kernel leaves the evaluations a wave cannot reach from its
// first light curve on a list; a second launch sweeps them one per wave (its workgroups find the
// list empty and leave at once when batches are grouped by light curve, the usual case).
int sweep_launch(mtg_ctx *ctx, mtg_solve_launcher fn, MtgSolveArgs sa, int64_t B, int k, hipStream_t s)
{
    sa.solo = 0;
    sa.left_list = nullptr;
    sa.left_count = nullptr;
    if (sa.yv_bytes <= sa.window_bytes) {
        fn(sa, B, s);
        return MTG_OK;
    }
    int *left_list = bank_lists(ctx) + ((int64_t)ctx->nsig_ws + k) * ctx->cstride;
    int *left_count = bank_counts(ctx) + 32 + k;
    HIP_TRY(ctx, hipMemsetAsync(left_count, 0, sizeof(int), s));
    sa.left_list = left_list;
    sa.left_count = left_count;
    fn(sa, B, s);
    sa.solo = 1;
    sa.list = left_list;
    sa.count_ptr = left_count;
    sa.seg_counts = nullptr;  // (the left-over list starts at 0, whatever segment of a sorted order it came from)
    sa.seg_k = 0;
    sa.left_list = nullptr;
    sa.left_count = nullptr;
    fn(sa, B * 64, s);  // one wave per left-over evaluation
    return MTG_OK;
}

int solve_prepared(mtg_ctx *ctx, int64_t B, const int32_t *d_lc, double *d_out, int32_t *d_status, hipStream_t s,
                   bool may_sort = false);

// theta -> coefficients -> solver(s) for B evaluations; timing events around the launches
int run_model_batch(mtg_ctx *ctx, int64_t B, const double *d_theta, const int32_t *d_lc,
                    int add_prior, double *d_out, int32_t *d_status, hipStream_t s)
{
    int rc = check_model_workspace(ctx, B);
    if (rc) return rc;
    const int nsig = ctx->model.nsho + 1;
    const bool prof = ctx->prof_n < ctx->prof_cap;
    hipEvent_t *pe = prof ? &ctx->prof_ev[3 * (size_t)ctx->prof_n] : nullptr;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, s));
    if (prof) HIP_TRY(ctx, hipEventRecord(pe[0], s));
    {
        mtg_trace::Range range("mtg:prepare (theta -> prior, coefficients)");
        if (nsig > 1) HIP_TRY(ctx, hipMemsetAsync(bank_counts(ctx), 0, 64 * sizeof(int), s));
        mtg_launch_prepare(make_prep_args(ctx, B, d_theta, add_prior, d_out, d_status, nsig), s);
    }
    if (prof) HIP_TRY(ctx, hipEventRecord(pe[1], s));
    {
        mtg_trace::Range range("mtg:solve (factorisation + forward solve)");
        ctx->no_prior_batch = !add_prior;
        rc = solve_prepared(ctx, B, d_lc, d_out, d_status, s, true);
        ctx->no_prior_batch = false;
    }
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
    if (prof) {
        HIP_TRY(ctx, hipEventRecord(pe[2], s));
        ctx->prof_n += 1;
    }
    ctx->timed = true;
    return MTG_OK;
}

// A pipelined half-step of a paired context (MtgPair): *paired = 1 when its rows went out -- or will go out, ordered
// before anything that follows on `s` -- in a launch shared with the partner's; 0: the caller launches alone.
int pair_launch(mtg_ctx *ctx, const MtgSolveArgs &sa, int64_t B, const MtgPipeShapeId &shape, hipStream_t s, int *paired)
{
    *paired = 0;
    const std::shared_ptr<MtgPair> p = std::atomic_load(&ctx->pair);   // ours for the whole call, whatever the partner does
    if (!p) return MTG_OK;
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->broken) { p->n_solo += 1; return MTG_OK; }
    const int me = p->members[0] == ctx ? 0 : 1;
    if (!p->waiting) {
        HIP_TRY(ctx, hipEventRecord(p->ready[me], s));
        p->sa = sa; p->rows = B; p->shape = shape; p->who = me; p->waiting = true;
        const uint64_t seen = p->launched;
        const int patience = std::max(1, p->patience_ms >> std::min(p->misses, 8));
        p->cv.wait_for(lk, std::chrono::milliseconds(patience), [&] { return p->launched != seen || p->broken; });
        if (p->launched != seen) {   // the partner launched both
            p->misses = 0;
            HIP_TRY(ctx, hipStreamWaitEvent(s, p->done, 0));
            *paired = 1;
            return MTG_OK;
        }
        p->waiting = false;          // nobody came: alone this time; for good after a few misses in a row
        p->misses += 1;
        if (p->misses >= MTG_PAIR_MAX_MISSES) p->broken = true;
        p->n_solo += 1;
        return MTG_OK;
    }
    // the partner's half-step is waiting: both in one launch, on this stream
    const MtgSolveArgs &other = p->sa;
    mtg_pipe_pair_launcher fn = nullptr;
    bool mine_first = false;
    if (other.N == sa.N && p->who != me) {
        // (member 0's model first, as the pairs are listed: null, alternative; then the other way round)
        const bool other_is_0 = p->who == 0;
        fn = other_is_0 ? mtg_find_pipe_pair_solver(p->shape, shape) : mtg_find_pipe_pair_solver(shape, p->shape);
        mine_first = !other_is_0;
        if (!fn) {
            fn = other_is_0 ? mtg_find_pipe_pair_solver(shape, p->shape) : mtg_find_pipe_pair_solver(p->shape, shape);
            mine_first = other_is_0;
        }
    }
    if (!fn) {   // different samplings, or a pair of shapes that is not compiled: both go alone from now on
        p->broken = true;
        p->n_solo += 1;
        lk.unlock();
        p->cv.notify_all();
        return MTG_OK;
    }
    if (hipStreamWaitEvent(s, p->ready[p->who], 0) != hipSuccess) {   // nothing launched: the waiter goes alone
        p->broken = true;
        p->n_solo += 1;
        lk.unlock();
        p->cv.notify_all();
        return fail(ctx, MTG_E_HIP, "pair_launch: hipStreamWaitEvent failed");
    }
    if (mine_first) fn(sa, B, other, p->rows, s);
    else fn(other, p->rows, sa, B, s);
    // The partner's rows ARE in flight from here on: whatever happens next, its wait must end with "launched" (a waiter
    // that timed out would launch them a second time), and `done` is what its stream orders itself behind.
    const hipError_t recorded = hipEventRecord(p->done, s);
    p->waiting = false;
    p->launched += 1;
    p->n_pair += 1;
    p->misses = 0;
    *paired = 1;
    if (recorded != hipSuccess) p->broken = true;
    lk.unlock();
    p->cv.notify_all();
    if (recorded != hipSuccess) return fail(ctx, MTG_E_HIP, "pair_launch: hipEventRecord(done) failed: %s", hipGetErrorString(recorded));
    return MTG_OK;
}

// What every solver launch of B evaluations takes from the context alone: the coefficient columns, the resident light
// curves and the window over them, the context's tables (made at the first call).
int solve_args_context(mtg_ctx *ctx, int64_t B, const int32_t *d_lc, double *d_out, int32_t *d_status, hipStream_t s, MtgSolveArgs &sa)
{
    sa.coef = ctx->coef.as<double>();
    sa.cstride = ctx->cstride;
    sa.B = B;
    sa.lc_index = d_lc;
    sa.status = d_status;
    sa.out = d_out;
    sa.dxt = ctx->dxt.as<double2>();
    sa.yv = ctx->yv.as<double2>();
    sa.N = ctx->N;
    sa.t_stride = ctx->t_per_lc ? ctx->N : 0;
    sa.dxmax = ctx->dxmax.as<double>();
    sa.yv_bytes = (uint64_t)ctx->L * (uint64_t)ctx->N * 16u;
    sa.dxt_bytes = (uint64_t)(ctx->t_per_lc ? ctx->L : 1) * (uint64_t)ctx->N * 16u;
    sa.window_bytes = ctx->window_bytes;
    if (!ctx->tables_ready) {   // once per context, on the stream of its first batch (every later one is ordered behind it)
        HIP_TRY(ctx, ctx->tables.reserve(mtg_tables_bytes()));
        mtg_launch_tables(ctx->tables.p, s);
        HIP_TRY(ctx, hipGetLastError());
        ctx->tables_ready = true;
    }
    sa.tables = ctx->tables.p;
    if (const char *env = mtg_measure_env("MTG_GLOBAL_TABLES"))   // MTG_MEASURE builds only: 0 = every workgroup computes its own
        if (atoi(env) == 0) sa.tables = nullptr;
    return MTG_OK;
}

// ... and from the model whose expansion filled the columns (mtg_loglike_coeffs, which has none, says these itself)
void solve_args_model(const MtgModel &m, MtgSolveArgs &sa)
{
    sa.lay = MtgCoefLayout{m.nr_max, m.nc_max};
    sa.mean_kind = m.mean_kind;
    // the mean vanishes identically when it is a frozen constant equal to 0 (the
    // per-light-curve frozen mean lives in y_offset)
    sa.has_mean = !(m.mean_kind == MTG_MEAN_CONSTANT && m.src[m.nk] < 0 && m.defaults[m.nk] == 0.0);
    for (int i = 0; i < m.nterms; ++i)
        if (m.kinds[i] == MTG_TERM_JITTER) sa.has_mean = 1;  // the plain sweep variant also skips the jitter add
}

// an MTG_MEASURE knob's value (shipped builds, or the variable not set: `unset`)
long measure_knob(const char *name, long unset)
{
    const char *v = mtg_measure_env(name);
    return v ? atol(v) : unset;
}

// the compiled shapes, as the planner asks for them
const MtgCatalogue g_catalogue = {
    [](int nr, int nc, int b0) { return mtg_find_solver(nr, nc, b0) != nullptr; },
    mtg_solver_uses_b0,
    [](int nr, int nc) { return mtg_find_tp_solver(nr, nc) != nullptr; },
    [](int nr, int nc) { return mtg_find_tp_wide_solver(nr, nc) != nullptr; },
    [](int nr0, int nc0, int nsig, int lanes) { return mtg_find_tp_fused_solver(nr0, nc0, nsig, lanes) != nullptr; },
    [](int nr0, int nc0, int nsig, int b0) { return mtg_find_pipe_solver(nr0, nc0, nsig, b0) != nullptr; },
    [](int nr0, int nc0, int nsig, int b0) { return mtg_find_multi_solver(nr0, nc0, nsig, b0) != nullptr; },
};

// what the planner sees of B prepared evaluations (may_sort: see solve_prepared)
MtgPlanIn plan_input(const mtg_ctx *ctx, int64_t B, bool may_sort, const MtgSolveArgs &sa)
{
    const MtgModel &m = ctx->model;
    MtgPlanIn in;
    in.N = ctx->N; in.B = B; in.L = ctx->L;
    in.Bw = ctx->live_rows > 0 ? ctx->live_rows : B;
    in.nr0 = m.nr0; in.nc0 = m.nc0; in.nsig = m.nsho + 1; in.last_b0 = m.last_b0;
    in.tp_mode = ctx->tp_mode; in.pipe_mode = ctx->pipe_mode; in.sort_mode = ctx->sort_mode;
    in.may_sort = may_sort;
    in.lc_grouped_hint = ctx->lc_grouped_hint != 0;
    in.no_prior_batch = ctx->no_prior_batch;
    for (int i = 0; i < m.nterms; ++i) in.free_b = in.free_b || m.kinds[i] == MTG_TERM_COMPLEX4 || m.kinds[i] == MTG_TERM_BPL;
    in.in_window = sa.yv_bytes <= sa.window_bytes;
    in.cus = ctx->cus;
    in.profile_mean = mtg_mean_is_profile(m.mean_kind);
    in.sweep_multi = measure_knob("MTG_SWEEP_MULTI", 1) != 0;
    in.sweep_fan_out = measure_knob("MTG_SWEEP_FANOUT", 1) != 0;
    in.tp_gsize = (int)measure_knob("MTG_TP_GSIZE", 0);
    in.tp_chunk_target = measure_knob("MTG_TP_CHUNK_TARGET", 0);
    return in;
}

// The structures of an MTG_SOLVE_STRUCTURES plan, each on the stream the plan gives it, joined on `s`.  The side
// streams first: their (usually few) waves are resident before the common structure's launch fills every slot its
// registers allow (J = 6: two waves of 204 VGPRs leave no room for a third of 166).
int launch_structures(mtg_ctx *ctx, const MtgSolvePlan &plan, MtgSolveArgs &sa, const int *sorted, int64_t B, hipStream_t s)
{
    const MtgModel &m = ctx->model;
    const int nsig = m.nsho + 1;
    if (plan.fan_out) {
        if (!ctx->fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming));
        int prio_low = 0, prio_high = 0;
        HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        for (int k = 0; k + 1 < nsig; ++k) {
            // (above the caller's stream: the few rows of a rare structure should not queue behind the common one)
            if (!ctx->side[k]) HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->side[k], hipStreamNonBlocking, prio_high));
            if (!ctx->side_done[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->side_done[k], hipEventDisableTiming));
        }
        HIP_TRY(ctx, hipEventRecord(ctx->fork, s));
    }
    for (int kk = 0; kk < nsig; ++kk) {
        const int k = plan.fan_out ? nsig - 1 - kk : kk;
        const int nr = m.nr0 + 2 * k, nc = m.nc0 - k;
        if (plan.kernel[k] == MTG_STRUCT_NONE) continue;
        sa.list = nsig > 1 ? bank_lists(ctx) + (int64_t)k * ctx->cstride : nullptr;
        sa.count_ptr = nsig > 1 ? bank_counts(ctx) + k : nullptr;
        sa.seg_counts = nullptr; sa.seg_k = 0;
        if (sorted && plan.kernel[k] == MTG_STRUCT_SWEEP) {  // the k-th segment of the sorted order
            sa.list = sorted;
            sa.seg_counts = nsig > 1 ? bank_counts(ctx) : nullptr;
            sa.seg_k = k;
        }
        const hipStream_t sk = plan.side[k] < 0 ? s : ctx->side[plan.side[k]];
        if (sk != s) HIP_TRY(ctx, hipStreamWaitEvent(sk, ctx->fork, 0));
        if (plan.kernel[k] == MTG_STRUCT_SWEEP) {
            const int rc = sweep_launch(ctx, find_sweep(m.mean_kind, nr, nc, m.last_b0), sa, B, k, sk);
            if (rc) return rc;
        } else {
            sa.solo = 0; sa.left_list = nullptr; sa.left_count = nullptr;
            (plan.kernel[k] == MTG_STRUCT_TP_WIDE ? mtg_find_tp_wide_solver(nr, nc) : mtg_find_tp_solver(nr, nc))(sa, B, sk);
        }
        if (sk != s) HIP_TRY(ctx, hipEventRecord(ctx->side_done[plan.side[k]], sk));
    }
    for (int k = 1; k < nsig; ++k)
        if (plan.side[k] >= 0 && plan.kernel[k] != MTG_STRUCT_NONE) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->side_done[plan.side[k]], 0));
    return MTG_OK;
}

// Launch the solver(s) for B prepared evaluations living in ctx->coef (lists / counts filled), as mtg_plan_solve
// (mtg_solve_plan.h) decides.  may_sort: the caller's order is arbitrary (mtg_loglike_batch[_device]); the device
// sampler's batches are grouped by ensemble, hence by light curve, by construction.
int solve_prepared(mtg_ctx *ctx, int64_t B, const int32_t *d_lc, double *d_out, int32_t *d_status, hipStream_t s, bool may_sort)
{
    const MtgModel &m = ctx->model;
    const int nsig = m.nsho + 1;
    MtgSolveArgs sa;
    {
        const int rc = solve_args_context(ctx, B, d_lc, d_out, d_status, s, sa);
        if (rc) return rc;
        solve_args_model(m, sa);
    }
    const MtgPlanIn in = plan_input(ctx, B, may_sort && d_lc, sa);
    MtgSolvePlan plan = mtg_plan_solve(in, g_catalogue);
    sa.tp_ws = nullptr;
    sa.tp_chunks = plan.tp_chunks;
    sa.tp_gsize = plan.tp_gsize;
    sa.tp_direct = ctx->tp_direct;
    sa.tp_nr0 = m.nr0; sa.tp_nc0 = m.nc0;
    sa.sig = ctx->sig.as<int32_t>();
    if (plan.tp_ws_bytes) {
        HIP_TRY(ctx, ctx->tp_ws.reserve(plan.tp_ws_bytes));
        sa.tp_ws = ctx->tp_ws.as<double>();
    }
    sa.solo = 0; sa.left_list = nullptr; sa.left_count = nullptr;
    const int *sorted = nullptr;
    if (plan.sort) {
        mtg_trace::Range range("mtg:sort (evaluations by structure, light curve)");
        const size_t tmp = mtg_sort_temp_bytes(B, mtg_sort_key_bits(ctx->L, nsig));
        HIP_TRY(ctx, ctx->sort_keys.reserve((size_t)B * 4));
        HIP_TRY(ctx, ctx->sort_keys_out.reserve((size_t)B * 4));
        HIP_TRY(ctx, ctx->sort_order.reserve((size_t)B * 4));
        HIP_TRY(ctx, ctx->sort_tmp.reserve(tmp > 0 ? tmp : 16));
        HIP_TRY(ctx, mtg_launch_sort_by_lightcurve(B, d_status, nsig > 1 ? ctx->sig.as<int32_t>() : nullptr, d_lc, ctx->L, nsig,
                                                   ctx->sort_keys.as<uint32_t>(), ctx->sort_keys_out.as<uint32_t>(),
                                                   ctx->sort_order.as<int>(), ctx->sort_tmp.p, tmp, s));
        sorted = ctx->sort_order.as<int>();
    }
    switch (plan.family) {
    case MTG_SOLVE_TP_BIG:
        sa.list = nullptr;
        sa.count_ptr = nullptr;
        mtg_launch_tp_big(sa, B, s);
        break;
    case MTG_SOLVE_TP_FUSED:
        sa.list = bank_lists(ctx);
        sa.count_ptr = bank_counts(ctx);
        mtg_find_tp_fused_solver(m.nr0, m.nc0, nsig, plan.fused_lanes)(sa, B, s);
        break;
    case MTG_SOLVE_PIPE: {
        sa.list = sorted;            // nsig == 1: the sorted order, or NULL = the caller's
        sa.count_ptr = nullptr;
        sa.seg_counts = nsig > 1 ? bank_counts(ctx) : nullptr;
        sa.seg_k = 0;
        int paired = 0;
        if (std::atomic_load(&ctx->pair)) {
            const int rc = pair_launch(ctx, sa, B, MtgPipeShapeId{m.nr0, m.nc0, nsig, m.last_b0 ? 1 : 0}, s, &paired);
            if (rc) return rc;
        }
        if (paired) mtg_plan_name_paired(plan, in);
        else mtg_find_pipe_solver(m.nr0, m.nc0, nsig, m.last_b0)(sa, B, s);
        break;
    }
    case MTG_SOLVE_MULTI:
        sa.list = sorted;
        sa.count_ptr = nullptr;
        sa.seg_counts = bank_counts(ctx);
        sa.seg_k = 0;
        mtg_find_multi_solver(m.nr0, m.nc0, nsig, m.last_b0)(sa, B, s);
        break;
    case MTG_SOLVE_STRUCTURES: {
        const int rc = launch_structures(ctx, plan, sa, sorted, B, s);
        if (rc) return rc;
        break;
    }
    }
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "%s", plan.name);
    HIP_TRY(ctx, hipGetLastError());
    return MTG_OK;
}

int check_ready(mtg_ctx *ctx, bool need_model)
{
    if (!ctx) return MTG_E_ARG;
    if (ctx->N <= 0) return fail(ctx, MTG_E_STATE, "mtg_set_lightcurves has not been called");
    if (need_model && !ctx->has_model) return fail(ctx, MTG_E_STATE, "mtg_set_model has not been called");
    return MTG_OK;
}

// The stream and the stages of one host-pointer call in flight.  Once the entry has its stream nothing returns early: a
// step runs only while the call is ok(), the first failure is kept -- a HIP error in `e`, or in `rc` the code of a helper
// that has written its own report -- and finish() is the one way out: it waits for the stream whatever happened, so that
// the caller's arrays are no longer the target of a queued copy when the call returns, and reports "who: <HIP error>".
struct StagedCall {
    mtg_ctx *ctx;
    const char *who;
    hipStream_t s = nullptr;
    hipError_t e = hipSuccess;
    int rc = MTG_OK;
    struct Room { DevBuf &buf; size_t bytes; };
    StagedCall(mtg_ctx *ctx_, const char *who_) : ctx(ctx_), who(who_) {}

    bool ok() const { return rc == MTG_OK && e == hipSuccess; }
    template <class F> void then(F step) { if (ok()) e = step(); }   // step() -> hipError_t
    void reserve(std::initializer_list<Room> rooms) { for (const Room &r : rooms) then([&] { return r.buf.reserve(r.bytes); }); }
    void upload(void *dev, const void *host, size_t bytes) { then([&] { return hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s); }); }
    void gather(void *host, const void *dev, size_t bytes) { then([&] { return hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s); }); }
    void sync() { then([&] { return hipStreamSynchronize(s); }); }
    int finish();
};

// the stream waited for: the end of every staged call, and the only place where one reports a HIP error
int StagedCall::finish()
{
    const hipError_t drained = hipStreamSynchronize(s);
    if (ok()) e = drained;
    if (rc) return rc;
    return e == hipSuccess ? MTG_OK : fail(ctx, MTG_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

// One host-pointer call over rows of theta (`who`: mtg_loglike_batch, mtg_loglike_coeffs, mtg_predict, mtg_predict_at,
// mtg_predict_terms, mtg_gp_draw, mtg_gp_cond_draw, mtg_loglike_grad, mtg_apply_inverse).  The entry runs ready, its own
// argument checks and begin -- in that order; each returns at once, nothing is queued yet -- then the stages below and its
// own reservations and launches, and leaves through finish(status).
struct RowCall : StagedCall {
    int64_t B;
    const double *theta;             // [B][P] on the host
    const int32_t *lc_index;         // [B] on the host, or NULL: light curve 0
    int add_prior;
    const int32_t *d_lc = nullptr;   // stage_inputs: lc_index on the device, NULL when lc_index is (never an earlier call's)
    RowCall(mtg_ctx *ctx_, const char *who_, int64_t B_, const double *theta_, const int32_t *lc_index_, int add_prior_)
        : StagedCall(ctx_, who_), B(B_), theta(theta_), lc_index(lc_index_), add_prior(add_prior_) {}

    int ready(bool need_model = true) { return check_ready(ctx, need_model); }
    int bad_arguments() { return fail(ctx, MTG_E_ARG, "%s: bad arguments", who); }
    int begin(bool refuse_profile);
    void stage_inputs(bool with_theta = true);
    void expand(MtgRowArgs &head, DevBuf *owner = nullptr);
    int finish(int32_t *status);
};

// the model's profile mean refused where the entry cannot read one, the light-curve indices, the device and the context's
// stream, ordered after whatever ran last on a caller's
int RowCall::begin(bool refuse_profile)
{
    int r = refuse_profile ? refuse_profile_mean(ctx, who) : MTG_OK;
    if (r || (r = check_lc_index(ctx, B, lc_index)) || (r = use_device(ctx))) return r;
    s = ctx->stream;
    return enter_stream(ctx, s);
}

// room for B rows of theta, results and statuses in the context's staging; theta and lc_index uploaded
void RowCall::stage_inputs(bool with_theta)
{
    const size_t rows = (size_t)B;
    const int P = ctx->model.P;
    reserve({{ctx->theta, with_theta ? rows * (P > 0 ? P : 1) * 8 : 0}, {ctx->out, rows * 8}, {ctx->status, rows * 4},
             {ctx->lc, lc_index ? rows * 4 : 0}});
    if (with_theta && P > 0) upload(ctx->theta.p, theta, rows * P * 8);
    if (lc_index) upload(ctx->lc.p, lc_index, rows * 4);
    d_lc = lc_index ? ctx->lc.as<int32_t>() : nullptr;
}

// The staged theta expanded into the coefficient workspace -- the prior's verdict in ctx->status, the structure of every
// row in ctx->sig -- and the head of the per-row kernels' arguments filled for the whole batch.  (ctx->sig, like
// ctx->coef, is rewritten by every expansion and read by nothing before the next one.)  owner (mtg_predict_terms): room
// for, and from this expansion, the term of every slot of every accepted row, [nr_max + nc_max][cstride] int32.
void RowCall::expand(MtgRowArgs &head, DevBuf *owner)
{
    const MtgModel &m = ctx->model;
    if (ok()) rc = reserve_workspace(ctx, B, model_nslots(m), 1);
    if (owner) reserve({{*owner, (size_t)(m.nr_max + m.nc_max) * (size_t)ctx->cstride * 4}});
    then([&] {
        mtg_launch_prepare(make_prep_args(ctx, B, ctx->theta.as<double>(), add_prior, ctx->out.as<double>(),
                                          ctx->status.as<int32_t>(), 1), s, owner ? owner->as<int32_t>() : nullptr);
        return hipGetLastError();
    });
    head.coef = ctx->coef.as<double>(); head.cstride = ctx->cstride; head.lay = MtgCoefLayout{m.nr_max, m.nc_max};
    head.nr0 = m.nr0; head.nc0 = m.nc0; head.sig = ctx->sig.as<int32_t>();
    head.row0 = 0; head.B = B; head.lc_index = d_lc; head.status = ctx->status.as<int32_t>();
    head.dxt = ctx->dxt.as<double2>(); head.yv = ctx->yv.as<double2>();
    head.N = ctx->N; head.t_stride = ctx->t_per_lc ? ctx->N : 0;
}

// the statuses on their way to the host behind the entry's own results (NULL: the entry has fetched them), then the
// stream waited for: the end of every row entry
int RowCall::finish(int32_t *status)
{
    if (status) gather(status, ctx->status.p, (size_t)B * 4);
    return StagedCall::finish();
}

// The workspace of one slab of Bs rows of the new-time prediction (mtg_predict_at, mtg_gp_cond_draw) and everything of
// its kernels' arguments but the slab's rows: the M times uploaded, with the order to visit them in unless they ascend
// as given (order == NULL)
struct PredictAtRoom {
    DevBuf work, ckf, ckb, ckr, mu, var, ts, order;
    void reserve(RowCall &c, MtgPredictAtArgs &qa, int64_t Bs, int J, int64_t M, const double *h_ts, const int64_t *h_order,
                 bool want_var)
    {
        const int64_t N = c.ctx->N;
        const size_t row_bytes = (size_t)N * (3 * J + 3) * 8, tri_bytes = (size_t)(J * (J + 1) / 2) * 8;
        const int64_t nck = (N + MTG_PAT_C - 1) / MTG_PAT_C;
        const size_t ck_bytes = (size_t)nck * (tri_bytes + J * 8), ts_bytes = (size_t)M * 8;
        c.reserve({{work, (size_t)Bs * row_bytes + 8}, {ckf, (size_t)Bs * ck_bytes + 8}, {ckb, (size_t)Bs * ck_bytes + 8},
                   {ckr, (size_t)Bs * tri_bytes + 8}, {mu, (size_t)Bs * ts_bytes}, {var, want_var ? (size_t)Bs * ts_bytes : 0},
                   {ts, ts_bytes}, {order, h_order ? ts_bytes : 0}});
        c.upload(ts.p, h_ts, ts_bytes);
        if (h_order) c.upload(order.p, h_order, ts_bytes);
        qa.work = work.as<double>();
        qa.nck = nck; qa.ckf = ckf.as<double>(); qa.ckb = ckb.as<double>(); qa.ckr = ckr.as<double>(); qa.want_var = want_var ? 1 : 0;
        qa.M = M; qa.ts = ts.as<double>(); qa.order = h_order ? order.as<int64_t>() : nullptr;
        qa.mu = mu.as<double>(); qa.var = want_var ? var.as<double>() : nullptr;
        qa.data = nullptr;
    }
};

// what mtg_lag_sums and mtg_cross_sums refuse about their bins, in the order both always did (lag: no negative lags)
int lag_refuse_edges(mtg_ctx *ctx, const char *who, int nbins, const double *edges, bool nothing_asked, bool allow_negative)
{
    if (nbins < 1 || nbins > MTG_LAG_MAX_BINS) return fail(ctx, MTG_E_ARG, "%s: nbins = %d is outside 1 .. %d", who, nbins, MTG_LAG_MAX_BINS);
    if (!edges) return fail(ctx, MTG_E_ARG, "%s: need nbins + 1 edges", who);
    if (nothing_asked) return fail(ctx, MTG_E_ARG, "%s: every output is NULL", who);
    for (int b = 0; b <= nbins; ++b)
        if (!std::isfinite(edges[b])) return fail(ctx, MTG_E_ARG, "%s: edges[%d] is not finite", who, b);
    if (!allow_negative && edges[0] < 0.0) return fail(ctx, MTG_E_ARG, "%s: edges[0] = %g is negative", who, edges[0]);
    for (int b = 0; b < nbins; ++b)
        if (!(edges[b] < edges[b + 1])) return fail(ctx, MTG_E_ARG, "%s: edges[%d] = %g is not above edges[%d] = %g", who, b + 1, edges[b + 1], b, edges[b]);
    return MTG_OK;
}

// K optional outputs of one entry, each NULL or the same number of 8-byte entries, in the order of its arguments: where
// the host wants each and its room on the device.  (mtg_lag_sums, mtg_cross_sums: the order of the planner's MTG_LAG_* /
// MTG_CROSS_* bits.)
template <int K>
struct OptionalOutputs {
    void *host[K];
    DevBuf dev[K];
    size_t bytes = 0;
    int what() const
    {
        int bits = 0;
        for (int k = 0; k < K; ++k) bits |= host[k] ? 1 << k : 0;
        return bits;
    }
    void reserve(StagedCall &c, size_t entries)
    {
        bytes = entries * 8;
        for (int k = 0; k < K; ++k) c.reserve({{dev[k], host[k] ? bytes : 0}});
    }
    template <class T = double> T *at(int k, int64_t entry = 0) const { return host[k] ? dev[k].template as<T>() + entry : nullptr; }   // on the device
    void gather(StagedCall &c)
    {
        for (int k = 0; k < K; ++k)
            if (host[k]) c.gather(host[k], dev[k].p, bytes);
    }
};
static_assert(MTG_LAG_COUNT == 1 << 0 && MTG_LAG_LAG == 1 << 1 && MTG_LAG_SF == 1 << 2 && MTG_LAG_CF == 1 << 3 && MTG_LAG_CF2 == 1 << 4 &&
                  MTG_LAG_NOISE == 1 << 5, "bit k is output k of mtg_lag_sums");
static_assert(MTG_CROSS_COUNT == 1 << 0 && MTG_CROSS_LAG == 1 << 1 && MTG_CROSS_CF == 1 << 2 && MTG_CROSS_CF2 == 1 << 3 && MTG_CROSS_SA == 1 << 4 &&
                  MTG_CROSS_SB == 1 << 5 && MTG_CROSS_SAA == 1 << 6 && MTG_CROSS_SBB == 1 << 7, "bit k is output k of mtg_cross_sums");

// One host-pointer call on the resident light curves alone: no model, no rows of theta (`who`: mtg_lomb_scargle / _multi,
// mtg_lomb_scargle_envelope / _multi, mtg_epoch_fold, mtg_phase_fold, mtg_wwz, mtg_lag_sums, mtg_cross_sums).  The entry
// runs ready, its refusals and begin -- in that order; each returns at once, nothing is queued yet -- then reserves what
// is its own, takes the pre-pass arguments from args() (the last of the call's allocations: no hipMalloc behind a queued
// copy), uploads, queues its kernels with run_slabs(), gathers and leaves through finish().
struct ResidentCall : StagedCall {
    DevBuf stats, peak, index;   // args: the pre-pass's [L][4]; reserve_peaks: [L] maxima and where each is
    using StagedCall::StagedCall;

    int ready() { return check_ready(ctx, false); }
    // the device and the context's stream, ordered after whatever ran last on a caller's
    int begin()
    {
        if (const int r = use_device(ctx)) return r;
        s = ctx->stream;
        return enter_stream(ctx, s);
    }
    // room for the maximum of every light curve and the first index attaining it, when either is wanted
    void reserve_peaks(bool want)
    {
        const size_t bytes = want ? (size_t)ctx->L * 8 : 0;
        reserve({{peak, bytes}, {index, bytes}});
    }
    void gather_peaks(double *peak_power, int64_t *peak_index)
    {
        if (peak_power) gather(peak_power, peak.p, (size_t)ctx->L * 8);
        if (peak_index) gather(peak_index, index.p, (size_t)ctx->L * 8);
    }
    // The arguments of the pre-pass (mtg_launch_lomb_scargle_stats) and of the sweeps that read its statistics: the resident
    // set, the call's choices, the F uploaded frequencies (none: 0, NULL), where the powers go and, with want_peak, the peaks.
    MtgLombScargleArgs args(int nterms, int normalization, int weighted, int64_t F, const double *d_freqs, double *d_power, bool want_peak)
    {
        reserve({{stats, (size_t)ctx->L * 32}});
        reserve_peaks(want_peak);
        MtgLombScargleArgs qa;
        qa.dxt = ctx->dxt.as<double2>(); qa.yv = ctx->yv.as<double2>();
        qa.N = ctx->N; qa.t_stride = ctx->t_per_lc ? ctx->N : 0; qa.L = ctx->L;
        qa.weighted = weighted ? 1 : 0; qa.normalization = normalization; qa.nterms = nterms;
        qa.stats = stats.as<double>(); qa.F = F; qa.freqs = d_freqs; qa.power = d_power;
        qa.peak_power = want_peak ? peak.as<double>() : nullptr; qa.peak_index = want_peak ? index.as<int64_t>() : nullptr;
        return qa;
    }
    // The call's timed work (mtg_last_kernel_ms): the pre-pass, then for the slabs [i0, i0 + n) of `extent`, `slab` at a time,
    // launch(i0, n) -> hipError_t and collect(i0, n), the slab's copies to the host (none: every output is whole on the
    // device).  One stream: the next slab's kernels overwrite the workspace only after this slab's kernels and copies.
    // After the first failure nothing more is queued.
    template <class Prepass, class Launch, class Collect = void (*)(int64_t, int64_t)>
    void run_slabs(int64_t extent, int64_t slab, Prepass prepass, Launch launch, Collect collect = [](int64_t, int64_t) {})
    {
        then([&] { return hipEventRecord(ctx->ev0, s); });
        then([&] { return prepass(), hipGetLastError(); });
        if (ok()) e = for_each_slab(extent, slab, [&](int64_t i0, int64_t n) {
            then([&] { return launch(i0, n); });
            if (i0 + n == extent) then([&] { return hipEventRecord(ctx->ev1, s); });   // up to the last slab's kernels
            collect(i0, n);
            return e;
        });
        if (ok()) ctx->timed = true;
    }
};

// the refusals the resident-set entries share, each written once; an entry calls them in the order of its own messages
int refuse_no_freqs(mtg_ctx *ctx, const char *who, int64_t F, const double *freqs)
{
    return F < 1 || !freqs ? fail(ctx, MTG_E_ARG, "%s: need F >= 1 frequencies", who) : MTG_OK;
}
int refuse_normalization(mtg_ctx *ctx, const char *who, int normalization)
{
    return normalization < MTG_LS_STANDARD || normalization > MTG_LS_PSD ? fail(ctx, MTG_E_ARG, "%s: unknown normalization %d", who, normalization) : MTG_OK;
}
int refuse_bad_freqs(mtg_ctx *ctx, const char *who, int64_t F, const double *freqs)
{
    for (int64_t k = 0; k < F; ++k)
        if (!std::isfinite(freqs[k]) || freqs[k] <= 0.0)
            return fail(ctx, MTG_E_ARG, "%s: freqs[%lld] = %g is not a finite positive frequency", who, (long long)k, freqs[k]);
    return MTG_OK;
}

}  // namespace

extern "C" {

MTG_API int mtg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

MTG_API const char *mtg_version(void) { return "mtg-hip 0.1 (gfx950)"; }

MTG_API int mtg_term_nparams(int kind) { return nparams(kind); }

MTG_API int mtg_mean_nparams(int kind) { return mtg_mean_nparams_of(kind); }

MTG_API int mtg_structure_supported(int jr, int jc) { return mtg_find_solver(jr, jc) ? 1 : 0; }

static mtg_ctx *create_context(int device, int part, int parts)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        fail(nullptr, MTG_E_NODEVICE, "no HIP device available (%s)",
             e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(nullptr, MTG_E_ARG, "device %d out of range [0, %d)", device, n);
        return nullptr;
    }
    if (parts < 1 || parts > 8 || part < 0 || part >= parts) {
        fail(nullptr, MTG_E_ARG, "slice %d of %d compute-unit slices: 1 to 8 slices", part, parts);
        return nullptr;
    }
    mtg_ctx *ctx = new (std::nothrow) mtg_ctx();
    if (!ctx) return nullptr;
    ctx->device = device;
    bool ok = hipSetDevice(device) == hipSuccess;
    if (ok && (hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ctx->cus <= 0))
        ctx->cus = 256;
    if (ok && parts > 1) {
        // a contiguous run of mask bits per slice (MTG_CU_SLICE_INTERLEAVED=1: bit i to slice i mod parts): the contexts
        // of different slices run their kernels side by side on disjoint compute units (a queue's CU mask), whatever the
        // order their launches arrive in.  (The driver deals the bits of a mask round over the XCDs: a contiguous run
        // leaves every XCD with its share of enabled compute units, which a dispatch split over all XCDs needs.)
        uint32_t mask[16] = {};
        int mine = 0;
        const bool interleaved = mtg_measure_env("MTG_CU_SLICE_INTERLEAVED") && atoi(mtg_measure_env("MTG_CU_SLICE_INTERLEAVED")) == 1;
        const int per = ctx->cus / parts;
        for (int i = 0; i < ctx->cus && i < 512; ++i)
            if (interleaved ? i % parts == part : (i / per == part || (part == parts - 1 && i / per >= parts))) {
                mask[i / 32] |= 1u << (i % 32);
                ++mine;
            }
        ok = hipExtStreamCreateWithCUMask(&ctx->stream, (uint32_t)((ctx->cus + 31) / 32), mask) == hipSuccess;
        ctx->cus = mine;
    } else if (ok) {
        ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    }
    if (!ok || hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->foreign_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->own_done, hipEventDisableTiming) != hipSuccess) {
        fail(nullptr, MTG_E_HIP, "could not create stream/events on device %d", device);
        delete ctx;
        return nullptr;
    }
    return ctx;
}

MTG_API mtg_ctx *mtg_create(int device) { return create_context(device, 0, 1); }

MTG_API mtg_ctx *mtg_create_on_slice(int device, int part, int parts) { return create_context(device, part, parts); }

MTG_API int mtg_unpair_contexts(mtg_ctx *ctx);

MTG_API void mtg_destroy(mtg_ctx *ctx)
{
    if (!ctx) return;
    (void)mtg_unpair_contexts(ctx);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->foreign_pending) (void)hipEventSynchronize(ctx->foreign_done);
    // In this order: the RCCL / host exchange, then the hipFFT plans -- reset here, by hand, because they must go before
    // the stream they were set on, and the stream is destroyed below, before the members are.  The device buffers need
    // no list: ~DevBuf frees each with `delete ctx`.
    shard_release(ctx);
    ctx->reset_plans();
    for (hipEvent_t e : ctx->prof_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ens.shard_ev) (void)hipEventDestroy(e);
    if (ctx->foreign_done) (void)hipEventDestroy(ctx->foreign_done);
    if (ctx->own_done) (void)hipEventDestroy(ctx->own_done);
    for (hipStream_t st : ctx->side) if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t ev : ctx->side_done) if (ev) (void)hipEventDestroy(ev);
    if (ctx->fork) (void)hipEventDestroy(ctx->fork);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

MTG_API int mtg_set_window_bytes(mtg_ctx *ctx, uint64_t bytes)
{
    if (!ctx) return MTG_E_ARG;
    if (bytes < 16 || bytes > 0xffffffffull) return fail(ctx, MTG_E_ARG, "mtg_set_window_bytes: 16 <= bytes < 2^32");
    if (ctx->N > 0 && (uint64_t)ctx->N * 16u > bytes)
        return fail(ctx, MTG_E_ARG, "mtg_set_window_bytes: a resident light curve (%lld samples) does not fit", (long long)ctx->N);
    ctx->window_bytes = bytes;
    return MTG_OK;
}

MTG_API const char *mtg_last_error(const mtg_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

static int set_lightcurves_common(mtg_ctx *ctx, int64_t N, int64_t L, const double *t, int t_per_lc,
                                  const double *y, const double *yerr, const double *y_offset,
                                  hipMemcpyKind kind)
{
    if (!ctx) return MTG_E_ARG;
    if (N <= 0 || L <= 0 || !t || !y || !yerr)
        return fail(ctx, MTG_E_ARG, "mtg_set_lightcurves: need N > 0, L > 0 and non-NULL t, y, yerr");
    // one light curve must fit the reach of a buffer descriptor; the set itself may fill the HBM
    if ((uint64_t)N * 16u > ctx->window_bytes)
        return fail(ctx, MTG_E_ARG, "light curve too long: N * 16 bytes must stay below %llu",
                    (unsigned long long)ctx->window_bytes);
    if (L > 0x7fffffff) return fail(ctx, MTG_E_ARG, "too many light curves (32-bit indices)");
    int rc = use_device(ctx);
    if (rc) return rc;
    mtg_trace::Range range("mtg:set_lightcurves (upload, sigma^2, dx)");
    const int64_t t_rows = t_per_lc ? L : 1;
    rc = enter_stream(ctx, ctx->stream);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, ctx->dxt.reserve((size_t)t_rows * N * 16));
    HIP_TRY(ctx, ctx->yv.reserve((size_t)L * N * 16));
    // staged in blocks of light curves (<= ~256 MiB of staging per array), so that a resident set
    // of tens of GB does not need its own size again in scratch
    int64_t block = ((int64_t)256 << 20) / (N * 8);
    if (block < 1) block = 1;
    if (block > L) block = L;
    HIP_TRY(ctx, ctx->t_tmp.reserve((size_t)(t_per_lc ? block : 1) * N * 8));
    HIP_TRY(ctx, ctx->y_tmp.reserve((size_t)block * N * 8));
    HIP_TRY(ctx, ctx->dy_tmp.reserve((size_t)block * N * 8));
    HIP_TRY(ctx, ctx->dxmax.reserve(64));
    HIP_TRY(ctx, hipMemsetAsync(ctx->dxmax.p, 0, 16, ctx->stream));  // [0] max dx, [1] "unsorted" flag
    if (y_offset) HIP_TRY(ctx, ctx->off_tmp.reserve((size_t)block * 8));
    for (int64_t l0 = 0; l0 < L; l0 += block) {
        const int64_t lb = l0 + block <= L ? block : L - l0;
        const int64_t tr = t_per_lc ? lb : (l0 == 0 ? 1 : 0);  // a shared sampling is set up once
        if (tr)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->t_tmp.p, t + (t_per_lc ? l0 * N : 0), (size_t)tr * N * 8, kind, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->y_tmp.p, y + l0 * N, (size_t)lb * N * 8, kind, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dy_tmp.p, yerr + l0 * N, (size_t)lb * N * 8, kind, ctx->stream));
        const double *d_off = nullptr;
        if (y_offset) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->off_tmp.p, y_offset + l0, (size_t)lb * 8, kind, ctx->stream));
            d_off = ctx->off_tmp.as<double>();
        }
        mtg_launch_lc_setup(N, lb, tr, ctx->t_tmp.as<double>(), ctx->y_tmp.as<double>(), ctx->dy_tmp.as<double>(),
                            d_off, ctx->dxt.as<double2>() + (t_per_lc ? l0 * N : 0), ctx->yv.as<double2>() + l0 * N,
                            ctx->dxmax.as<double>(), ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        // the staging buffers are reused by the next block; pageable host copies have returned by
        // now, device-to-device ones are ordered on the stream
    }
    uint64_t flags[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(flags, ctx->dxmax.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flags[1]) {  // device-resident times cannot be checked on the host
        ctx->N = 0; ctx->L = 0;
        return fail(ctx, MTG_E_ARG, "the input coordinates must be sorted");
    }
    ctx->N = N; ctx->L = L; ctx->t_per_lc = t_per_lc ? 1 : 0;
    return MTG_OK;
}

MTG_API int mtg_set_lightcurves(mtg_ctx *ctx, int64_t N, int64_t L, const double *t, int t_per_lc,
                                const double *y, const double *yerr, const double *y_offset)
{
    if (!ctx) return MTG_E_ARG;
    if (N <= 0 || L <= 0 || !t || !y || !yerr)
        return fail(ctx, MTG_E_ARG, "mtg_set_lightcurves: need N > 0, L > 0 and non-NULL t, y, yerr");
    // celerite.GP.compute raises ValueError for unsorted times
    const int64_t t_rows = t_per_lc ? L : 1;
    for (int64_t r = 0; r < t_rows; ++r)
        for (int64_t n = 1; n < N; ++n)
            if (!(t[r * N + n] >= t[r * N + n - 1]))
                return fail(ctx, MTG_E_ARG, "the input coordinates must be sorted");
    return set_lightcurves_common(ctx, N, L, t, t_per_lc, y, yerr, y_offset, hipMemcpyHostToDevice);
}

MTG_API int mtg_set_lightcurves_device(mtg_ctx *ctx, int64_t N, int64_t L, const double *d_t,
                                       int t_per_lc, const double *d_y, const double *d_yerr,
                                       const double *d_y_offset)
{
    return set_lightcurves_common(ctx, N, L, d_t, t_per_lc, d_y, d_yerr, d_y_offset, hipMemcpyDeviceToDevice);
}

MTG_API int mtg_set_model(mtg_ctx *ctx, int nterms, const int32_t *kinds, const double *term_extra,
                          int mean_kind, int PF, const double *full_values, int P,
                          const int32_t *free_index, const double *bounds)
{
    if (!ctx) return MTG_E_ARG;
    if (nterms <= 0 || nterms > MTG_MAX_TERMS || !kinds)
        return fail(ctx, MTG_E_ARG, "mtg_set_model: nterms must be in [1, %d]", MTG_MAX_TERMS);
    if (mtg_mean_nparams_of(mean_kind) < 0)
        return fail(ctx, MTG_E_ARG, "mtg_set_model: unknown mean kind %d", mean_kind);
    MtgModel m;
    memset(&m, 0, sizeof m);
    m.nterms = nterms;
    m.mean_kind = mean_kind;
    int off = 0;
    for (int i = 0; i < nterms; ++i) {
        const int np = nparams(kinds[i]);
        if (np < 0) return fail(ctx, MTG_E_ARG, "mtg_set_model: unknown term kind %d", kinds[i]);
        m.kinds[i] = kinds[i];
        m.poff[i] = off;
        m.extra[i] = term_extra ? term_extra[i] : 0.01;
        off += np;
        switch (kinds[i]) {
        case MTG_TERM_REAL: case MTG_TERM_DRW: m.nr0 += 1; break;
        case MTG_TERM_JITTER: break;
        case MTG_TERM_SHO: m.nc0 += 1; m.nsho += 1; break;
        default: m.nc0 += 1; break;
        }
    }
    m.nk = off;
    // the last complex slot: slots are handed out in term order, an over-damped SHOTerm takes none -- so it holds
    // the last term that is complex whatever its parameters, if that term comes after every SHOTerm
    for (int i = nterms - 1; i >= 0; --i) {
        const int kd = kinds[i];
        if (kd == MTG_TERM_REAL || kd == MTG_TERM_DRW || kd == MTG_TERM_JITTER) continue;
        m.last_b0 = kd == MTG_TERM_LORENTZIAN || kd == MTG_TERM_COMPLEX3 || kd == MTG_TERM_COSINUS;
        break;
    }
    const int nmean = mtg_mean_nparams_of(mean_kind);
    if (PF != off + nmean)
        return fail(ctx, MTG_E_ARG, "mtg_set_model: PF = %d but the terms + mean hold %d parameters",
                    PF, off + nmean);
    if (PF > MTG_MAX_PARAMS) return fail(ctx, MTG_E_ARG, "mtg_set_model: more than %d parameters", MTG_MAX_PARAMS);
    if (P < 0 || P > PF || (P > 0 && !free_index) || !full_values)
        return fail(ctx, MTG_E_ARG, "mtg_set_model: bad P / free_index / full_values");
    m.PF = PF;
    m.P = P;
    for (int k = 0; k < PF; ++k) {
        m.src[k] = -1;
        m.defaults[k] = full_values[k];
        m.lo[k] = bounds ? bounds[2 * k] : -INFINITY;
        m.hi[k] = bounds ? bounds[2 * k + 1] : INFINITY;
    }
    for (int i = 0; i < P; ++i) {
        if (free_index[i] < 0 || free_index[i] >= PF || m.src[free_index[i]] != -1)
            return fail(ctx, MTG_E_ARG, "mtg_set_model: free_index[%d] = %d invalid or repeated", i,
                        free_index[i]);
        m.src[free_index[i]] = i;
    }
    m.nr_max = m.nr0 + 2 * m.nsho;
    m.nc_max = m.nc0;
    for (int k = 0; k <= m.nsho; ++k) {
        const int nr = m.nr0 + 2 * k, nc = m.nc0 - k;
        if (!find_sweep(mean_kind, nr, nc))
            return fail(ctx, MTG_E_UNSUPPORTED,
                        "mtg_set_model: no compiled kernel for %d real + %d complex terms (J = %d > %d?)",
                        nr, nc, nr + 2 * nc, MTG_MAX_J);
    }
    ctx->model = m;
    ctx->has_model = true;
    return MTG_OK;
}

MTG_API int mtg_loglike_batch_device(mtg_ctx *ctx, int64_t B, const double *d_theta,
                                     const int32_t *d_lc_index, int add_prior, double *d_out,
                                     int32_t *d_status, void *stream)
{
    int rc = check_ready(ctx, true);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!d_out || !d_status || (!d_theta && ctx->model.P > 0))))
        return fail(ctx, MTG_E_ARG, "mtg_loglike_batch_device: bad arguments");
    if (B == 0) return MTG_OK;
    if (B > INT32_MAX) return fail(ctx, MTG_E_ARG, "batch too large");
    rc = use_device(ctx);
    if (rc) return rc;
    hipStream_t s = stream == MTG_STREAM_CONTEXT ? ctx->stream : (hipStream_t)stream;  // NULL: HIP's default stream
    rc = enter_stream(ctx, s);
    if (rc) return rc;
    ctx->lc_grouped_hint = 0;   // device-resident indices: the host cannot see their order
    rc = run_model_batch(ctx, B, d_theta, d_lc_index, add_prior, d_out, d_status, s);
    // whatever happened: kernels may already be queued on the caller's stream, and the next call on another stream
    // must wait for them before it touches the shared workspaces (the first error is the one reported)
    const std::string first_error = ctx->err;
    const int rc_leave = leave_stream(ctx, s);
    if (rc) { ctx->err = first_error; return rc; }
    return rc_leave;
}

MTG_API int mtg_loglike_batch(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index,
                              int add_prior, double *out, int32_t *status)
{
    RowCall c{ctx, "mtg_loglike_batch", B, theta, lc_index, add_prior};
    int rc = c.ready();
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!out || !status || (!theta && ctx->model.P > 0)))) return c.bad_arguments();
    if (B == 0) return MTG_OK;
    if (B > INT32_MAX) return fail(ctx, MTG_E_ARG, "batch too large");
    if ((rc = c.begin(false))) return rc;
    // is the caller's order already grouped by light curve?  Then the sweep keeps it
    int64_t runs = 1;
    bool ascending = true;
    for (int64_t b = 1; lc_index && b < B; ++b) {
        if (lc_index[b] != lc_index[b - 1]) ++runs;
        if (lc_index[b] < lc_index[b - 1]) ascending = false;
    }
    // grouped: already in ascending order (sorting changes nothing), or in runs of equal indices long enough that a
    // wave of 64 lanes straddles two or three light curves at most
    ctx->lc_grouped_hint = !lc_index || ascending || B / runs >= 32;
    c.stage_inputs();
    if (c.ok()) c.rc = run_model_batch(ctx, B, ctx->theta.as<double>(), c.d_lc, add_prior, ctx->out.as<double>(),
                                       ctx->status.as<int32_t>(), c.s);
    mtg_trace::Range range("mtg:gather (lnP, status -> host)");
    c.gather(out, ctx->out.p, (size_t)B * 8);
    return c.finish(status);
}

MTG_API int mtg_loglike_coeffs(mtg_ctx *ctx, int64_t B, int jr, int jc, const double *a_real,
                               const double *c_real, const double *a_comp, const double *b_comp,
                               const double *c_comp, const double *d_comp, const double *jitter,
                               int mean_kind, const double *mean_params, const int32_t *lc_index,
                               double *out, int32_t *status)
{
    RowCall c{ctx, "mtg_loglike_coeffs", B, nullptr, lc_index, 0};
    int rc = c.ready(false);
    if (rc) return rc;
    if (B < 0 || jr < 0 || jc < 0 || (B > 0 && (!out || !status))) return c.bad_arguments();
    if ((jr > 0 && (!a_real || !c_real)) || (jc > 0 && (!a_comp || !b_comp || !c_comp || !d_comp)))
        return fail(ctx, MTG_E_ARG, "mtg_loglike_coeffs: NULL coefficient array");
    if (mtg_mean_nparams_of(mean_kind) < 0)
        return fail(ctx, MTG_E_ARG, "mtg_loglike_coeffs: unknown mean kind %d", mean_kind);
    const bool profile = mtg_mean_is_profile(mean_kind);
    if (profile && !mean_params)
        return fail(ctx, MTG_E_ARG, "mtg_loglike_coeffs: mean kind %d (%s) needs mean_params", mean_kind, mtg_mean_name(mean_kind));
    if (B == 0) return MTG_OK;
    if (B > INT32_MAX) return fail(ctx, MTG_E_ARG, "batch too large");
    mtg_solve_launcher fn = find_sweep(mean_kind, jr, jc);
    if (!fn)
        return fail(ctx, MTG_E_UNSUPPORTED, "no compiled kernel for %d real + %d complex terms", jr, jc);
    if ((rc = c.begin(false))) return rc;
    MtgCoefLayout lay{jr, jc};
    const int nslots = lay.nslots() + mtg_mean_extra_slots(mean_kind);
    if ((rc = reserve_workspace(ctx, B, nslots, 1))) return rc;
    const int64_t cs = ctx->cstride;
    // host-side transpose [B][j] -> SoA columns, then one upload
    const int nmean = mtg_mean_nparams_of(mean_kind);
    std::vector<double> h;
    try {
        h.resize((size_t)cs * nslots);
    } catch (const std::bad_alloc &) {
        return fail(ctx, MTG_E_ARG, "out of host memory");
    }
    for (int64_t b = 0; b < B; ++b) {
        double asum = jitter ? jitter[b] : 0.0;
        for (int j = 0; j < jr; ++j) {
            h[lay.ar(j) * cs + b] = a_real[b * jr + j];
            h[lay.cr(j) * cs + b] = c_real[b * jr + j];
            asum += a_real[b * jr + j];
        }
        for (int k = 0; k < jc; ++k) {
            h[lay.ac(k) * cs + b] = a_comp[b * jc + k];
            h[lay.bc(k) * cs + b] = b_comp[b * jc + k];
            h[lay.cc(k) * cs + b] = c_comp[b * jc + k];
            h[lay.dc(k) * cs + b] = d_comp[b * jc + k];
            asum += a_comp[b * jc + k];
        }
        h[lay.asum() * cs + b] = asum;
        h[lay.jit() * cs + b] = jitter ? jitter[b] : 0.0;
        // slots are (slope, intercept); a constant mean is slope 0
        const double m0 = mean_params ? mean_params[b * nmean] : 0.0;
        h[lay.mean(0) * cs + b] = nmean == 2 ? m0 : 0.0;
        h[lay.mean(1) * cs + b] = nmean == 2 ? mean_params[b * nmean + 1] : m0;
        if (profile) {   // the constants mtg_prepare_from derives on the device
            const double *p = mean_params + b * nmean;
            const MtgMeanConsts mc = mtg_mean_derive(mean_kind, p[0], p[1], p[2], p[3], nmean > 4 ? p[4] : 0.0, nmean > 5 ? p[5] : 0.0);
            h[lay.mean(0) * cs + b] = 0.0;
            h[lay.mean(1) * cs + b] = mc.level;
            for (int i = 0; i < mtg_mean_extra_slots(mean_kind); ++i) h[lay.mean_extra(i) * cs + b] = mc.ex(i);
        }
    }
    c.upload(ctx->coef.p, h.data(), h.size() * 8);   // (h lives until finish() has waited for the stream)
    c.stage_inputs(false);
    c.then([&] { return hipMemsetAsync(ctx->status.p, 0, (size_t)B * 4, c.s); });
    MtgSolveArgs sa{};   // no lists, no time-parallel workspace, no structure words: one sweep in the caller's order
    if (c.ok()) c.rc = solve_args_context(ctx, B, c.d_lc, ctx->out.as<double>(), ctx->status.as<int32_t>(), c.s, sa);
    sa.lay = lay;
    sa.mean_kind = mean_kind;
    sa.has_mean = mean_params != nullptr || jitter != nullptr;
    sa.tp_nr0 = jr; sa.tp_nc0 = jc;
    if (c.ok()) {
        ctx->timed = true;
        c.e = hipEventRecord(ctx->ev0, c.s);
    }
    if (c.ok()) {
        if (profile) mtg_mean_kernel_name(ctx->last_solver, sizeof ctx->last_solver, jr, jc, 0, " (coefficients)");
        else mtg_struct_kernel_name(ctx->last_solver, sizeof ctx->last_solver, MTG_STRUCT_SWEEP, jr, jc, 0, " (coefficients)");
        c.rc = sweep_launch(ctx, fn, sa, B, 0, c.s);
    }
    c.then([&] { return hipGetLastError(); });
    c.then([&] { return hipEventRecord(ctx->ev1, c.s); });
    c.gather(out, ctx->out.p, (size_t)B * 8);
    return c.finish(status);
}

MTG_API int mtg_ensemble_init(mtg_ctx *ctx, int64_t E, int W, uint64_t seed, const double *coords,
                              const int32_t *lc_of_ensemble)
{
    int rc = check_ready(ctx, true);
    if (rc) return rc;
    const int P = ctx->model.P;
    if (E <= 0 || W < 2 || (W & 1) || !coords || P <= 0)
        return fail(ctx, MTG_E_ARG, "mtg_ensemble_init: need E > 0, an even W >= 2, P > 0 and coords");
    if (W < 2 * P)
        return fail(ctx, MTG_E_ARG, "mtg_ensemble_init: fewer walkers (%d) than twice the dimension (%d)", W, 2 * P);
    if (E * (int64_t)W > INT32_MAX) return fail(ctx, MTG_E_ARG, "mtg_ensemble_init: too many walkers");
    if (W > MTG_MAX_WALKERS)
        return fail(ctx, MTG_E_ARG, "mtg_ensemble_init: at most %d walkers per ensemble", MTG_MAX_WALKERS);
    if (!lc_of_ensemble && E != ctx->L && ctx->L != 1)
        return fail(ctx, MTG_E_ARG, "mtg_ensemble_init: %lld ensembles but %lld light curves and no map",
                    (long long)E, (long long)ctx->L);
    rc = use_device(ctx);
    if (rc) return rc;
    const int64_t EW = E * W, EH = E * (W / 2);
    std::vector<int32_t> lc_full((size_t)EW), lc_spec((size_t)(3 * EH));
    for (int64_t e = 0; e < E; ++e) {
        const int32_t l = lc_of_ensemble ? lc_of_ensemble[e] : (ctx->L == 1 ? 0 : (int32_t)e);
        if (l < 0 || l >= ctx->L) return fail(ctx, MTG_E_ARG, "mtg_ensemble_init: light curve %d out of range", l);
        for (int w = 0; w < W; ++w) lc_full[(size_t)(e * W + w)] = l;
        for (int k = 0; k < W / 2; ++k)
            lc_spec[(size_t)(e * (W / 2) + k)] = lc_spec[(size_t)(EH + e * (W / 2) + k)] = lc_spec[(size_t)(2 * EH + e * (W / 2) + k)] = l;
    }
    CTX_STREAM(ctx, s);
    mtg_ctx::Ensembles &en = ctx->ens;
    const mtg_ctx::Ensembles::Sizes z = mtg_ctx::Ensembles::sizes(E, W, P);
    HIP_TRY(ctx, en.reserve(z));
    HIP_TRY(ctx, hipMemcpyAsync(en.coords.p, coords, z.coords, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(en.lc_full.p, lc_full.data(), z.lc_full, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(en.lc_spec.p, lc_spec.data(), z.lc_spec, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(en.naccept.p, 0, z.naccept, s));
    HIP_TRY(ctx, hipMemsetAsync(en.notpd.p, 0, z.notpd, s));
    // log-probability of the initial state (emcee evaluates p0 once); the rows are grouped by ensemble, hence by light curve
    ctx->lc_grouped_hint = 1;
    rc = run_model_batch(ctx, EW, en.coords.as<double>(), en.lc_full.as<int32_t>(), 1, en.lnp.as<double>(), en.st.as<int32_t>(), s);
    if (rc) return rc;
    mtg_launch_initial_best((int)E, W, P, en.coords.as<double>(), en.lnp.as<double>(), en.best_lnp.as<double>(),
                            en.best_coords.as<double>(), s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));  // lc_full / lc_spec live on this stack frame
    en.E = E; en.W = W; en.P = P; en.seed = seed; en.iteration = 0; en.base = ctx->stream_base; en.L = ctx->L; en.N = ctx->N;
    shard_release(ctx);  // a new set of ensembles starts unsharded (mtg_ensemble_shard_* after this call)
    return MTG_OK;
}

// ---------------------------------------------------------------------------
// Walker sharding of the device-resident ensembles (replaces the reference's
// multiprocessing.Pool.map per half-step, gpmodelling.py:245-248)
// ---------------------------------------------------------------------------
// Every rank runs the whole sampler -- same Philox key, same proposals, same accept step -- but evaluates
// only rows [rank * chunk, (rank + 1) * chunk) of each half-step's proposals; one all-gather of the
// log-probabilities (8 bytes per walker, plus the status word) on the launch stream brings the rest
// before the accept kernel.  RCCL is looked up at run time: a process that has PyTorch loaded must use
// PyTorch's copy of librccl.so.1 (two copies in one process is asking for trouble), and a library
// linked against /opt/rocm's would bring that one in first.
namespace {

struct Id128 { char b[128]; };  // ncclUniqueId
struct Rccl {
    void *lib = nullptr;
    // (ncclComm_t, ncclUniqueId, ncclDataType_t of rccl.h, restated as plain types)
    int (*GetUniqueId)(void *id128) = nullptr;
    int (*CommInitRank)(void **comm, int nranks, Id128 id, int rank) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*CommCount)(void *comm, int *count) = nullptr;
    int (*AllGather)(const void *send, void *recv, size_t count, int dtype, void *comm, hipStream_t s) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why;
} g_rccl;
enum { RCCL_INT32 = 2, RCCL_FLOAT64 = 8 };  // ncclInt32, ncclFloat64

bool rccl_load(const char *path)
{
    if (g_rccl.lib) return true;
    void *h = nullptr;
    if (path && *path) h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);  // the copy already in the process (PyTorch's)
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        g_rccl.why = std::string("librccl.so.1 not found: ") + (dlerror() ? dlerror() : "");
        return false;
    }
    auto sym = [&](const char *n) { return dlsym(h, n); };
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))sym("ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))sym("ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
    g_rccl.CommCount = (decltype(g_rccl.CommCount))sym("ncclCommCount");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))sym("ncclAllGather");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))sym("ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))sym("ncclGroupEnd");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllGather || !g_rccl.GroupStart ||
        !g_rccl.GroupEnd || !g_rccl.GetErrorString) {
        g_rccl.why = "librccl.so.1 lacks one of the nccl* entry points";
        return false;
    }
    g_rccl.lib = h;
    return true;
}

#define RCCL_TRY(ctx, call)                                                                          \
    do {                                                                                             \
        int r__ = (call);                                                                            \
        if (r__ != 0) return fail((ctx), MTG_E_HIP, "%s failed: %s", #call, g_rccl.GetErrorString(r__)); \
    } while (0)

void shard_release(mtg_ctx *ctx)
{
    mtg_ctx::Ensembles::Shard &sh = ctx->ens.shard;
    if (sh.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(sh.comm);
    if (sh.h_lnp) (void)hipHostFree(sh.h_lnp);
    if (sh.h_st) (void)hipHostFree(sh.h_st);
    sh = {};
    ctx->ens.shard_generation.fetch_add(1);
}

// rows of the half-step batch this rank evaluates, and buffers large enough for the padded all-gather
int shard_layout(mtg_ctx *ctx, int rank, int world)
{
    mtg_ctx::Ensembles &en = ctx->ens;
    if (en.E <= 0) return fail(ctx, MTG_E_STATE, "mtg_ensemble_init has not been called");
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, MTG_E_ARG, "mtg_ensemble_shard: rank %d of %d", rank, world);
    const int64_t EH = en.E * (en.W / 2);
    const int64_t chunk = (EH + world - 1) / world;
    int rc = use_device(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    shard_release(ctx);
    // (DevBuf::reserve keeps the contents only when it does not grow: the buffers hold nothing between runs)
    const mtg_ctx::Ensembles::Sizes z = en.sizes();
    HIP_TRY(ctx, en.new_lnp.reserve(std::max(z.new_lnp, (size_t)(chunk * world) * sizeof(double))));
    HIP_TRY(ctx, en.st.reserve(std::max(z.st, (size_t)(chunk * world) * sizeof(int32_t))));
    en.shard.rank = rank; en.shard.world = world; en.shard.chunk = chunk;
    en.shard.lo = std::min<int64_t>((int64_t)rank * chunk, EH);
    en.shard.hi = std::min<int64_t>(en.shard.lo + chunk, EH);
    return MTG_OK;
}

// after the solve of a half-step: everybody's log-probabilities and status words into ens.new_lnp / ens.st
int shard_exchange(mtg_ctx *ctx, int64_t EH, hipStream_t s)
{
    double *lnp = ctx->ens.new_lnp.as<double>();
    int32_t *st = ctx->ens.st.as<int32_t>();
    const int64_t chunk = ctx->ens.shard.chunk, lo = ctx->ens.shard.lo, hi = ctx->ens.shard.hi;
    if (ctx->ens.shard.kind == 1) {
        mtg_trace::Range range("mtg:all-gather of the half-step's log-probabilities (RCCL)");
        // in place: this rank's block already sits at rank * chunk of the receive buffer
        const int64_t at = (int64_t)ctx->ens.shard.rank * chunk;
        const bool timed = ctx->ens.shard_ev_n < ctx->ens.shard_ev_cap;
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ens.shard_ev[2 * (size_t)ctx->ens.shard_ev_n], s));
        struct Stamp {  // the closing event, whatever way the block is left
            mtg_ctx *c; hipStream_t st; bool on;
            ~Stamp() { if (on) { (void)hipEventRecord(c->ens.shard_ev[2 * (size_t)c->ens.shard_ev_n + 1], st); c->ens.shard_ev_n += 1; } }
        } stamp{ctx, s, timed};
        RCCL_TRY(ctx, g_rccl.GroupStart());
        int r1 = g_rccl.AllGather(lnp + at, lnp, (size_t)chunk, RCCL_FLOAT64, ctx->ens.shard.comm, s);
        int r2 = r1 ? r1 : g_rccl.AllGather(st + at, st, (size_t)chunk, RCCL_INT32, ctx->ens.shard.comm, s);
        const int r3 = g_rccl.GroupEnd();   // (always closed, whatever the calls inside it said)
        if (r2 || r3)
            return fail(ctx, MTG_E_HIP, "ncclAllGather of the half-step's log-probabilities failed: %s",
                        g_rccl.GetErrorString(r2 ? r2 : r3));
        return MTG_OK;
    }
    // host callback: stage this rank's rows, let the caller fill in the others, upload everything
    mtg_trace::Range range("mtg:exchange of the half-step's log-probabilities (host callback)");
    if (ctx->ens.shard.h_rows < EH) {
        if (ctx->ens.shard.h_lnp) (void)hipHostFree(ctx->ens.shard.h_lnp);
        if (ctx->ens.shard.h_st) (void)hipHostFree(ctx->ens.shard.h_st);
        ctx->ens.shard.h_lnp = nullptr; ctx->ens.shard.h_st = nullptr; ctx->ens.shard.h_rows = 0;
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->ens.shard.h_lnp, (size_t)EH * 8));
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->ens.shard.h_st, (size_t)EH * 4));
        ctx->ens.shard.h_rows = EH;
    }
    if (hi > lo) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ens.shard.h_lnp + lo, lnp + lo, (size_t)(hi - lo) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ens.shard.h_st + lo, st + lo, (size_t)(hi - lo) * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const int rc = ctx->ens.shard.fn(ctx->ens.shard.user, ctx->ens.shard.h_lnp, ctx->ens.shard.h_st, EH, lo, hi);
    if (rc) return fail(ctx, MTG_E_STATE, "the exchange callback of the walker-sharded ensemble returned %d", rc);
    HIP_TRY(ctx, hipMemcpyAsync(lnp, ctx->ens.shard.h_lnp, (size_t)EH * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(st, ctx->ens.shard.h_st, (size_t)EH * 4, hipMemcpyHostToDevice, s));
    return MTG_OK;
}

}  // namespace

MTG_API int mtg_rccl_load(const char *path)
{
    return rccl_load(path) ? MTG_OK : MTG_E_UNSUPPORTED;
}

MTG_API int mtg_rccl_unique_id(void *id128)
{
    if (!id128) return MTG_E_ARG;
    if (!rccl_load(nullptr)) return MTG_E_UNSUPPORTED;
    return g_rccl.GetUniqueId(id128) == 0 ? MTG_OK : MTG_E_HIP;
}

MTG_API int mtg_ensemble_shard_rccl(mtg_ctx *ctx, const void *id128, int rank, int world)
{
    if (!ctx || !id128) return MTG_E_ARG;
    if (!rccl_load(nullptr)) return fail(ctx, MTG_E_UNSUPPORTED, "%s", g_rccl.why.c_str());
    int rc = shard_layout(ctx, rank, world);
    if (rc) return rc;
    Id128 id;
    memcpy(id.b, id128, sizeof id.b);
    void *comm = nullptr;
    const int generation = ctx->ens.shard_generation.load();
    RCCL_TRY(ctx, g_rccl.CommInitRank(&comm, world, id, rank));
    if (ctx->ens.shard_generation.load() != generation) {
        // ncclCommInitRank took so long that the caller gave up and (un)sharded the context another way meanwhile
        // (distributed.shard_device_ensemble's fall-back to the host-staged exchange): this communicator is nobody's
        (void)g_rccl.CommDestroy(comm);
        return fail(ctx, MTG_E_STATE, "mtg_ensemble_shard_rccl: the context was re-sharded while ncclCommInitRank was running");
    }
    ctx->ens.shard.comm = comm;
    ctx->ens.shard.kind = 1;
    return MTG_OK;
}

MTG_API int mtg_ensemble_shard_host(mtg_ctx *ctx, int rank, int world, mtg_exchange_fn fn, void *user)
{
    if (!ctx || !fn) return MTG_E_ARG;
    int rc = shard_layout(ctx, rank, world);
    if (rc) return rc;
    ctx->ens.shard.fn = fn;
    ctx->ens.shard.user = user;
    ctx->ens.shard.kind = 2;
    return MTG_OK;
}

MTG_API int mtg_ensemble_shard_info(const mtg_ctx *ctx, int *kind, int *rank, int *world, int *comm_ranks)
{
    if (!ctx) return MTG_E_ARG;
    if (kind) *kind = ctx->ens.shard.kind;
    if (rank) *rank = ctx->ens.shard.rank;
    if (world) *world = ctx->ens.shard.world;
    if (comm_ranks) {
        *comm_ranks = 0;
        if (ctx->ens.shard.kind == 1 && ctx->ens.shard.comm && g_rccl.CommCount) (void)g_rccl.CommCount(ctx->ens.shard.comm, comm_ranks);
    }
    return MTG_OK;
}

MTG_API int mtg_ensemble_shard_profile(mtg_ctx *ctx, int capacity)
{
    if (!ctx || capacity < 0) return MTG_E_ARG;
    int rc = use_device(ctx);
    if (rc) return rc;
    while ((int)ctx->ens.shard_ev.size() < 2 * capacity) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->ens.shard_ev.push_back(e);
    }
    ctx->ens.shard_ev_cap = capacity;
    ctx->ens.shard_ev_n = 0;
    return MTG_OK;
}

MTG_API int mtg_ensemble_shard_profile_read(mtg_ctx *ctx, int capacity, double *exchange_ms)
{
    if (!ctx || capacity < 0) return MTG_E_ARG;
    const int n = ctx->ens.shard_ev_n < capacity ? ctx->ens.shard_ev_n : capacity;
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        HIP_TRY(ctx, hipEventSynchronize(ctx->ens.shard_ev[2 * (size_t)i + 1]));
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ens.shard_ev[2 * (size_t)i], ctx->ens.shard_ev[2 * (size_t)i + 1]));
        if (exchange_ms) exchange_ms[i] = ms;
    }
    ctx->ens.shard_ev_cap = 0;
    return n;
}

MTG_API int mtg_ensemble_unshard(mtg_ctx *ctx)
{
    if (!ctx) return MTG_E_ARG;
    int rc = use_device(ctx);
    if (rc) return rc;
    if (ctx->stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    shard_release(ctx);
    return MTG_OK;
}

namespace {

// One mtg_ensemble_run in flight.  The entry runs the stages in order -- check (which plans the run:
// mtg_plan_ensemble_run), stage, then for every solve of the plan solve and launch as the schedule says
// (mtg_ensemble_step) -- and returns at the first that fails; the chain's way back to the caller is the entry's own end.
// Between two solves ONE launch does the accept step of the solve just made and the proposals (with their expansion) of
// the next: mtg_sampler_step_kernel, or mtg_sampler_spec_kernel for a speculative iteration.  The structure lists have
// two banks: the proposals of solve k + 1 are appended to one while workgroup 0 clears the counters of the other, which
// solve k has just used.
struct EnsembleRun {
    mtg_ctx *ctx;
    mtg_ctx::Ensembles &en;
    int steps;
    double *chain, *lnp_chain;
    hipStream_t s = nullptr;
    int64_t EW = 0;
    uint32_t iteration0 = 0;       // of the ensembles when the run began
    MtgEnsembleRunPlan plan{};
    MtgEnsembleArgs g{};
    int32_t *perm_all = nullptr;   // plan.splits_up_front: [steps][E][W]

    int check();
    int stage();
    int solve(const MtgEnsembleStep &st);
    void launch(const MtgEnsembleStep &st);
};

int EnsembleRun::check()
{
    if (const int rc = check_ready(ctx, true)) return rc;
    if (en.E <= 0) return fail(ctx, MTG_E_STATE, "mtg_ensemble_init has not been called");
    if (steps < 0) return fail(ctx, MTG_E_ARG, "mtg_ensemble_run: negative step count");
    if (en.P != ctx->model.P) return fail(ctx, MTG_E_STATE, "the model changed since mtg_ensemble_init");
    if (en.L != ctx->L || en.N != ctx->N)
        return fail(ctx, MTG_E_STATE, "the resident light curves changed shape since mtg_ensemble_init");
    if (const int rc = use_device(ctx)) return rc;
    CTX_STREAM(ctx, own);
    s = own;
    EW = en.E * en.W;
    iteration0 = en.iteration;
    // (a profile mean runs on the serial sweep alone: nothing to speculate for)
    plan = mtg_plan_ensemble_run(en.E, en.W, steps, mtg_mean_is_profile(ctx->model.mean_kind) ? 0 : ctx->tp_mode, ctx->spec_mode, ctx->model.nr0 + 2 * ctx->model.nc0, ctx->N,
                                 en.shard.kind, en.shard.lo, en.shard.hi);
    return MTG_OK;
}

// room for the chain and the plan's solves, both banks' counters cleared, the splits where the plan makes them up front
int EnsembleRun::stage()
{
    if (chain) HIP_TRY(ctx, en.chain.reserve((size_t)steps * en.sizes().coords));
    if (lnp_chain) HIP_TRY(ctx, en.lnp_chain.reserve((size_t)steps * en.sizes().lnp));
    if (const int rc = check_model_workspace(ctx, plan.rows_per_solve)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->counts.p, 0, 2 * 64 * sizeof(int), s));
    g.E = (int)en.E; g.W = en.W; g.P = en.P;
    g.e_base = (uint32_t)en.base; g.seed_lo = (uint32_t)en.seed; g.seed_hi = (uint32_t)(en.seed >> 32); g.a = 2.0;
    g.perm = en.perm.as<int32_t>(); g.coords = en.coords.as<double>(); g.lnp = en.lnp.as<double>();
    g.factor = en.factor.as<double>(); g.naccept = en.naccept.as<int32_t>(); g.n_notpd = en.notpd.as<int32_t>();
    g.best_lnp = en.best_lnp.as<double>(); g.best_coords = en.best_coords.as<double>();
    if (plan.splits_up_front) {
        HIP_TRY(ctx, en.perm_all.reserve(plan.perm_bytes));
        perm_all = en.perm_all.as<int32_t>();
        mtg_launch_split_all(g, iteration0, steps, perm_all, s);
    }
    return MTG_OK;
}

// the proposals in the bank the last launch filled; sharded: then everybody's log-probabilities and status words
int EnsembleRun::solve(const MtgEnsembleStep &st)
{
    ctx->bank = st.bank_used;
    const int rc = solve_prepared(ctx, plan.rows_per_solve, en.lc_spec.as<int32_t>(), en.new_lnp.as<double>(), en.st.as<int32_t>(), s);
    return rc || !en.shard.kind ? rc : shard_exchange(ctx, plan.rows_per_solve, s);
}

void EnsembleRun::launch(const MtgEnsembleStep &st)
{
    g.perm = st.perm >= 0 ? perm_all + st.perm * EW : en.perm.as<int32_t>();
    g.perm_next = st.perm_next >= 0 ? perm_all + st.perm_next * EW : nullptr;
    MtgSamplerLaunch l;
    l.do_accept = st.do_accept; l.half = st.half; l.iteration = st.iteration;
    l.do_propose = st.do_propose; l.next_half = st.next_half; l.next_iteration = st.next_iteration;
    if (st.do_accept) {
        ctx->bank = st.bank_used;
        l.new_lnp = en.new_lnp.as<double>(); l.status = en.st.as<int32_t>(); l.clear_counts = bank_counts(ctx);
    }
    if (st.chain_row >= 0 && chain) l.chain_row = en.chain.as<double>() + st.chain_row * EW * en.P;
    if (st.chain_row >= 0 && lnp_chain) l.lnp_chain_row = en.lnp_chain.as<double>() + st.chain_row * EW;
    ctx->bank = st.bank_next;
    MtgPrepArgs pa = make_prep_args(ctx, plan.rows_per_solve, en.q.as<double>(), 1, en.new_lnp.as<double>(), en.st.as<int32_t>(),
                                    ctx->model.nsho + 1);
    if (en.shard.kind) { pa.row_lo = en.shard.lo; pa.row_hi = en.shard.hi; }
    (plan.speculative ? mtg_launch_sampler_spec : mtg_launch_sampler_step)(g, l, pa, s);
    en.iteration = st.next_iteration;
}

// mtg_ensemble_get / mtg_ensemble_restore: the state a caller may read or put back as (host pointer, buffer, bytes),
// copied to the host or from it -- NULL host pointers skipped -- and the stream waited for
int ens_copy_state(mtg_ctx *ctx, hipMemcpyKind kind, const double *coords, const double *lnp, const double *best_lnp,
                   const double *best_coords, const int32_t *naccept, const int32_t *n_notpd)
{
    if (const int rc = use_device(ctx)) return rc;
    CTX_STREAM(ctx, s);
    mtg_ctx::Ensembles &en = ctx->ens;
    const mtg_ctx::Ensembles::Sizes z = en.sizes();
    const struct { const void *host; DevBuf &buf; size_t bytes; } state[] = {
        {coords, en.coords, z.coords}, {lnp, en.lnp, z.lnp}, {best_lnp, en.best_lnp, z.best_lnp},
        {best_coords, en.best_coords, z.best_coords}, {naccept, en.naccept, z.naccept}, {n_notpd, en.notpd, z.notpd}};
    for (const auto &r : state) {
        if (!r.host) continue;
        if (kind == hipMemcpyHostToDevice) HIP_TRY(ctx, hipMemcpyAsync(r.buf.p, r.host, r.bytes, kind, s));
        else HIP_TRY(ctx, hipMemcpyAsync(const_cast<void *>(r.host), r.buf.p, r.bytes, kind, s));   // (mtg_ensemble_get's own pointers)
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return MTG_OK;
}

}  // namespace

MTG_API int mtg_ensemble_run(mtg_ctx *ctx, int steps, double *chain, double *lnp_chain)
{
    if (!ctx) return MTG_E_ARG;
    EnsembleRun r{ctx, ctx->ens, steps, chain, lnp_chain};
    int rc = r.check();
    if (rc) return rc;
    mtg_trace::Range range("mtg:ensemble_run (stretch moves, device resident)");
    struct BankGuard { mtg_ctx *c; ~BankGuard() { c->bank = 0; } } bank_guard{ctx};   // everybody else uses bank 0
    struct LiveRows { mtg_ctx *c; ~LiveRows() { c->live_rows = 0; } } live_rows{ctx};
    ctx->live_rows = r.plan.live_rows;   // the solver's kernel choice looks at the rows this rank evaluates
    if ((rc = r.stage())) return rc;
    if (r.plan.solves > 0) r.launch(mtg_ensemble_step(r.plan, -1, steps, r.iteration0));   // the first proposals of the run
    for (int64_t k = 0; k < r.plan.solves; ++k) {
        const MtgEnsembleStep st = mtg_ensemble_step(r.plan, k, steps, r.iteration0);
        if ((rc = r.solve(st))) return rc;
        r.launch(st);
    }
    HIP_TRY(ctx, hipGetLastError());
    const mtg_ctx::Ensembles::Sizes z = ctx->ens.sizes();
    if (chain) HIP_TRY(ctx, hipMemcpyAsync(chain, ctx->ens.chain.p, (size_t)steps * z.coords, hipMemcpyDeviceToHost, r.s));
    if (lnp_chain) HIP_TRY(ctx, hipMemcpyAsync(lnp_chain, ctx->ens.lnp_chain.p, (size_t)steps * z.lnp, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(ctx, hipStreamSynchronize(r.s));
    return MTG_OK;
}

MTG_API int mtg_ensemble_restore(mtg_ctx *ctx, int64_t iteration, const double *lnp, const int32_t *naccept,
                                 const double *best_lnp, const double *best_coords)
{
    if (!ctx) return MTG_E_ARG;
    if (ctx->ens.E <= 0) return fail(ctx, MTG_E_STATE, "mtg_ensemble_init has not been called");
    if (iteration < 0 || iteration > 0xffffffffll) return fail(ctx, MTG_E_ARG, "mtg_ensemble_restore: iteration out of range");
    // the saved log-probabilities as they are: mtg_ensemble_init has just evaluated the saved coordinates again, but
    // in ONE batch of E W rows, where the run evaluated them in half-steps of E W/2 (or a rank's share of them) -- the
    // kernel and its summation order follow the row count, so those values may differ in the last bits and flip an
    // accept decision of the continued chain
    const int rc = ens_copy_state(ctx, hipMemcpyHostToDevice, nullptr, lnp, best_lnp, best_coords, naccept, nullptr);
    if (rc == MTG_OK) ctx->ens.iteration = (uint32_t)iteration;
    return rc;
}

MTG_API int mtg_ensemble_get(mtg_ctx *ctx, double *coords, double *lnp, double *best_lnp, double *best_coords,
                             int32_t *naccept, int64_t *iteration, int32_t *n_notpd)
{
    if (!ctx) return MTG_E_ARG;
    if (ctx->ens.E <= 0) return fail(ctx, MTG_E_STATE, "mtg_ensemble_init has not been called");
    const int rc = ens_copy_state(ctx, hipMemcpyDeviceToHost, coords, lnp, best_lnp, best_coords, naccept, n_notpd);
    if (rc == MTG_OK && iteration) *iteration = ctx->ens.iteration;
    return rc;
}

MTG_API int mtg_fft_warmup(mtg_ctx *ctx)
{
    // HIP's current device is per THREAD: a helper thread starts on device 0 whatever the context's is
    if (ctx && hipSetDevice(ctx->device) != hipSuccess) return MTG_E_HIP;
    // hipFFT needs ~1.4 s the first time a plan is made in a process (rocFFT loads its kernels): callers that will
    // need mtg_chain_autocorr or mtg_simulate_tk95 later can pay that early, from another thread
    FftPlan plan;
    return plan.get({HIPFFT_D2Z, 64, 1}) ? MTG_OK : MTG_E_HIP;
}

MTG_API int mtg_chain_autocorr(mtg_ctx *ctx, int64_t n_t, int64_t E, int W, int P, const double *chain, double *rho)
{
    if (!ctx) return MTG_E_ARG;
    if (n_t < 2 || E < 1 || W < 1 || P < 1 || !chain || !rho) return fail(ctx, MTG_E_ARG, "mtg_chain_autocorr: bad arguments");
    int64_t n = 1;
    while (n < n_t) n *= 2;
    const int64_t n2 = 2 * n, nk = n + 1, S = E * (int64_t)W * P, EP = E * P;
    if (n2 > ((int64_t)1 << 30) || S > ((int64_t)1 << 24) || n2 * S > ((int64_t)1 << 32))
        return fail(ctx, MTG_E_ARG, "mtg_chain_autocorr: chain too large");
    int rc = use_device(ctx);
    if (rc) return rc;
    CTX_STREAM(ctx, s);
    mtg_trace::Range range("mtg:chain_autocorr (convergence check)");
    DevBuf &d_chain = ctx->acf_chain, &d_x = ctx->acf_x, &d_f = ctx->acf_f, &d_g = ctx->acf_g, &d_r = ctx->acf_r, &d_ss = ctx->acf_ss;
    HIP_TRY(ctx, d_chain.reserve((size_t)n2 * S * 8));        // the chain, then the transposed series [S][n2]
    HIP_TRY(ctx, d_x.reserve((size_t)n2 * S * 8));            // centred and padded, [n2][S]
    HIP_TRY(ctx, d_f.reserve((size_t)nk * S * 16));
    HIP_TRY(ctx, d_g.reserve((size_t)nk * EP * 16));
    HIP_TRY(ctx, d_r.reserve((size_t)(n2 + n_t) * EP * 8));   // inverse transforms [EP][n2], then rho [n_t][EP]
    HIP_TRY(ctx, d_ss.reserve((size_t)S * 8));
    HIP_TRY(ctx, ctx->acf_tmp.reserve((size_t)((n2 / 256 + 2) * S) * 8));
    HIP_TRY(ctx, hipMemcpyAsync(d_chain.p, chain, (size_t)n_t * S * 8, hipMemcpyHostToDevice, s));
    mtg_launch_acf_center(n_t, n2, S, d_chain.as<double>(), d_x.as<double>(), d_ss.as<double>(), ctx->acf_tmp.as<double>(), s);
    mtg_launch_acf_transpose(n2, S, d_x.as<double>(), d_chain.as<double>(), s);
    // contiguous batched transforms (stock kernels: no run-time compilation inside rocFFT)
    MtgAcfSlot held[MTG_ACF_SLOTS];
    for (int i = 0; i < MTG_ACF_SLOTS; ++i) {
        const FftKey *kf = ctx->acf_slots[i].fwd.held(), *ki = ctx->acf_slots[i].inv.held();
        held[i] = kf && ki ? MtgAcfSlot{true, kf->len, kf->batch, ki->batch, ctx->acf_slots[i].used} : MtgAcfSlot{};
    }
    bool hit = false;
    mtg_ctx::AcfPlans &slot = ctx->acf_slots[mtg_acf_slot_choose(held, n2, S, EP, &hit)];
    hipfftHandle fwd = 0, inv = 0;
    const int bad = fft_pair_get(slot.fwd, {HIPFFT_D2Z, n2, (int)S, n2, nk}, slot.inv, {HIPFFT_Z2D, n2, (int)EP, nk, n2}, &fwd, &inv);
    if (bad) return fail(ctx, MTG_E_HIP, "mtg_chain_autocorr: hipfftPlanMany (%s) failed", bad == 1 ? "forward" : "inverse");
    if (!hit) {   // a pair made now: counted, and bound to the context's stream once
        ctx->acf_plans_built += 1;
        if (hipfftSetStream(fwd, s) != HIPFFT_SUCCESS || hipfftSetStream(inv, s) != HIPFFT_SUCCESS)
            return fail(ctx, MTG_E_HIP, "mtg_chain_autocorr: hipfftSetStream failed");
    }
    slot.used = ++ctx->acf_clock;
    if (hipfftExecD2Z(fwd, d_chain.as<double>(), (hipfftDoubleComplex *)d_f.p) != HIPFFT_SUCCESS)
        return fail(ctx, MTG_E_HIP, "mtg_chain_autocorr: hipfftExecD2Z failed");
    mtg_launch_acf_power(nk, E, W, P, d_f.as<double2>(), d_ss.as<double>(), d_g.as<double2>(), s);
    if (hipfftExecZ2D(inv, (hipfftDoubleComplex *)d_g.p, d_r.as<double>()) != HIPFFT_SUCCESS)
        return fail(ctx, MTG_E_HIP, "mtg_chain_autocorr: hipfftExecZ2D failed");
    double *d_rho = d_r.as<double>() + n2 * EP;
    mtg_launch_acf_out(n_t, n2, EP, 1.0 / (double)n2, d_r.as<double>(), d_rho, s);   // hipFFT does not normalise
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(rho, d_rho, (size_t)n_t * EP * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return MTG_OK;
}

// ---- the TK95 simulator: how a call is cut and which cached plan serves it is mtg_sim_plan.h's to say ----
static MtgSimLayout sim_layout(const mtg_ctx *ctx, int64_t nfft, int64_t S)
{
    const char *env = mtg_measure_env("MTG_SIM_BATCH");   // MTG_MEASURE builds only
    return mtg_sim_layout(nfft, S, ctx->sim_transform, ctx->czt.pairs_on, env ? atoi(env) : 0);
}

// the context's cached plan for a layout -- the Z2D plan of length nfft, or the chirp-z path's Z2Z plan of length m --
// made, or remade for another length or batch, under sim_mu; 0 when hipFFT refuses.  No fail(): may run on a helper thread
static hipfftHandle sim_plan_get(mtg_ctx *ctx, int64_t nfft, const MtgSimLayout &cut)
{
    std::lock_guard<std::mutex> lock(ctx->sim_mu);
    return cut.czt ? ctx->czt.plans[cut.slot].get({HIPFFT_Z2Z, cut.m, cut.batch})
                   : ctx->sim_plans[cut.slot].get({HIPFFT_Z2D, nfft, cut.batch});
}

// chirp and transformed wrapped chirp of length nfft (mtg_simulate.hip), made on `s` the first time a length is used
static int czt_tables_get(mtg_ctx *ctx, int64_t nfft, hipStream_t s)
{
    mtg_ctx::SimCzt &z = ctx->czt;
    const int64_t m = mtg_czt_length(nfft);
    if (z.tables && z.nfft == nfft) return MTG_OK;
    z.tables = false;
    if (z.chirp.reserve_n<double2>(nfft) != hipSuccess || z.bhat.reserve_n<double2>(m) != hipSuccess) return MTG_E_HIP;
    mtg_launch_czt_tables(nfft, m, z.chirp.as<double2>(), z.bhat.as<double2>(), s);
    FftPlan one;   // (the plan and its own work area go at the return: after the synchronisation, where it ran)
    const hipfftHandle h = one.get({HIPFFT_Z2Z, m, 1});
    if (!h || hipfftSetStream(h, s) != HIPFFT_SUCCESS ||
        hipfftExecZ2Z(h, (hipfftDoubleComplex *)z.bhat.p, (hipfftDoubleComplex *)z.bhat.p, HIPFFT_FORWARD) != HIPFFT_SUCCESS ||
        hipStreamSynchronize(s) != hipSuccess)
        return MTG_E_HIP;
    z.tables = true;
    z.nfft = nfft;
    z.m = m;
    return MTG_OK;
}

MTG_API int mtg_simulate_plan(mtg_ctx *ctx, int64_t nfft)
{
    if (!ctx || nfft < 4 || nfft > ((int64_t)1 << 30)) return MTG_E_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return MTG_E_HIP;   // (HIP's current device is per thread)
    // the bulk plan: of the power-of-two transforms for a chirp-z length (milliseconds; the tables at first use)
    return sim_plan_get(ctx, nfft, sim_layout(ctx, nfft, INT64_MAX)) ? MTG_OK : MTG_E_HIP;
}

// The E13 flux-PDF adjustment (mtg_e13.hip) of the `sc` segments e13.seg[sc][n] of one simulation chunk (global indices
// s0 .. s0 + sc): on return e13.x[sc][n] holds the adjusted series.  `chunk` = the batch of the plans (sc <= chunk).
static int e13_adjust_chunk(mtg_ctx *ctx, int64_t sc, int64_t chunk, int64_t s0, int64_t n, double mean_rate, uint64_t seed, hipStream_t s)
{
    mtg_ctx::E13 &E = ctx->e13;
    const int64_t nk = n / 2 + 1;
    if (chunk * n >= ((int64_t)1 << 31)) return fail(ctx, MTG_E_ARG, "E13 adjustment: %lld segments of %lld samples per chunk exceed 2^31 elements", (long long)chunk, (long long)n);
    const size_t temp_bytes = mtg_e13_sort_temp_bytes(chunk, n);
    HIP_TRY(ctx, E.x.reserve((size_t)chunk * n * 8));
    HIP_TRY(ctx, E.fresh.reserve((size_t)chunk * n * 8));
    HIP_TRY(ctx, E.values.reserve((size_t)chunk * n * 8));
    HIP_TRY(ctx, E.adj.reserve((size_t)chunk * n * 8));
    HIP_TRY(ctx, E.keys.reserve((size_t)chunk * n * 8));
    HIP_TRY(ctx, E.amp.reserve((size_t)chunk * nk * 8));
    HIP_TRY(ctx, E.spec.reserve((size_t)chunk * nk * 16));
    HIP_TRY(ctx, E.idx.reserve((size_t)chunk * n * 4));
    HIP_TRY(ctx, E.order.reserve((size_t)chunk * n * 4));
    HIP_TRY(ctx, E.order_tmp.reserve((size_t)chunk * n * 4));
    HIP_TRY(ctx, E.segment.reserve((size_t)chunk * n * 4));
    HIP_TRY(ctx, E.segment_out.reserve((size_t)chunk * n * 4));
    HIP_TRY(ctx, E.flags.reserve((size_t)(2 * chunk + 1) * 4));
    HIP_TRY(ctx, E.stdv.reserve((size_t)chunk * 8));
    HIP_TRY(ctx, E.temp.reserve(temp_bytes > 0 ? temp_bytes : 16));
    hipfftHandle fwd = 0, inv = 0;
    const int bad = fft_pair_get(E.fwd, {HIPFFT_D2Z, n, (int)chunk, n, nk}, E.inv, {HIPFFT_Z2D, n, (int)chunk, nk, n}, &fwd, &inv);
    if (bad)
        return fail(ctx, MTG_E_HIP, "E13 adjustment: hipfftPlanMany (%s, n = %lld, batch = %lld) failed", bad == 1 ? "forward" : "inverse",
                    (long long)n, (long long)chunk);
    if (hipfftSetStream(fwd, s) != HIPFFT_SUCCESS || hipfftSetStream(inv, s) != HIPFFT_SUCCESS)
        return fail(ctx, MTG_E_HIP, "E13 adjustment: hipfftSetStream failed");
    double *seg = E.seg.as<double>(), *x = E.x.as<double>(), *fresh = E.fresh.as<double>(), *values = E.values.as<double>();
    double *adj = E.adj.as<double>(), *keys = E.keys.as<double>(), *amp = E.amp.as<double>();
    double2 *spec = E.spec.as<double2>();
    int32_t *idx = E.idx.as<int32_t>(), *order = E.order.as<int32_t>(), *order_tmp = E.order_tmp.as<int32_t>();
    uint32_t *segment = E.segment.as<uint32_t>(), *segment_out = E.segment_out.as<uint32_t>();
    int32_t *done = E.flags.as<int32_t>(), *notconv = done + chunk, *running = done + 2 * chunk;
    HIP_TRY(ctx, hipMemsetAsync(E.flags.p, 0, (size_t)(2 * chunk + 1) * 4, s));
    if (sc < chunk) {   // the plans transform `chunk` slots: the unused ones hold zeros
        HIP_TRY(ctx, hipMemsetAsync(seg + sc * n, 0, (size_t)(chunk - sc) * n * 8, s));
        HIP_TRY(ctx, hipMemsetAsync(x + sc * n, 0, (size_t)(chunk - sc) * n * 8, s));
    }
    mtg_launch_e13_iota(sc, n, idx, done, s);
    // the target: amplitudes of the TK95 segment; the white series and its sorted values
    if (hipfftExecD2Z(fwd, seg, (hipfftDoubleComplex *)spec) != HIPFFT_SUCCESS) return fail(ctx, MTG_E_HIP, "E13 adjustment: hipfftExecD2Z failed");
    mtg_launch_e13_abs(sc * nk, spec, amp, s);
    if (E.given_S) {
        const int64_t gS = E.given_S, gn = E.given_n;
        if (gn != n || s0 + sc > gS) return fail(ctx, MTG_E_ARG, "E13 adjustment: the draws of mtg_set_simulate_pdf_draws are [%lld][%lld], this call needs series %lld..%lld of %lld samples",
                                                  (long long)gS, (long long)gn, (long long)s0, (long long)(s0 + sc), (long long)n);
        HIP_TRY(ctx, hipMemcpyAsync(x, E.given.as<double>() + s0 * n, (size_t)sc * n * 8, hipMemcpyDeviceToDevice, s));
    } else {
        mtg_launch_e13_std(sc, n, seg, E.stdv.as<double>(), s);
        mtg_launch_e13_draw(sc, s0, ctx->stream_base, n, E.kind, mean_rate, E.stdv.as<double>(), seed, x, s);
    }
    HIP_TRY(ctx, mtg_launch_e13_sort_values(sc, n, x, keys, idx, order_tmp, segment, segment_out, order, values, E.temp.p, temp_bytes, s));
    HIP_TRY(ctx, hipGetLastError());
    int it = 0;
    int32_t still = (int32_t)sc;
    for (; it <= E.max_iter && still > 0; ++it) {
        if (hipfftExecD2Z(fwd, x, (hipfftDoubleComplex *)spec) != HIPFFT_SUCCESS) return fail(ctx, MTG_E_HIP, "E13 adjustment: hipfftExecD2Z failed");
        mtg_launch_e13_phase(sc * nk, amp, spec, s);
        if (hipfftExecZ2D(inv, (hipfftDoubleComplex *)spec, adj) != HIPFFT_SUCCESS) return fail(ctx, MTG_E_HIP, "E13 adjustment: hipfftExecZ2D failed");
        HIP_TRY(ctx, mtg_launch_e13_rank(sc, n, adj, keys, idx, order_tmp, segment, segment_out, order, E.temp.p, temp_bytes, s));
        HIP_TRY(ctx, hipMemsetAsync(running, 0, 4, s));
        mtg_launch_e13_step(sc, n, order, values, x, fresh, done, notconv, running, s);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&still, running, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    if (it > E.iterations) E.iterations = it;
    E.not_converged += still;
    return MTG_OK;
}

namespace {

struct SimArgs {   // what mtg_simulate_tk95 is called with, in its order
    int64_t S; const double *theta, *psd_table; int64_t psd_rows; uint64_t seed; int64_t nfft; double sim_dt, mean_rate;
    int64_t seg_len; const int32_t *win_lo, *win_hi; int noise_kind; double sigma_noise; const double *exposures;
    double *clean, *rates, *dy, *lc_means, *segments; int make_resident;
};

// One mtg_simulate_tk95 in flight.  The entry runs the stages in order -- check, stage, make_plan, then transform and
// observe chunk by chunk, finish -- and returns at the first that fails; ~SimCall is the epilogue of every return.
struct SimCall : SimArgs {
    SimCall(const SimArgs &a, mtg_ctx *c) : SimArgs(a), ctx(c) {}
    mtg_ctx *ctx;
    hipStream_t s = nullptr;
    int64_t N = 0, nk = 0;
    int P = 0;
    MtgSimLayout cut{};
    hipfftHandle plan = 0;
    DevBuf d_lo, d_hi, d_expo, d_clean, d_rates, d_dy, d_means, d_psd, d_seg, yv_tmp;
    MtgTk95Spectrum spectrum;   // the launchers' arguments: the call's part filled by check() and stage(), the chunk's as it comes
    MtgTk95Segment segment;
    MtgTk95Observe observed;
    const char *what = "allocation";   // the stage a HIP error is reported under
    bool entered = false;              // the checks passed: the draws handed in for this call are consumed
    bool armed = false;                // staging has begun: a failure now may leave the resident set freed or half written
    bool done = false;

    int check();
    int stage();
    int make_plan();
    int transform(int64_t s0, int64_t sc);
    int observe(int64_t s0, int64_t sc);
    int finish();
    ~SimCall();
};

#define SIM_TRY(call)                                                                                         \
    do {                                                                                                      \
        hipError_t e__ = (call);                                                                              \
        if (e__ != hipSuccess)                                                                                \
            return fail(ctx, MTG_E_HIP, "mtg_simulate_tk95 (%s): %s", what, hipGetErrorString(e__));          \
    } while (0)

// arguments and state; the draws handed in for this call
int SimCall::check()
{
    int rc = check_ready(ctx, psd_table == nullptr);   // a tabulated spectrum needs no model
    if (rc) return rc;
    if (psd_table && psd_rows != 1 && psd_rows != S)
        return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: psd_rows must be 1 or S");
    N = ctx->N;
    nk = nfft / 2 + 1;
    if (nfft > ((int64_t)1 << 30)) return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: nfft above 2^30");
    if (S <= 0 || nfft < 4 || !(sim_dt > 0.0) || seg_len <= 0 || seg_len > nfft || !win_lo || !win_hi || !rates || !dy ||
        (!psd_table && !theta && ctx->model.P > 0))
        return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: bad arguments");
    if (noise_kind < 0 || noise_kind > 3 || (noise_kind >= 2 && !exposures) || (noise_kind == 1 && !(sigma_noise >= 0.0)))
        return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: bad noise specification");
    if (noise_kind == 3 && ctx->kraft.N != N)
        return fail(ctx, MTG_E_STATE, "mtg_simulate_tk95: noise_kind 3 (Kraft) needs mtg_set_simulate_kraft for the %lld epochs of the resident sampling", (long long)N);
    if (noise_kind == 3) {
        MtgKraftTables &kraft = observed.kraft;
        kraft.bkg_counts = ctx->kraft.bkg.as<double>(); kraft.bkg_rate_err = ctx->kraft.err.as<double>();
        kraft.median = ctx->kraft.med.as<double>(); kraft.half = ctx->kraft.half.as<double>();
        kraft.K = ctx->kraft.K; kraft.threshold = ctx->kraft.threshold;
    }
    for (int64_t n = 0; n < N; ++n)
        if (win_lo[n] < 0 || win_hi[n] < win_lo[n] || win_hi[n] > seg_len)
            return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: window %lld = [%d, %d) outside the segment of %lld samples",
                        (long long)n, win_lo[n], win_hi[n], (long long)seg_len);
    if (make_resident && ctx->t_per_lc)
        return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: make_resident needs a shared sampling");
    // draws handed in for this call (consumed whatever happens next)
    const int64_t given_S = ctx->given.S, given_nk = ctx->given.nk;
    ctx->given.S = 0;
    if (given_S && (given_S != S || given_nk != nk))
        return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: the draws of mtg_set_simulate_draws are for %lld series of %lld frequencies, "
                    "this call simulates %lld of %lld", (long long)given_S, (long long)given_nk, (long long)S, (long long)nk);
    for (int64_t i = 0; i < given_S; ++i)  // a start is an index into the series: the kernels do not check it
        if (ctx->given.starts_host[i] + seg_len > nfft)
            return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: given start %lld + segment %lld beyond the series of %lld samples",
                        (long long)ctx->given.starts_host[i], (long long)seg_len, (long long)nfft);
    spectrum.given = given_S ? ctx->given.normals.as<double>() : nullptr;
    segment.given_start = observed.given_start = given_S ? ctx->given.starts.as<int64_t>() : nullptr;
    rc = use_device(ctx);
    if (rc) return rc;
    entered = true;   // (the E13 draws too are consumed from here on; the report starts afresh)
    ctx->e13.iterations = 0;
    ctx->e13.not_converged = 0;
    if (ctx->e13.kind != 0 && !(mean_rate > 0.0) && ctx->e13.kind == 1)
        return fail(ctx, MTG_E_ARG, "mtg_simulate_tk95: a lognormal flux PDF needs a positive mean rate");
    return MTG_OK;
}

// the layout of the call; allocations, uploads and the model's expansion; the launchers' arguments that every chunk shares
int SimCall::stage()
{
    MtgModel m0;
    memset(&m0, 0, sizeof m0);
    const MtgModel &m = psd_table ? m0 : ctx->model;
    P = m.P;
    const MtgCoefLayout lay{m.nr_max, m.nc_max};
    int rc = reserve_workspace(ctx, S, model_nslots(m) > 4 ? model_nslots(m) : 4, 1);   // (the expansion writes a profile mean's constants too; nothing here reads a mean)
    if (rc) return rc;
    CTX_STREAM(ctx, st);
    s = st;
    // the simulations go through the context's plan `chunk` at a time (the last group may be short: the transforms of
    // the unused slots run on zeros and are not looked at)
    cut = sim_layout(ctx, nfft, S);
    HIP_TRY(ctx, ctx->theta.reserve((size_t)S * (P > 0 ? P : 1) * 8));
    HIP_TRY(ctx, ctx->out.reserve((size_t)S * 8));
    HIP_TRY(ctx, ctx->status.reserve((size_t)S * 4));
    armed = true;
    const auto upload = [this](DevBuf &b, const void *src, size_t bytes) {
        const hipError_t e = b.reserve(bytes);
        return e != hipSuccess || !src ? e : hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s);
    };
    SIM_TRY(ctx->sim_spec.reserve((size_t)cut.spec_bytes));
    SIM_TRY(ctx->sim_series.reserve((size_t)cut.series_bytes));
    SIM_TRY(upload(d_lo, win_lo, (size_t)N * 4));
    SIM_TRY(upload(d_hi, win_hi, (size_t)N * 4));
    SIM_TRY(upload(d_expo, exposures, (size_t)N * 8));
    if (clean) SIM_TRY(d_clean.reserve_n<double>(S * N));
    SIM_TRY(d_rates.reserve_n<double>(S * N));
    SIM_TRY(d_dy.reserve_n<double>(S * N));
    SIM_TRY(d_means.reserve_n<double>(S));
    if (psd_table) SIM_TRY(upload(d_psd, psd_table, (size_t)psd_rows * nk * 8));
    if (segments) SIM_TRY(d_seg.reserve_n<double>(S * seg_len));
    if (P > 0) SIM_TRY(hipMemcpyAsync(ctx->theta.p, theta, (size_t)S * P * 8, hipMemcpyHostToDevice, s));
    if (!psd_table) {
        // theta -> celerite coefficients (no prior: the samples come from the posterior itself)
        mtg_launch_prepare(make_prep_args(ctx, S, ctx->theta.as<double>(), 0, ctx->out.as<double>(), ctx->status.as<int32_t>(), 1), s);
        SIM_TRY(hipGetLastError());
    }
    // irfft normalisation (hipFFT C2R is unnormalised) and the reference's power scaling
    const double scale = sqrt((double)nfft * sim_dt * sqrt(2.0 * M_PI)) / (double)nfft;
    spectrum.sbase = segment.sbase = observed.sbase = ctx->stream_base;
    spectrum.seed = segment.seed = observed.seed = seed;
    spectrum.nfft = nfft; spectrum.dt = sim_dt;
    spectrum.coef = ctx->coef.as<double>(); spectrum.cstride = ctx->cstride; spectrum.lay = lay; spectrum.nr0 = m.nr0; spectrum.nc0 = m.nc0;
    spectrum.sig = ctx->sig.as<int32_t>(); spectrum.psd_table = psd_table ? d_psd.as<double>() : nullptr; spectrum.psd_rows = psd_rows;
    spectrum.X = ctx->sim_spec.as<double2>();
    segment.nfft = nfft; segment.seg_len = seg_len; segment.dt = sim_dt; segment.scale = scale; segment.mean_rate = mean_rate;
    segment.series = ctx->sim_series.as<double>();
    observed.N = N; observed.seg_len = seg_len; observed.dt = sim_dt;
    observed.win_lo = d_lo.as<int32_t>(); observed.win_hi = d_hi.as<int32_t>();
    observed.noise_kind = noise_kind; observed.sigma_noise = sigma_noise; observed.exposures = d_expo.as<double>();
    observed.clean = clean ? d_clean.as<double>() : nullptr; observed.rates = d_rates.as<double>(); observed.dy = d_dy.as<double>();
    if (ctx->e13.kind != 0) {
        // the epochs are averaged from the ADJUSTED segments: start 0, no rescaling
        observed.nfft = seg_len; observed.scale = sim_dt; observed.mean_rate = 0.0; observed.fixed_start = 0; observed.given_start = nullptr;
    } else {
        observed.nfft = nfft; observed.scale = scale; observed.mean_rate = mean_rate; observed.series = ctx->sim_series.as<double>();
    }
    return MTG_OK;
}

// the cached plan of the layout, on the call's stream; for a chirp-z length its tables and work area
int SimCall::make_plan()
{
    const bool ready = !cut.czt || (czt_tables_get(ctx, nfft, s) == MTG_OK && ctx->czt.work.reserve((size_t)cut.work_bytes) == hipSuccess);
    plan = ready ? sim_plan_get(ctx, nfft, cut) : 0;
    if (!plan || hipfftSetStream(plan, s) != HIPFFT_SUCCESS)
        return fail(ctx, MTG_E_HIP, "mtg_simulate_tk95: hipFFT plan creation failed (nfft = %lld, batch = %lld)",
                    (long long)nfft, (long long)cut.chunk);
    return MTG_OK;
}

// series s0 .. s0 + sc: random spectra, then their inverse transforms into sim_series[sc][nfft]
int SimCall::transform(int64_t s0, int64_t sc)
{
    what = "simulation kernels";
    spectrum.S = sc; spectrum.s0 = s0;
    mtg_launch_tk95_spectrum(spectrum, s);
    double2 *spec = ctx->sim_spec.as<double2>();
    if (!cut.czt) {
        if (sc < cut.chunk)  // a short last group: the unused slots transform zeros
            SIM_TRY(hipMemsetAsync(spec + sc * nk, 0, (size_t)(cut.chunk - sc) * nk * 16, s));
        if (hipfftExecZ2D(plan, (hipfftDoubleComplex *)spec, ctx->sim_series.as<double>()) != HIPFFT_SUCCESS)
            return fail(ctx, MTG_E_HIP, "mtg_simulate_tk95: hipfftExecZ2D failed");
        return MTG_OK;
    }
    // pairs of series through two power-of-two complex transforms (a short last group packs zeros into the pairs it
    // does not fill: the plan's batch is fixed)
    const mtg_ctx::SimCzt &z = ctx->czt;
    double2 *work = z.work.as<double2>();
    hipfftDoubleComplex *w = (hipfftDoubleComplex *)work;
    mtg_launch_czt_pack(sc, cut.per, nfft, cut.m, spec, z.chirp.as<double2>(), work, s);
    const int64_t used = (sc + cut.per - 1) / cut.per;
    if (used < cut.batch) SIM_TRY(hipMemsetAsync(work + used * cut.m, 0, (size_t)(cut.batch - used) * cut.m * 16, s));
    if (hipfftExecZ2Z(plan, w, w, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return fail(ctx, MTG_E_HIP, "mtg_simulate_tk95: hipfftExecZ2Z failed");
    mtg_launch_czt_mul(used, cut.m, z.bhat.as<double2>(), work, s);
    if (hipfftExecZ2Z(plan, w, w, HIPFFT_BACKWARD) != HIPFFT_SUCCESS) return fail(ctx, MTG_E_HIP, "mtg_simulate_tk95: hipfftExecZ2Z failed");
    mtg_launch_czt_unpack(sc, cut.per, nfft, cut.m, work, z.chirp.as<double2>(), ctx->sim_series.as<double>(), s);
    return MTG_OK;
}

// series s0 .. s0 + sc at the epochs: cut, averaged over the windows, with noise -- for a non-Gaussian flux PDF
// (simulator.py:65-140) the cut segments as rates on the fine grid, adjusted on the device (mtg_e13.hip), then averaged
int SimCall::observe(int64_t s0, int64_t sc)
{
    segment.S = observed.S = sc;
    segment.s0 = observed.s0 = s0;
    if (ctx->e13.kind == 0) {
        mtg_launch_tk95_observe(observed, s);
        if (segments) {
            segment.out = d_seg.as<double>();
            mtg_launch_tk95_segment(segment, s);
        }
        SIM_TRY(hipGetLastError());
        return MTG_OK;
    }
    what = "E13 adjustment";
    SIM_TRY(ctx->e13.seg.reserve_n<double>(cut.chunk * seg_len));
    segment.out = ctx->e13.seg.as<double>();
    segment.out_first = s0;
    mtg_launch_tk95_segment(segment, s);
    if (segments)   // (what the caller asked for: the segments as the reference hands them to its adjustment)
        SIM_TRY(hipMemcpyAsync(d_seg.as<double>() + s0 * seg_len, ctx->e13.seg.p, (size_t)sc * seg_len * 8, hipMemcpyDeviceToDevice, s));
    const int rc = e13_adjust_chunk(ctx, sc, cut.chunk, s0, seg_len, mean_rate, seed, s);
    if (rc) return rc;
    observed.series = ctx->e13.x.as<double>();
    mtg_launch_tk95_observe(observed, s);
    SIM_TRY(hipGetLastError());
    return MTG_OK;
}

// the resident set and the means, the downloads
int SimCall::finish()
{
    if (make_resident || lc_means) {
        what = "resident set";
        DevBuf &target = make_resident ? ctx->yv : yv_tmp;  // without make_resident only the means are wanted
        SIM_TRY(target.reserve_n<double2>(S * N));
        mtg_launch_tk95_resident(S, N, d_rates.as<double>(), d_dy.as<double>(), target.as<double2>(), d_means.as<double>(), s);
        SIM_TRY(hipGetLastError());
        if (lc_means) SIM_TRY(hipMemcpyAsync(lc_means, d_means.p, (size_t)S * 8, hipMemcpyDeviceToHost, s));
    }
    if (clean) SIM_TRY(hipMemcpyAsync(clean, d_clean.p, (size_t)S * N * 8, hipMemcpyDeviceToHost, s));
    if (segments) SIM_TRY(hipMemcpyAsync(segments, d_seg.p, (size_t)S * seg_len * 8, hipMemcpyDeviceToHost, s));
    SIM_TRY(hipMemcpyAsync(rates, d_rates.p, (size_t)S * N * 8, hipMemcpyDeviceToHost, s));
    SIM_TRY(hipMemcpyAsync(dy, d_dy.p, (size_t)S * N * 8, hipMemcpyDeviceToHost, s));
    SIM_TRY(hipStreamSynchronize(s));
    if (make_resident) ctx->L = S;  // the simulated light curves replace the resident set (same sampling)
    done = true;
    return MTG_OK;
}

// The epilogue, on every return once the checks have passed.
SimCall::~SimCall()
{
    if (!entered) return;
    ctx->e13.given_S = 0;
    // the plan's buffers stay with the context for the next call of the workflow -- unless they are large enough to be
    // in somebody's way (a fine simulation grid: hundreds of MB per transform)
    DevBuf &spec = ctx->sim_spec, &series = ctx->sim_series, &work = ctx->czt.work;
    if (spec.cap + series.cap + work.cap > ((size_t)1 << 30)) { spec.release(); series.release(); work.release(); }
    // ... and so do the E13 adjustment's (92 bytes per fine sample and segment of a chunk; the flags and standard
    // deviations counted with them are (2 chunk + 1) 4 + chunk 8 bytes: nothing).  e13.given is the caller's, not scratch
    size_t held = 0;
    ctx->e13.each_scratch([&held](DevBuf &b) { held += b.cap; });
    if (held > ((size_t)1 << 30)) ctx->e13.each_scratch([](DevBuf &b) { b.release(); });
    // after a failure the resident set may have been freed or partly overwritten on the way: nothing is resident any more
    if (!done && armed && make_resident) { ctx->N = 0; ctx->L = 0; }
}

}  // namespace

MTG_API int mtg_simulate_tk95(mtg_ctx *ctx, int64_t S, const double *theta, const double *psd_table, int64_t psd_rows,
                              uint64_t seed, int64_t nfft, double sim_dt, double mean_rate, int64_t seg_len,
                              const int32_t *win_lo, const int32_t *win_hi, int noise_kind, double sigma_noise,
                              const double *exposures, double *clean, double *rates, double *dy, double *lc_means,
                              double *segments, int make_resident)
{
    SimCall c({S, theta, psd_table, psd_rows, seed, nfft, sim_dt, mean_rate, seg_len, win_lo, win_hi, noise_kind, sigma_noise,
               exposures, clean, rates, dy, lc_means, segments, make_resident}, ctx);
    int rc = c.check();
    if (rc) return rc;
    mtg_trace::Range range("mtg:simulate_tk95");
    if ((rc = c.stage()) || (rc = c.make_plan())) return rc;
    for (int64_t s0 = 0; s0 < S; s0 += c.cut.chunk) {
        const int64_t sc = s0 + c.cut.chunk <= S ? c.cut.chunk : S - s0;
        if ((rc = c.transform(s0, sc)) || (rc = c.observe(s0, sc))) return rc;
    }
    return c.finish();
}

MTG_API int mtg_tk95_observe_series(mtg_ctx *ctx, int64_t S, int64_t nfft, int64_t seg_len, int64_t start,
                                    const double *series, const int32_t *win_lo, const int32_t *win_hi, double *rates)
{
    int rc = check_ready(ctx, false);
    if (rc) return rc;
    const int64_t N = ctx->N;
    if (S <= 0 || nfft <= 0 || seg_len <= 0 || start < 0 || start + seg_len > nfft || !series || !win_lo || !win_hi || !rates)
        return fail(ctx, MTG_E_ARG, "mtg_tk95_observe_series: bad arguments");
    for (int64_t n = 0; n < N; ++n)
        if (win_lo[n] < 0 || win_hi[n] < win_lo[n] || win_hi[n] > seg_len)
            return fail(ctx, MTG_E_ARG, "mtg_tk95_observe_series: window %lld outside the segment", (long long)n);
    RowCall c{ctx, "mtg_tk95_observe_series", S, nullptr, nullptr, 0};   // (no rows of theta: the call's stream and its one way out)
    if ((rc = c.begin(false))) return rc;
    DevBuf d_series, d_lo, d_hi, d_rates, d_dy;
    c.reserve({{d_series, (size_t)S * nfft * 8}, {d_lo, (size_t)N * 4}, {d_hi, (size_t)N * 4}, {d_rates, (size_t)S * N * 8},
               {d_dy, (size_t)S * N * 8}});
    c.upload(d_series.p, series, (size_t)S * nfft * 8);
    c.upload(d_lo.p, win_lo, (size_t)N * 4);
    c.upload(d_hi.p, win_hi, (size_t)N * 4);
    c.then([&] {
        MtgTk95Observe oa;   // scale = dt = 1, mean 0, no noise: the plain window average of the series
        oa.N = N; oa.nfft = nfft; oa.seg_len = seg_len; oa.fixed_start = start;
        oa.win_lo = d_lo.as<int32_t>(); oa.win_hi = d_hi.as<int32_t>(); oa.rates = d_rates.as<double>(); oa.dy = d_dy.as<double>();
        oa.S = S; oa.series = d_series.as<double>();
        mtg_launch_tk95_observe(oa, c.s);
        return hipGetLastError();
    });
    c.gather(rates, d_rates.p, (size_t)S * N * 8);
    return c.finish(nullptr);
}

MTG_API int mtg_predict(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, double *mu,
                        double *var, int32_t *status)
{
    RowCall c{ctx, "mtg_predict", B, theta, lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (B <= 0 || !mu || !var || !status || (!theta && ctx->model.P > 0)) return c.bad_arguments();
    if ((rc = c.begin(true))) return rc;
    const int J = ctx->model.nr_max + 2 * ctx->model.nc_max, N = (int)ctx->N;
    const size_t out_bytes = (size_t)B * N * 8;
    MtgPredictArgs qa;
    c.stage_inputs();
    c.expand(qa);
    DevBuf work, d_mu, d_var;
    c.reserve({{work, (size_t)B * N * (3 * J + 2) * 8}, {d_mu, out_bytes}, {d_var, out_bytes}});
    c.then([&] {
        qa.work = work.as<double>(); qa.mu = d_mu.as<double>(); qa.var = d_var.as<double>();
        mtg_launch_predict(qa, c.s);
        return hipGetLastError();
    });
    c.gather(mu, d_mu.p, out_bytes);
    c.gather(var, d_var.p, out_bytes);
    return c.finish(status);
}

MTG_API int mtg_predict_at(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int64_t M,
                           const double *ts, double *mu, double *var, int32_t *status)
{
    RowCall c{ctx, "mtg_predict_at", B, theta, lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (B <= 0 || M <= 0 || !ts || !mu || !status || (!theta && ctx->model.P > 0)) return c.bad_arguments();
    if ((rc = c.begin(true))) return rc;
    bool ascending = true;
    for (int64_t m = 0; m < M; ++m) {
        if (!std::isfinite(ts[m])) return fail(ctx, MTG_E_ARG, "mtg_predict_at: ts[%lld] is not finite", (long long)m);
        if (m > 0 && ts[m] < ts[m - 1]) ascending = false;
    }
    // lanes of a wave take neighbouring times so that they replay the same stored samples: the times are visited in
    // ascending order and each result is stored where its time was given
    std::vector<int64_t> order;
    if (!ascending) {
        order.resize((size_t)M);
        for (int64_t m = 0; m < M; ++m) order[(size_t)m] = m;
        std::sort(order.begin(), order.end(), [ts](int64_t i, int64_t j) { return ts[i] < ts[j] || (ts[i] == ts[j] && i < j); });
    }
    const int J = ctx->model.nr0 + 2 * ctx->model.nc0;
    const int64_t N = ctx->N;
    if (J > MTG_MAX_J) return fail(ctx, MTG_E_UNSUPPORTED, "mtg_predict_at: rank %d > %d", J, MTG_MAX_J);
    const int64_t Bs = mtg_plan_predict_at_slab(N, J, M, B);
    if (Bs == 0) return fail(ctx, MTG_E_ARG, "mtg_predict_at: M = %lld is too large", (long long)M);
    const size_t ts_bytes = (size_t)M * 8;
    MtgPredictAtArgs qa;
    c.stage_inputs();
    c.expand(qa);
    PredictAtRoom room;
    room.reserve(c, qa, Bs, J, M, ts, ascending ? nullptr : order.data(), var != nullptr);
    if (c.ok()) c.e = for_each_slab(B, Bs, [&](int64_t row0, int64_t rows) {
        qa.row0 = row0; qa.B = rows;
        c.then([&] { return mtg_launch_predict_at(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        // (the copies are ordered on the stream: the next slab's kernels overwrite the buffers only after them)
        c.gather(mu + row0 * M, room.mu.p, (size_t)rows * ts_bytes);
        if (var) c.gather(var + row0 * M, room.var.p, (size_t)rows * ts_bytes);
        return c.e;
    });
    return c.finish(status);
}

MTG_API int mtg_predict_terms(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int T,
                              const uint32_t *term_mask, int64_t M, const double *ts, double *mu, double *var, int32_t *status)
{
    RowCall c{ctx, "mtg_predict_terms", B, theta, lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (B <= 0 || T < 1 || T > 32 || !term_mask || M <= 0 || !ts || !mu || !status || (!theta && ctx->model.P > 0))
        return c.bad_arguments();
    if ((rc = c.begin(true))) return rc;
    const uint32_t known = ((uint32_t)1 << ctx->model.nterms) - 1u;    // (nterms <= MTG_MAX_TERMS < 31)
    for (int k = 0; k < T; ++k)
        if (term_mask[k] & ~(known | MTG_TERMS_MEAN))
            return fail(ctx, MTG_E_ARG, "mtg_predict_terms: term_mask[%d] = 0x%x selects a term beyond the model's %d", k,
                        term_mask[k], ctx->model.nterms);
    bool ascending = true;
    for (int64_t m = 0; m < M; ++m) {
        if (!std::isfinite(ts[m])) return fail(ctx, MTG_E_ARG, "mtg_predict_terms: ts[%lld] is not finite", (long long)m);
        if (m > 0 && ts[m] < ts[m - 1]) ascending = false;
    }
    // the times in ascending order along a wave, each result stored where its time was given (as mtg_predict_at)
    std::vector<int64_t> order;
    if (!ascending) {
        order.resize((size_t)M);
        for (int64_t m = 0; m < M; ++m) order[(size_t)m] = m;
        std::sort(order.begin(), order.end(), [ts](int64_t i, int64_t j) { return ts[i] < ts[j] || (ts[i] == ts[j] && i < j); });
    }
    const int J = ctx->model.nr0 + 2 * ctx->model.nc0;
    const int64_t N = ctx->N;
    if (J > MTG_MAX_J) return fail(ctx, MTG_E_UNSUPPORTED, "mtg_predict_terms: rank %d > %d", J, MTG_MAX_J);
    // (a row's T M means and variances within the slab's budget)
    const int64_t Bs = mtg_plan_predict_at_slab(N, J, M, B, (size_t)T * (size_t)M * 16);
    if (Bs == 0) return fail(ctx, MTG_E_ARG, "mtg_predict_terms: M = %lld is too large", (long long)M);
    const size_t out_bytes = (size_t)T * (size_t)M * 8;
    MtgPredictTermsArgs qa;
    DevBuf owner, masks, d_mu, d_var;
    c.stage_inputs();
    c.expand(qa, &owner);
    PredictAtRoom room;
    room.reserve(c, qa, Bs, J, M, ts, ascending ? nullptr : order.data(), var != nullptr);
    c.reserve({{masks, (size_t)T * 4}, {d_mu, (size_t)Bs * out_bytes}, {d_var, var ? (size_t)Bs * out_bytes : 0}});
    c.upload(masks.p, term_mask, (size_t)T * 4);
    qa.T = T; qa.masks = masks.as<uint32_t>(); qa.owner = owner.as<int32_t>();
    qa.mu = d_mu.as<double>(); qa.var = var ? d_var.as<double>() : nullptr;
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_predict_terms_eval_kernel<%d>", J);
    if (c.ok()) c.e = for_each_slab(B, Bs, [&](int64_t row0, int64_t rows) {
        qa.row0 = row0; qa.B = rows;
        c.then([&] { return mtg_launch_predict_at_factor(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        c.then([&] { return mtg_launch_predict_terms_eval(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        // (the copies are ordered on the stream: the next slab's kernels overwrite the buffers only after them)
        c.gather(mu + row0 * T * M, d_mu.p, (size_t)rows * out_bytes);
        if (var) c.gather(var + row0 * T * M, d_var.p, (size_t)rows * out_bytes);
        return c.e;
    });
    return c.finish(status);
}

// what the periodogram entries refuse about the number of harmonics and of samples (MTG_OK: nothing): K harmonics with a
// floating mean fit 2 K + 1 samples exactly
static int ls_refuse_terms(mtg_ctx *ctx, const char *who, int nterms, int64_t N)
{
    if (nterms < 1 || nterms > MTG_LS_MAX_TERMS)
        return fail(ctx, MTG_E_ARG, "%s: nterms = %d is outside 1 .. %d", who, nterms, MTG_LS_MAX_TERMS);
    if (nterms == 1 && N < 4)
        return fail(ctx, MTG_E_ARG, "%s: N = %lld < 4 samples (a sinusoid with a floating mean fits three exactly)", who, (long long)N);
    if (N < 2 * nterms + 2)
        return fail(ctx, MTG_E_ARG, "%s: N = %lld < %d samples (%d harmonics with a floating mean fit %d exactly)", who, (long long)N,
                    2 * nterms + 2, nterms, 2 * nterms + 1);
    return MTG_OK;
}

// what both periodogram entries refuse about the frequencies, the normalization, the harmonics and the samples (MTG_OK:
// nothing), in the order of their messages; nothing_asked: mtg_lomb_scargle's three outputs are all NULL
static int ls_refuse_call(mtg_ctx *ctx, const char *who, int64_t F, const double *freqs, int nterms, int normalization, bool nothing_asked)
{
    int rc = refuse_no_freqs(ctx, who, F, freqs);
    if (rc) return rc;
    if (nothing_asked) return fail(ctx, MTG_E_ARG, "%s: power, peak_power and peak_index are all NULL", who);
    if ((rc = refuse_normalization(ctx, who, normalization)) || (rc = ls_refuse_terms(ctx, who, nterms, ctx->N))) return rc;
    return refuse_bad_freqs(ctx, who, F, freqs);
}

// the kernel that computes the powers, as mtg_last_solver names it
static void ls_kernel_name(char *out, size_t n, int nterms, int R)
{
    if (nterms == 1) snprintf(out, n, "mtg_lomb_scargle_kernel<%d>", R);
    else snprintf(out, n, "mtg_lomb_scargle_multi_kernel<%d,%d>", nterms, R);
}

// mtg_lomb_scargle (nterms = 1) and mtg_lomb_scargle_multi
static int lomb_scargle_entry(mtg_ctx *ctx, const char *who, int64_t F, const double *freqs, int nterms, int normalization, int weighted,
                              double *power, double *peak_power, int64_t *peak_index)
{
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    if ((rc = ls_refuse_call(ctx, who, F, freqs, nterms, normalization, !power && !peak_power && !peak_index))) return rc;
    if ((rc = c.begin())) return rc;
    const int64_t L = ctx->L;
    const int R = mtg_ls_tile(nterms, L, !ctx->t_per_lc, weighted);
    const int64_t Ls = mtg_ls_slab(F, R, L);
    DevBuf d_freqs, d_power;
    c.reserve({{d_freqs, (size_t)F * 8}, {d_power, (size_t)Ls * (size_t)F * 8}});
    const MtgLombScargleArgs qa = c.args(nterms, normalization, weighted, F, d_freqs.as<double>(), d_power.as<double>(), peak_power || peak_index);
    c.upload(d_freqs.p, freqs, (size_t)F * 8);
    ls_kernel_name(ctx->last_solver, sizeof ctx->last_solver, nterms, R);
    c.run_slabs(L, Ls, [&] { mtg_launch_lomb_scargle_stats(qa, c.s); },
                [&](int64_t l0, int64_t rows) { return mtg_launch_lomb_scargle(qa, l0, rows, c.s) ? hipGetLastError() : hipErrorInvalidValue; },
                [&](int64_t l0, int64_t rows) { if (power) c.gather(power + l0 * F, d_power.p, (size_t)rows * (size_t)F * 8); });
    c.gather_peaks(peak_power, peak_index);
    return c.finish();
}

MTG_API int mtg_lomb_scargle(mtg_ctx *ctx, int64_t F, const double *freqs, int normalization, int weighted, double *power,
                             double *peak_power, int64_t *peak_index)
{
    return lomb_scargle_entry(ctx, "mtg_lomb_scargle", F, freqs, 1, normalization, weighted, power, peak_power, peak_index);
}

MTG_API int mtg_lomb_scargle_multi(mtg_ctx *ctx, int64_t F, const double *freqs, int nterms, int normalization, int weighted,
                                   double *power, double *peak_power, int64_t *peak_index)
{
    return lomb_scargle_entry(ctx, "mtg_lomb_scargle_multi", F, freqs, nterms, normalization, weighted, power, peak_power, peak_index);
}

// what mtg_epoch_fold and mtg_phase_fold refuse, in the order of their messages (MTG_OK: nothing)
static int ef_refuse_call(mtg_ctx *ctx, const char *who, int64_t F, const double *freqs, int nbins, double time_0, int normalization,
                          bool nothing_asked)
{
    int rc = refuse_no_freqs(ctx, who, F, freqs);
    if (rc) return rc;
    if (nothing_asked) return fail(ctx, MTG_E_ARG, "%s: every output is NULL", who);
    if (nbins < 2 || nbins > MTG_EF_MAX_BINS) return fail(ctx, MTG_E_ARG, "%s: nbins = %d is outside 2 .. %d", who, nbins, MTG_EF_MAX_BINS);
    if (!std::isfinite(time_0)) return fail(ctx, MTG_E_ARG, "%s: time_0 = %g is not finite", who, time_0);
    if ((rc = refuse_normalization(ctx, who, normalization))) return rc;
    if (ctx->N < 2) return fail(ctx, MTG_E_ARG, "%s: N = %lld < 2 samples", who, (long long)ctx->N);
    return refuse_bad_freqs(ctx, who, F, freqs);
}

MTG_API int mtg_epoch_fold(mtg_ctx *ctx, int64_t F, const double *freqs, int nbins, double time_0, int normalization, int weighted,
                           double *power, double *peak_power, int64_t *peak_index)
{
    const char *who = "mtg_epoch_fold";
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    if ((rc = ef_refuse_call(ctx, who, F, freqs, nbins, time_0, normalization, !power && !peak_power && !peak_index))) return rc;
    if ((rc = c.begin())) return rc;
    const int64_t L = ctx->L;
    const MtgEfPlan plan = mtg_ef_plan(nbins, F, L, !ctx->t_per_lc, weighted ? 1 : 0);
    const int64_t Ls = mtg_ls_slab(F, plan.tile, L);
    DevBuf d_freqs, d_power;
    c.reserve({{d_freqs, (size_t)F * 8}, {d_power, (size_t)Ls * (size_t)F * 8}});
    MtgEpochFoldArgs qa;
    qa.ls = c.args(1, normalization, weighted, F, d_freqs.as<double>(), d_power.as<double>(), peak_power || peak_index);
    c.upload(d_freqs.p, freqs, (size_t)F * 8);
    qa.nbins = nbins; qa.time_0 = time_0;
    qa.wsum = qa.wrsum = qa.varsum = nullptr; qa.count = nullptr;
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_epoch_fold_kernel<%d,%d> lanes %d", plan.tile, weighted ? 1 : 0, plan.lanes);
    c.run_slabs(L, Ls, [&] { mtg_launch_lomb_scargle_stats(qa.ls, c.s); },
                [&](int64_t l0, int64_t rows) { return mtg_launch_epoch_fold(qa, plan, l0, rows, c.s); },
                [&](int64_t l0, int64_t rows) { if (power) c.gather(power + l0 * F, d_power.p, (size_t)rows * (size_t)F * 8); });
    c.gather_peaks(peak_power, peak_index);
    return c.finish();
}

MTG_API int mtg_phase_fold(mtg_ctx *ctx, int64_t F, const double *freqs, int nbins, double time_0, int weighted, int64_t *count,
                           double *wsum, double *wrsum, double *varsum)
{
    const char *who = "mtg_phase_fold";
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    OptionalOutputs<4> out;
    out.host[0] = count; out.host[1] = wsum; out.host[2] = wrsum; out.host[3] = varsum;
    if ((rc = ef_refuse_call(ctx, who, F, freqs, nbins, time_0, MTG_LS_STANDARD, out.what() == 0))) return rc;
    const int64_t L = ctx->L;
    // every asked-for output whole on the device: at most MTG_PF_MAX_ENTRIES entries each
    if (F > MTG_PF_MAX_ENTRIES / nbins || L > MTG_PF_MAX_ENTRIES / (F * nbins))
        return fail(ctx, MTG_E_ARG, "%s: L F nbins = %lld x %lld x %d exceeds %lld entries per output (fold fewer frequencies per call)", who,
                    (long long)L, (long long)F, nbins, (long long)MTG_PF_MAX_ENTRIES);
    if ((rc = c.begin())) return rc;
    const MtgEfPlan plan = mtg_ef_plan(nbins, F, L, !ctx->t_per_lc, weighted ? 1 : 0);
    DevBuf d_freqs;
    c.reserve({{d_freqs, (size_t)F * 8}});
    out.reserve(c, (size_t)L * (size_t)F * (size_t)nbins);
    MtgEpochFoldArgs qa;
    qa.ls = c.args(1, MTG_LS_STANDARD, weighted, F, d_freqs.as<double>(), nullptr, false);
    c.upload(d_freqs.p, freqs, (size_t)F * 8);
    qa.nbins = nbins; qa.time_0 = time_0;
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_epoch_fold_kernel<%d,%d> lanes %d", plan.tile, weighted ? 1 : 0, plan.lanes);
    c.run_slabs(L, MTG_PF_SLAB, [&] { mtg_launch_lomb_scargle_stats(qa.ls, c.s); }, [&](int64_t l0, int64_t rows) {
        const int64_t at = l0 * F * nbins;
        qa.count = out.at<int64_t>(0, at); qa.wsum = out.at(1, at); qa.wrsum = out.at(2, at); qa.varsum = out.at(3, at);
        return mtg_launch_epoch_fold(qa, plan, l0, rows, c.s);
    });
    out.gather(c);
    return c.finish();
}

MTG_API int mtg_wwz(mtg_ctx *ctx, int64_t F, const double *freqs, int64_t T, const double *taus, double decay, int statistic, int weighted,
                    double *out, double *neff, double *peak, int64_t *peak_index)
{
    const char *who = "mtg_wwz";
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    if ((rc = refuse_no_freqs(ctx, who, F, freqs))) return rc;
    if (T < 1 || !taus) return fail(ctx, MTG_E_ARG, "%s: need T >= 1 window centres", who);
    if (!out && !neff && !peak && !peak_index) return fail(ctx, MTG_E_ARG, "%s: every output is NULL", who);
    if (!std::isfinite(decay) || decay < 0.0) return fail(ctx, MTG_E_ARG, "%s: decay = %g is not a finite constant >= 0", who, decay);
    if (statistic < MTG_WWZ_POWER || statistic > MTG_WWZ_AMPLITUDE) return fail(ctx, MTG_E_ARG, "%s: unknown statistic %d", who, statistic);
    if (ctx->N < 4)
        return fail(ctx, MTG_E_ARG, "%s: N = %lld < 4 samples (a sinusoid with a floating mean fits three exactly)", who, (long long)ctx->N);
    const int64_t L = ctx->L;
    if (T > INT64_MAX / 8 / F || L > INT64_MAX / 8 / (T * F))
        return fail(ctx, MTG_E_ARG, "%s: L T F = %lld x %lld x %lld is beyond int64", who, (long long)L, (long long)T, (long long)F);
    if ((rc = refuse_bad_freqs(ctx, who, F, freqs))) return rc;
    for (int64_t j = 0; j < T; ++j)
        if (!std::isfinite(taus[j])) return fail(ctx, MTG_E_ARG, "%s: taus[%lld] is not finite", who, (long long)j);
    if ((rc = c.begin())) return rc;
    const MtgWwzPlan plan = mtg_wwz_plan(F, T, L, !ctx->t_per_lc, weighted ? 1 : 0);
    const int64_t Ls = plan.slab;
    const size_t map_bytes = (size_t)T * (size_t)F * 8;
    const bool want_peak = peak || peak_index, want_values = out || want_peak;
    DevBuf d_freqs, d_taus, d_near, d_out, d_neff;
    c.reserve({{d_freqs, (size_t)F * 8}, {d_taus, (size_t)T * 8}, {d_near, (size_t)(ctx->t_per_lc ? Ls : 1) * (size_t)T * 8},
               {d_out, want_values ? (size_t)Ls * map_bytes : 0}, {d_neff, neff ? (size_t)Ls * map_bytes : 0}});
    MtgWwzArgs qa;
    qa.ls = c.args(1, MTG_LS_STANDARD, weighted, F, d_freqs.as<double>(), d_out.as<double>(), want_peak);
    c.upload(d_freqs.p, freqs, (size_t)F * 8);
    c.upload(d_taus.p, taus, (size_t)T * 8);
    qa.T = T; qa.taus = d_taus.as<double>(); qa.kc = 39.478417604357434 * decay;   // 4 pi^2
    qa.statistic = statistic; qa.neff = d_neff.as<double>(); qa.nearest = d_near.as<double>();
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_wwz_kernel<%d,%d> lanes %d", plan.tile, weighted ? 1 : 0, plan.lanes);
    c.run_slabs(L, Ls, [&] { mtg_launch_lomb_scargle_stats(qa.ls, c.s); },
                [&](int64_t l0, int64_t rows) { return mtg_launch_wwz(qa, plan, l0, rows, c.s); },
                [&](int64_t l0, int64_t rows) {
                    if (out) c.gather(out + l0 * T * F, d_out.p, (size_t)rows * map_bytes);
                    if (neff) c.gather(neff + l0 * T * F, d_neff.p, (size_t)rows * map_bytes);
                });
    c.gather_peaks(peak, peak_index);
    return c.finish();
}

MTG_API int mtg_lag_sums(mtg_ctx *ctx, int nbins, const double *edges, int64_t *count, double *lag, double *sf, double *cf, double *cf2,
                         double *noise)
{
    const char *who = "mtg_lag_sums";
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    OptionalOutputs<6> out;
    out.host[0] = count; out.host[1] = lag; out.host[2] = sf; out.host[3] = cf; out.host[4] = cf2; out.host[5] = noise;
    if ((rc = lag_refuse_edges(ctx, who, nbins, edges, out.what() == 0, false))) return rc;
    if (ctx->N < 2) return fail(ctx, MTG_E_ARG, "%s: N = %lld < 2 samples (no pairs)", who, (long long)ctx->N);
    if ((rc = c.begin())) return rc;
    const int64_t L = ctx->L;
    const MtgLagPlan plan = mtg_lag_plan(ctx->N, nbins, L, !ctx->t_per_lc, out.what());
    DevBuf d_edges, d_ws;
    c.reserve({{d_edges, (size_t)(nbins + 1) * 8}, {d_ws, (size_t)plan.ws_bytes}});
    out.reserve(c, (size_t)L * (size_t)nbins);
    MtgLagArgs qa;
    qa.ls = c.args(1, MTG_LS_STANDARD, 0, 0, nullptr, nullptr, false);
    c.upload(d_edges.p, edges, (size_t)(nbins + 1) * 8);
    qa.nbins = nbins; qa.edges = d_edges.as<double>(); qa.ws = d_ws.as<double>();
    qa.count = out.at<int64_t>(0); qa.lag = out.at(1); qa.sf = out.at(2); qa.cf = out.at(3); qa.cf2 = out.at(4); qa.noise = out.at(5);
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_lag_kernel<%d,%d> lanes %d", plan.tile, plan.all, (int)MTG_LAG_LANES);
    c.run_slabs(L, plan.slab, [&] { mtg_launch_lomb_scargle_stats(qa.ls, c.s); },
                [&](int64_t l0, int64_t rows) { return mtg_launch_lag(qa, plan, l0, rows, c.s); });
    out.gather(c);
    return c.finish();
}

MTG_API int mtg_cross_sums(mtg_ctx *ctx, int64_t M, const double *t2, int64_t L2, const double *y2, int nbins, const double *edges,
                           int64_t *count, double *lag, double *cf, double *cf2, double *sa, double *sb, double *saa, double *sbb)
{
    const char *who = "mtg_cross_sums";
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    const int64_t L = ctx->L;
    OptionalOutputs<8> out;
    out.host[0] = count; out.host[1] = lag; out.host[2] = cf; out.host[3] = cf2;
    out.host[4] = sa; out.host[5] = sb; out.host[6] = saa; out.host[7] = sbb;
    if (M < 1 || M >= MTG_CROSS_MAX_M) return fail(ctx, MTG_E_ARG, "%s: M = %lld is outside 1 .. 2^28 - 1", who, (long long)M);
    if (L2 != 1 && L2 != L) return fail(ctx, MTG_E_ARG, "%s: L2 = %lld is neither 1 nor L = %lld", who, (long long)L2, (long long)L);
    if (!t2 || !y2) return fail(ctx, MTG_E_ARG, "%s: need the companion's M times and L2 x M values", who);
    if ((rc = lag_refuse_edges(ctx, who, nbins, edges, out.what() == 0, true))) return rc;
    for (int64_t j = 0; j < M; ++j) {
        if (!std::isfinite(t2[j])) return fail(ctx, MTG_E_ARG, "%s: t2[%lld] is not finite", who, (long long)j);
        if (j > 0 && t2[j] < t2[j - 1])
            return fail(ctx, MTG_E_ARG, "%s: t2[%lld] = %g is below t2[%lld] = %g (the times must ascend)", who, (long long)j, t2[j],
                        (long long)(j - 1), t2[j - 1]);
    }
    for (int64_t k = 0; k < L2 * M; ++k)
        if (!std::isfinite(y2[k])) return fail(ctx, MTG_E_ARG, "%s: y2[%lld][%lld] is not finite", who, (long long)(k / M), (long long)(k % M));
    if ((rc = c.begin())) return rc;
    // (a set of one light curve has L2 == 1 == L: the shared-companion kernel, the same arithmetic)
    const MtgCrossPlan plan = mtg_cross_plan(ctx->N, M, nbins, L, !ctx->t_per_lc, L2 == L && L > 1, out.what());
    const size_t rows2 = (size_t)L2 * (size_t)M;
    // the companion as the pre-pass reads a light curve: (value, variance) pairs; the variance is not read unweighted
    std::vector<double2> pairs(rows2);
    for (size_t k = 0; k < rows2; ++k) pairs[k] = make_double2(y2[k], 1.0);
    DevBuf d_edges, d_t2, d_yv2, d_stats2, d_ws;
    c.reserve({{d_edges, (size_t)(nbins + 1) * 8}, {d_t2, (size_t)M * 8}, {d_yv2, rows2 * 16}, {d_stats2, (size_t)L2 * 32},
               {d_ws, (size_t)plan.ws_bytes}});
    out.reserve(c, (size_t)L * (size_t)nbins);
    MtgCrossArgs qa;
    qa.ls = c.args(1, MTG_LS_STANDARD, 0, 0, nullptr, nullptr, false);
    c.upload(d_edges.p, edges, (size_t)(nbins + 1) * 8);
    c.upload(d_t2.p, t2, (size_t)M * 8);
    c.upload(d_yv2.p, pairs.data(), rows2 * 16);
    MtgLombScargleArgs companion = qa.ls;      // the same pre-pass on the companion's rows as light curves of M samples
    companion.dxt = nullptr; companion.yv = d_yv2.as<double2>(); companion.N = M; companion.t_stride = 0; companion.L = L2;
    companion.stats = d_stats2.as<double>();
    qa.M = M; qa.t2 = d_t2.as<double>(); qa.yv2 = d_yv2.as<double2>(); qa.stats2 = d_stats2.as<double>();
    qa.nbins = nbins; qa.edges = d_edges.as<double>(); qa.ws = d_ws.as<double>();
    qa.count = out.at<int64_t>(0); qa.lag = out.at(1); qa.cf = out.at(2); qa.cf2 = out.at(3);
    qa.sa = out.at(4); qa.sb = out.at(5); qa.saa = out.at(6); qa.sbb = out.at(7);
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_cross_kernel<%d,%d,%d> lanes %d", plan.tile, plan.per, plan.all,
             (int)MTG_CROSS_LANES);
    c.run_slabs(L, plan.slab, [&] { mtg_launch_lomb_scargle_stats(qa.ls, c.s); mtg_launch_lomb_scargle_stats(companion, c.s); },
                [&](int64_t l0, int64_t rows) { return mtg_launch_cross(qa, plan, l0, rows, c.s); });
    out.gather(c);
    return c.finish();   // (waits for the stream: `pairs` outlives its upload)
}

MTG_API int mtg_iccf(mtg_ctx *ctx, int64_t M, const double *t2, int64_t L2, const double *y2, int64_t K, const double *tau, int mode,
                     double threshold, double *ccf, int64_t *n_a, int64_t *n_b, double *peak, int64_t *peak_index, double *centroid)
{
    const char *who = "mtg_iccf";
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    const int64_t L = ctx->L;
    if (M < 2 || M >= MTG_ICCF_MAX_M) return fail(ctx, MTG_E_ARG, "%s: M = %lld is outside 2 .. 2^28 - 1", who, (long long)M);
    if (ctx->N < 2) return fail(ctx, MTG_E_ARG, "%s: N = %lld < 2 samples (nothing to interpolate between)", who, (long long)ctx->N);
    if (L2 != 1 && L2 != L) return fail(ctx, MTG_E_ARG, "%s: L2 = %lld is neither 1 nor L = %lld", who, (long long)L2, (long long)L);
    if (!t2 || !y2) return fail(ctx, MTG_E_ARG, "%s: need the companion's M times and L2 x M values", who);
    if (K < 1 || K > MTG_ICCF_MAX_LAGS || !tau) return fail(ctx, MTG_E_ARG, "%s: K = %lld lags is outside 1 .. %d", who, (long long)K, (int)MTG_ICCF_MAX_LAGS);
    if (mode < MTG_ICCF_BOTH || mode > MTG_ICCF_RESIDENT) return fail(ctx, MTG_E_ARG, "%s: unknown mode %d", who, mode);
    if (!(threshold > 0.0 && threshold <= 1.0)) return fail(ctx, MTG_E_ARG, "%s: threshold = %g is outside (0, 1]", who, threshold);
    const bool want_peak = peak || peak_index || centroid, want_values = ccf || want_peak;
    if (!want_values && !n_a && !n_b) return fail(ctx, MTG_E_ARG, "%s: every output is NULL", who);
    for (int64_t j = 0; j < M; ++j) {
        if (!std::isfinite(t2[j])) return fail(ctx, MTG_E_ARG, "%s: t2[%lld] is not finite", who, (long long)j);
        if (j > 0 && t2[j] < t2[j - 1])
            return fail(ctx, MTG_E_ARG, "%s: t2[%lld] = %g is below t2[%lld] = %g (the times must ascend)", who, (long long)j, t2[j],
                        (long long)(j - 1), t2[j - 1]);
    }
    for (int64_t k = 0; k < L2 * M; ++k)
        if (!std::isfinite(y2[k])) return fail(ctx, MTG_E_ARG, "%s: y2[%lld][%lld] is not finite", who, (long long)(k / M), (long long)(k % M));
    for (int64_t k = 0; k < K; ++k)
        if (!std::isfinite(tau[k])) return fail(ctx, MTG_E_ARG, "%s: tau[%lld] is not finite", who, (long long)k);
    if ((rc = c.begin())) return rc;
    const int arrays = (want_values ? 1 : 0) + (n_a ? 1 : 0) + (n_b ? 1 : 0);
    // (a set of one light curve has L2 == 1 == L: the shared-companion kernel, the same arithmetic)
    const MtgIccfPlan plan = mtg_iccf_plan(K, L, !ctx->t_per_lc, L2 == L && L > 1, mode == MTG_ICCF_COMPANION, arrays);
    const int64_t Ls = plan.slab;
    const size_t rows2 = (size_t)L2 * (size_t)M, slab_bytes = (size_t)Ls * (size_t)K * 8;
    std::vector<double2> pairs(rows2);   // the companion as the pre-pass reads a light curve, as in mtg_cross_sums
    for (size_t k = 0; k < rows2; ++k) pairs[k] = make_double2(y2[k], 1.0);
    // neighbouring lanes take neighbouring lags: the lags' ranks, ties in the given order (no output bit depends on it)
    std::vector<int32_t> order((size_t)K);
    for (int64_t k = 0; k < K; ++k) order[(size_t)k] = (int32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return tau[p] < tau[q]; });
    DevBuf d_tau, d_order, d_t2, d_yv2, d_stats2, d_ccf, d_na, d_nb, d_centroid;
    c.reserve({{d_tau, (size_t)K * 8}, {d_order, (size_t)K * 4}, {d_t2, (size_t)M * 8}, {d_yv2, rows2 * 16}, {d_stats2, (size_t)L2 * 32},
               {d_ccf, want_values ? slab_bytes : 0}, {d_na, n_a ? slab_bytes : 0}, {d_nb, n_b ? slab_bytes : 0},
               {d_centroid, centroid ? (size_t)L * 8 : 0}});
    MtgIccfArgs qa;
    qa.ls = c.args(1, MTG_LS_STANDARD, 0, 0, nullptr, nullptr, peak || peak_index);
    c.upload(d_tau.p, tau, (size_t)K * 8);
    c.upload(d_order.p, order.data(), (size_t)K * 4);
    c.upload(d_t2.p, t2, (size_t)M * 8);
    c.upload(d_yv2.p, pairs.data(), rows2 * 16);
    MtgLombScargleArgs companion = qa.ls;      // the same pre-pass on the companion's rows as light curves of M samples
    companion.dxt = nullptr; companion.yv = d_yv2.as<double2>(); companion.N = M; companion.t_stride = 0; companion.L = L2;
    companion.stats = d_stats2.as<double>();
    qa.M = M; qa.t2 = d_t2.as<double>(); qa.yv2 = d_yv2.as<double2>(); qa.stats2 = d_stats2.as<double>();
    qa.K = K; qa.tau = d_tau.as<double>(); qa.order = d_order.as<int32_t>(); qa.mode = mode; qa.threshold = threshold;
    qa.ccf = want_values ? d_ccf.as<double>() : nullptr;
    qa.n_a = n_a ? d_na.as<int64_t>() : nullptr; qa.n_b = n_b ? d_nb.as<int64_t>() : nullptr;
    qa.peak = qa.ls.peak_power; qa.peak_index = qa.ls.peak_index;   // (both or neither)
    qa.centroid = centroid ? d_centroid.as<double>() : nullptr;
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_iccf_kernel<%d,%d,%d> lanes %d", plan.tile, plan.per, plan.all,
             (int)MTG_ICCF_LANES);
    c.run_slabs(L, Ls, [&] { mtg_launch_lomb_scargle_stats(qa.ls, c.s); mtg_launch_lomb_scargle_stats(companion, c.s); },
                [&](int64_t l0, int64_t rows) { return mtg_launch_iccf(qa, plan, l0, rows, c.s); },
                [&](int64_t l0, int64_t rows) {
                    const size_t bytes = (size_t)rows * (size_t)K * 8;
                    if (ccf) c.gather(ccf + l0 * K, d_ccf.p, bytes);
                    if (n_a) c.gather(n_a + l0 * K, d_na.p, bytes);
                    if (n_b) c.gather(n_b + l0 * K, d_nb.p, bytes);
                });
    c.gather_peaks(peak, peak_index);
    if (centroid) c.gather(centroid, d_centroid.p, (size_t)L * 8);
    return c.finish();   // (waits for the stream: `pairs` and `order` outlive their uploads)
}

// mtg_lomb_scargle_envelope (nterms = 1) and mtg_lomb_scargle_envelope_multi
static int lomb_scargle_envelope_entry(mtg_ctx *ctx, const char *who, int64_t F, const double *freqs, int nterms, int normalization,
                                       int weighted, int Q, const int64_t *ranks, double *order_stat, int64_t *valid,
                                       const double *reference, int64_t *exceed, const double *scale, double *peak_ratio,
                                       int64_t *peak_ratio_index)
{
    ResidentCall c{ctx, who};
    int rc = c.ready();
    if (rc) return rc;
    if ((rc = ls_refuse_call(ctx, who, F, freqs, nterms, normalization, false))) return rc;
    const int64_t L = ctx->L;
    if (Q < 0 || (Q > 0 && !ranks)) return fail(ctx, MTG_E_ARG, "%s: Q = %d ranks%s", who, Q, Q < 0 ? "" : ", ranks is NULL");
    if (Q > 0 && !order_stat) return fail(ctx, MTG_E_ARG, "%s: Q = %d ranks, order_stat is NULL", who, Q);
    for (int q = 0; q < Q; ++q)
        if (ranks[q] < 0 || ranks[q] >= L)
            return fail(ctx, MTG_E_ARG, "%s: ranks[%d] = %lld is outside [0, L = %lld)", who, q, (long long)ranks[q], (long long)L);
    if (exceed && !reference) return fail(ctx, MTG_E_ARG, "%s: exceed needs reference", who);
    const bool want_ratio = peak_ratio || peak_ratio_index, want_columns = Q > 0 || valid || exceed;
    if (want_ratio && !scale) return fail(ctx, MTG_E_ARG, "%s: peak_ratio and peak_ratio_index need scale", who);
    if (!want_columns && !want_ratio)
        return fail(ctx, MTG_E_ARG, "%s: order_stat, valid, exceed, peak_ratio and peak_ratio_index are all NULL", who);
    for (int64_t k = 0; reference && k < F; ++k)
        if (!std::isfinite(reference[k]))
            return fail(ctx, MTG_E_ARG, "%s: reference[%lld] = %g is not finite", who, (long long)k, reference[k]);
    for (int64_t k = 0; scale && k < F; ++k)
        if (!std::isfinite(scale[k]) || !(scale[k] > 0.0))
            return fail(ctx, MTG_E_ARG, "%s: scale[%lld] = %g is not finite and positive", who, (long long)k, scale[k]);
    if ((rc = c.begin())) return rc;
    // a slab of frequencies at a time, every light curve's power at them: mtg_ls_envelope_plan.h
    const int64_t Fs = mtg_lse_slab_width(L, F, Q, MTG_LSE_BUDGET);
    const bool in_lds = mtg_lse_in_lds(L) != 0;
    const size_t slab_bytes = (size_t)L * (size_t)Fs * 8, temp_bytes = want_columns ? mtg_ls_envelope_temp_bytes(L, Fs) : 0;
    MtgLsEnvelopeArgs ea;
    DevBuf d_freqs, d_power, d_ranks, d_os, d_valid, d_ref, d_exceed, d_scale, d_ka, d_kb, d_temp;
    const bool sort_global = want_columns && !in_lds;
    c.reserve({{d_freqs, (size_t)F * 8}, {d_power, slab_bytes}, {d_ranks, (size_t)Q * 8},
               {d_os, (size_t)Q * (size_t)Fs * 8}, {d_valid, valid ? (size_t)F * 8 : 0}, {d_ref, reference ? (size_t)F * 8 : 0},
               {d_exceed, exceed ? (size_t)F * 8 : 0}, {d_scale, want_ratio ? (size_t)F * 8 : 0},
               {d_ka, sort_global ? slab_bytes : 0}, {d_kb, sort_global ? slab_bytes : 0}, {d_temp, sort_global ? temp_bytes + 256 : 0}});
    MtgLombScargleArgs qa = c.args(nterms, normalization, weighted, 0, nullptr, d_power.as<double>(), false);   // (no peaks of the powers)
    c.reserve_peaks(want_ratio);      // the peaks of the ratios instead
    c.upload(d_freqs.p, freqs, (size_t)F * 8);
    if (Q > 0) c.upload(d_ranks.p, ranks, (size_t)Q * 8);
    if (reference) c.upload(d_ref.p, reference, (size_t)F * 8);
    if (want_ratio) c.upload(d_scale.p, scale, (size_t)F * 8);
    ea.slab = d_power.as<double>(); ea.L = L; ea.Q = Q; ea.ranks = d_ranks.as<int64_t>(); ea.order_stat = d_os.as<double>();
    ea.valid = valid ? d_valid.as<int64_t>() : nullptr; ea.reference = reference ? d_ref.as<double>() : nullptr;
    ea.exceed = exceed ? d_exceed.as<int64_t>() : nullptr; ea.scale = d_scale.as<double>();
    ea.peak_ratio = c.peak.as<double>(); ea.peak_ratio_index = c.index.as<int64_t>();
    ea.keys_a = d_ka.p; ea.keys_b = d_kb.p; ea.temp = d_temp.p; ea.temp_bytes = temp_bytes + 256;
    if (!want_columns) snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_ls_envelope_ratio_peak_kernel");
    else if (in_lds) snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_ls_envelope_column_kernel<%d>", mtg_lse_columns(L));
    else snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_ls_envelope_select_kernel");
    c.run_slabs(F, Fs, [&] { mtg_launch_lomb_scargle_stats(qa, c.s); },
                [&](int64_t k0, int64_t cols) {
                    qa.F = cols; qa.freqs = d_freqs.as<double>() + k0;   // the frequencies are each slab's
                    ea.Fs = cols; ea.k0 = k0;
                    hipError_t e = mtg_launch_lomb_scargle(qa, 0, L, c.s) ? hipGetLastError() : hipErrorInvalidValue;
                    if (e == hipSuccess && want_columns) e = mtg_launch_ls_envelope_columns(ea, c.s);
                    if (e == hipSuccess && want_ratio) e = mtg_launch_ls_envelope_ratio_peaks(ea, c.s);
                    return e;
                },
                [&](int64_t k0, int64_t cols) {
                    if (Q > 0) c.then([&] {
                        return hipMemcpy2DAsync(order_stat + k0, (size_t)F * 8, d_os.p, (size_t)cols * 8, (size_t)cols * 8, (size_t)Q,
                                                hipMemcpyDeviceToHost, c.s);
                    });
                });
    if (valid) c.gather(valid, d_valid.p, (size_t)F * 8);
    if (exceed) c.gather(exceed, d_exceed.p, (size_t)F * 8);
    c.gather_peaks(peak_ratio, peak_ratio_index);
    return c.finish();
}

MTG_API int mtg_lomb_scargle_envelope(mtg_ctx *ctx, int64_t F, const double *freqs, int normalization, int weighted, int Q,
                                      const int64_t *ranks, double *order_stat, int64_t *valid, const double *reference,
                                      int64_t *exceed, const double *scale, double *peak_ratio, int64_t *peak_ratio_index)
{
    return lomb_scargle_envelope_entry(ctx, "mtg_lomb_scargle_envelope", F, freqs, 1, normalization, weighted, Q, ranks, order_stat,
                                       valid, reference, exceed, scale, peak_ratio, peak_ratio_index);
}

MTG_API int mtg_lomb_scargle_envelope_multi(mtg_ctx *ctx, int64_t F, const double *freqs, int nterms, int normalization, int weighted,
                                            int Q, const int64_t *ranks, double *order_stat, int64_t *valid, const double *reference,
                                            int64_t *exceed, const double *scale, double *peak_ratio, int64_t *peak_ratio_index)
{
    return lomb_scargle_envelope_entry(ctx, "mtg_lomb_scargle_envelope_multi", F, freqs, nterms, normalization, weighted, Q, ranks,
                                       order_stat, valid, reference, exceed, scale, peak_ratio, peak_ratio_index);
}

MTG_API int mtg_gp_draw(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, uint64_t seed,
                        const double *normals, double *y, int32_t *status)
{
    RowCall c{ctx, "mtg_gp_draw", B, theta, lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (B <= 0 || !y || !status || (!theta && ctx->model.P > 0)) return c.bad_arguments();
    if ((rc = c.begin(true))) return rc;
    const int J = ctx->model.nr0 + 2 * ctx->model.nc0;
    const int64_t N = ctx->N;
    if (J > MTG_MAX_J) return fail(ctx, MTG_E_UNSUPPORTED, "mtg_gp_draw: rank %d > %d", J, MTG_MAX_J);
    const size_t row_bytes = (size_t)N * 8;
    const int64_t Bs = mtg_plan_draw_slab(N, B);
    MtgGpDrawArgs qa;
    c.stage_inputs();
    c.expand(qa);
    DevBuf d_y, d_q;
    c.reserve({{d_y, (size_t)Bs * row_bytes}, {d_q, normals ? (size_t)Bs * row_bytes : 0}});
    qa.normals = normals ? d_q.as<double>() : nullptr;
    qa.seed_lo = (uint32_t)seed; qa.seed_hi = (uint32_t)(seed >> 32); qa.draw0 = ctx->stream_base;
    qa.y = d_y.as<double>();
    if (c.ok()) c.e = for_each_slab(B, Bs, [&](int64_t row0, int64_t rows) {
        qa.row0 = row0; qa.B = rows;
        // (the copies are ordered on the stream: the next slab's upload and kernel touch the buffers only after them)
        if (normals) c.upload(d_q.p, normals + row0 * N, (size_t)rows * row_bytes);
        c.then([&] { return mtg_launch_gp_draw(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        c.gather(y + row0 * N, d_y.p, (size_t)rows * row_bytes);
        return c.e;
    });
    return c.finish(status);
}

MTG_API int mtg_whiten(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, const double *y, double *q,
                       int K, double *acf, double *stats, int32_t *status)
{
    RowCall c{ctx, "mtg_whiten", B, theta, lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (B < 0 || !status || (!theta && ctx->model.P > 0 && B > 0) || (!q && !acf && !stats)) return c.bad_arguments();
    const int64_t N = ctx->N;
    if (acf ? (K < 1 || K > N - 1) : K != 0)
        return fail(ctx, MTG_E_ARG, "mtg_whiten: K = %d lags%s (1 <= K <= N - 1 = %lld with acf, 0 without)", K, acf ? "" : ", acf is NULL",
                    (long long)(N - 1));
    if ((rc = c.begin(true))) return rc;
    const int J = ctx->model.nr0 + 2 * ctx->model.nc0;
    if (J > MTG_MAX_J) return fail(ctx, MTG_E_UNSUPPORTED, "mtg_whiten: rank %d > %d", J, MTG_MAX_J);
    if (B == 0) return MTG_OK;
    const size_t row_bytes = (size_t)N * 8, stat_bytes = (size_t)MTG_WHITEN_NSTATS * 8;
    // D+ and D- need the rows' residuals on the device: with stats alone the sweep stores nothing of size N, writes its
    // sums and leaves NaN in the two slots; with acf but no q the residuals go to the context's slab
    const bool need_q = q || acf, want_ks = stats && need_q;
    const int64_t Bs = mtg_plan_whiten_slab(N, B, ctx->window_bytes, want_ks);
    const size_t temp_bytes = want_ks ? mtg_whiten_sort_temp_bytes(Bs, N) : 0;
    if (want_ks && temp_bytes == 0) return fail(ctx, MTG_E_ARG, "mtg_whiten: N = %lld is too large for the KS sort", (long long)N);
    MtgWhitenArgs qa;
    c.stage_inputs();
    c.expand(qa);
    c.reserve({{ctx->whiten_y, y ? (size_t)Bs * row_bytes : 0}, {ctx->whiten_q, need_q ? (size_t)Bs * row_bytes : 0},
               {ctx->whiten_sorted, want_ks ? (size_t)Bs * row_bytes : 0}, {ctx->whiten_acf, acf ? (size_t)Bs * (size_t)K * 8 : 0},
               {ctx->whiten_temp, temp_bytes}, {ctx->whiten_stats, (size_t)B * stat_bytes}});
    qa.y = y ? ctx->whiten_y.as<double>() : nullptr;
    qa.q = need_q ? ctx->whiten_q.as<double>() : nullptr;
    qa.stats = ctx->whiten_stats.as<double>();
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_whiten_kernel<%d>", J);
    c.then([&] { return hipEventRecord(ctx->ev0, c.s); });
    if (c.ok()) c.e = for_each_slab(B, Bs, [&](int64_t row0, int64_t rows) {
        qa.row0 = row0; qa.B = rows;
        // (the copies are ordered on the stream: the next slab's upload and kernels touch the buffers only after them)
        if (y) c.upload(ctx->whiten_y.p, y + row0 * N, (size_t)rows * row_bytes);
        c.then([&] { return mtg_launch_whiten(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        if (want_ks) c.then([&] { return mtg_launch_whiten_ks(qa, ctx->whiten_sorted.as<double>(), ctx->whiten_temp.p, temp_bytes, c.s); });
        if (acf) c.then([&] { return mtg_launch_whiten_acf(qa, K, ctx->whiten_acf.as<double>(), c.s); });
        if (row0 + rows == B) c.then([&] { return hipEventRecord(ctx->ev1, c.s); });
        if (q) c.gather(q + row0 * N, ctx->whiten_q.p, (size_t)rows * row_bytes);
        if (acf) c.gather(acf + row0 * K, ctx->whiten_acf.p, (size_t)rows * (size_t)K * 8);
        return c.e;
    });
    if (c.ok()) ctx->timed = true;
    if (stats) c.gather(stats, ctx->whiten_stats.p, (size_t)B * stat_bytes);
    rc = c.finish(status);
    // (the stream is idle) a large call does not leave its slabs with the context: up to four of 256 MiB
    for (DevBuf *buf : {&ctx->whiten_y, &ctx->whiten_q, &ctx->whiten_sorted, &ctx->whiten_acf, &ctx->whiten_temp})
        if (buf->cap > MTG_WHITEN_KEEP_BYTES) buf->release();
    return rc;
}

MTG_API int mtg_gp_cond_draw(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int64_t M,
                             const double *ts, uint64_t seed, const double *normals, double *y, int32_t *status)
{
    RowCall c{ctx, "mtg_gp_cond_draw", B, theta, lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (B <= 0 || M < 0 || (M > 0 && (!ts || !y)) || !status || (!theta && ctx->model.P > 0)) return c.bad_arguments();
    if ((rc = c.begin(true))) return rc;
    for (int64_t m = 0; m < M; ++m)
        if (!std::isfinite(ts[m])) return fail(ctx, MTG_E_ARG, "mtg_gp_cond_draw: ts[%lld] is not finite", (long long)m);
    if (M == 0) return MTG_OK;
    // the unique times in ascending order, for each the first entry of ts that holds it (the sort is stable), and for
    // each entry of ts its unique time
    std::vector<int64_t> order((size_t)M), first, inv((size_t)M);
    for (int64_t m = 0; m < M; ++m) order[(size_t)m] = m;
    std::stable_sort(order.begin(), order.end(), [ts](int64_t i, int64_t j) { return ts[i] < ts[j]; });
    std::vector<double> tu;
    for (int64_t m : order) {
        if (tu.empty() || ts[m] != tu.back()) { tu.push_back(ts[m]); first.push_back(m); }
        inv[(size_t)m] = (int64_t)tu.size() - 1;
    }
    const int64_t Mu = (int64_t)tu.size();
    const int J = ctx->model.nr0 + 2 * ctx->model.nc0;
    const int64_t N = ctx->N;
    if (J > MTG_MAX_J) return fail(ctx, MTG_E_UNSUPPORTED, "mtg_gp_cond_draw: rank %d > %d", J, MTG_MAX_J);
    const size_t q_bytes = (size_t)(N + M) * 8;
    // (M >= Mu: the scatter's grid as well as the evaluation's; a row's normals, y - y~, f*, mu and draws within the budget)
    const int64_t Bs = mtg_plan_predict_at_slab(N, J, M, B, (normals ? q_bytes : 0) + (size_t)(N + 2 * Mu + M) * 8);
    if (Bs == 0) return fail(ctx, MTG_E_ARG, "mtg_gp_cond_draw: M = %lld is too large", (long long)M);
    MtgPredictAtArgs qa;
    MtgGpCondDrawArgs da;
    c.stage_inputs();
    c.expand(qa);
    static_cast<MtgRowArgs &>(da) = qa;
    PredictAtRoom room;
    room.reserve(c, qa, Bs, J, Mu, tu.data(), nullptr, false);
    DevBuf d_first, d_inv, d_q, d_data, d_fs, d_y;
    c.reserve({{d_first, normals ? (size_t)Mu * 8 : 0}, {d_inv, (size_t)M * 8}, {d_q, normals ? (size_t)Bs * q_bytes : 0},
               {d_data, (size_t)Bs * N * 8}, {d_fs, (size_t)Bs * Mu * 8}, {d_y, (size_t)Bs * M * 8}});
    if (normals) c.upload(d_first.p, first.data(), (size_t)Mu * 8);
    c.upload(d_inv.p, inv.data(), (size_t)M * 8);
    da.Mu = Mu; da.tu = qa.ts; da.first = normals ? d_first.as<int64_t>() : nullptr; da.M = M; da.inv = d_inv.as<int64_t>();
    da.normals = normals ? d_q.as<double>() : nullptr;
    da.seed_lo = (uint32_t)seed; da.seed_hi = (uint32_t)(seed >> 32); da.draw0 = ctx->stream_base;
    da.data = d_data.as<double>(); da.fs = d_fs.as<double>(); da.mu = qa.mu; da.y = d_y.as<double>();
    qa.data = da.data;
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_gp_cond_draw_kernel<%d>", J);
    if (c.ok()) c.e = for_each_slab(B, Bs, [&](int64_t row0, int64_t rows) {
        qa.row0 = da.row0 = row0; qa.B = da.B = rows;
        // (the copies are ordered on the stream: the next slab's upload and kernels touch the buffers only after them)
        if (normals) c.upload(d_q.p, normals + row0 * (N + M), (size_t)rows * q_bytes);
        c.then([&] { return mtg_launch_gp_cond_draw(da, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        c.then([&] { return mtg_launch_predict_at(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
        c.then([&] { mtg_launch_gp_cond_scatter(da, c.s); return hipGetLastError(); });
        c.gather(y + row0 * M, d_y.p, (size_t)rows * M * 8);
        return c.e;
    });
    return c.finish(status);
}

MTG_API int mtg_loglike_grad(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, int add_prior,
                             double *out, double *grad, int32_t *status)
{
    RowCall c{ctx, "mtg_loglike_grad", B, theta, lc_index, add_prior ? 1 : 0};
    int rc = c.ready();
    if (rc) return rc;
    const int P = ctx->model.P;
    if (B <= 0 || !theta || !out || !grad || !status) return c.bad_arguments();
    // (the refusal here and not in begin: the check of P has always stood between it and the light-curve indices)
    if ((rc = refuse_profile_mean(ctx, c.who))) return rc;
    if (P <= 0) return fail(ctx, MTG_E_ARG, "mtg_loglike_grad: the model has no free parameter");
    if ((rc = c.begin(false))) return rc;
    const int J = ctx->model.nr0 + 2 * ctx->model.nc0;
    if (J > MTG_GRAD_MAX_J)
        return fail(ctx, MTG_E_UNSUPPORTED, "mtg_loglike_grad: rank %d > %d (the tangent sweep keeps its state in registers)", J,
                    MTG_GRAD_MAX_J);
    if (B * P > ((int64_t)1 << 36)) return fail(ctx, MTG_E_ARG, "mtg_loglike_grad: B * P = %lld is too large", (long long)(B * P));
    MtgGradArgs qa;
    c.stage_inputs();
    c.expand(qa);
    const int64_t lanes = B * P, dstride = (lanes + 63) / 64 * 64;
    c.reserve({{ctx->grad_dcoef, (size_t)dstride * qa.lay.nslots() * 8}, {ctx->grad, (size_t)lanes * 8}, {ctx->grad_verdict, (size_t)B * 4}});
    qa.model = ctx->model; qa.theta = ctx->theta.as<double>(); qa.P = P;
    qa.dcoef = ctx->grad_dcoef.as<double>(); qa.dstride = dstride;
    qa.out = ctx->out.as<double>(); qa.grad = ctx->grad.as<double>(); qa.verdict = ctx->grad_verdict.as<int32_t>();
    c.then([&] { return hipEventRecord(ctx->ev0, c.s); });   // mtg_last_kernel_ms: the coefficient tangents and the sweep (not the expansion)
    c.then([&] { return mtg_launch_loglike_grad(qa, c.s) ? hipGetLastError() : hipErrorInvalidValue; });
    c.then([&] { return hipEventRecord(ctx->ev1, c.s); });
    if (c.ok()) ctx->timed = true;
    c.gather(out, ctx->out.p, (size_t)B * 8);
    c.gather(grad, ctx->grad.p, (size_t)lanes * 8);
    if ((rc = c.finish(status))) return rc;
    snprintf(ctx->last_solver, sizeof ctx->last_solver, "mtg_loglike_grad_kernel<%d>", J);
    return MTG_OK;
}

MTG_API int mtg_apply_inverse(mtg_ctx *ctx, const double *theta, int32_t lc_index, int64_t M, double *x,
                              int32_t *status)
{
    RowCall c{ctx, "mtg_apply_inverse", 1, theta, &lc_index, 1};
    int rc = c.ready();
    if (rc) return rc;
    if (M <= 0 || !x || !status || (!theta && ctx->model.P > 0)) return c.bad_arguments();
    if (lc_index < 0 || lc_index >= ctx->L)
        return fail(ctx, MTG_E_ARG, "lc_index = %d outside [0, %lld)", lc_index, (long long)ctx->L);
    if ((rc = c.begin(false))) return rc;
    const MtgModel &m = ctx->model;
    const int Jws = m.nr_max + 2 * m.nc_max, J = m.nr0 + 2 * m.nc0;
    const int64_t N = ctx->N;
    const size_t x_bytes = (size_t)N * M * 8;
    // the factorisation of this parameter vector: the forward sweep of mtg_predict_kernel leaves
    // U_n, W_n, phi_n, D_n of every sample in `work`
    MtgPredictArgs qa;
    c.stage_inputs();
    c.expand(qa);
    DevBuf work, d_mu, d_var, d_x;
    c.reserve({{work, (size_t)N * (3 * Jws + 2) * 8}, {d_mu, (size_t)N * 8}, {d_var, (size_t)N * 8}, {d_x, x_bytes}});
    c.upload(d_x.p, x, x_bytes);
    c.then([&] {
        qa.work = work.as<double>(); qa.mu = d_mu.as<double>(); qa.var = d_var.as<double>();
        mtg_launch_predict(qa, c.s);
        return hipGetLastError();
    });
    // the verdict first: the solve is launched, and x overwritten, only for a row the factorisation accepted
    c.gather(status, ctx->status.p, 4);
    c.sync();
    if (c.ok() && *status == MTG_ST_OK) {
        mtg_launch_apply_inverse(work.as<double>(), N, J, M, d_x.as<double>(), c.s);
        c.e = hipGetLastError();
        c.gather(x, d_x.p, x_bytes);
    }
    return c.finish(nullptr);
}

MTG_API int mtg_math_probe(mtg_ctx *ctx, int64_t n, const double *x, double *exp_neg, double *sin_x,
                           double *cos_x, double *rcp_x)
{
    if (!ctx || n <= 0 || !x || !exp_neg || !sin_x || !cos_x || !rcp_x) return MTG_E_ARG;
    RowCall c{ctx, "mtg_math_probe", n, nullptr, nullptr, 0};   // (no rows of theta: the call's stream and its one way out)
    if (const int rc = c.begin(false)) return rc;
    DevBuf buf;
    c.reserve({{buf, (size_t)n * 8 * 5}});
    double *d = buf.as<double>();
    c.upload(d, x, (size_t)n * 8);
    c.then([&] {
        mtg_launch_math_probe(n, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, c.s);
        return hipGetLastError();
    });
    double *const outs[4] = {exp_neg, sin_x, cos_x, rcp_x};
    for (int i = 0; i < 4; ++i) c.gather(outs[i], d + (i + 1) * n, (size_t)n * 8);
    return c.finish(nullptr);
}

MTG_API int mtg_set_time_parallel(mtg_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 3) return MTG_E_ARG;
    ctx->tp_mode = mode;
    return MTG_OK;
}

MTG_API int mtg_set_simulate_draws(mtg_ctx *ctx, int64_t S, int64_t nk, const double *normals, const int64_t *starts)
{
    if (!ctx) return MTG_E_ARG;
    ctx->given.S = 0;
    ctx->given.nk = 0;
    if (S == 0) return MTG_OK;  // cleared
    if (S < 0 || nk < 3 || !normals || !starts) return fail(ctx, MTG_E_ARG, "mtg_set_simulate_draws: bad arguments");
    for (int64_t i = 0; i < S; ++i)
        if (starts[i] < 0) return fail(ctx, MTG_E_ARG, "mtg_set_simulate_draws: starts[%lld] = %lld is negative", (long long)i, (long long)starts[i]);
    int rc = use_device(ctx);
    if (rc) return rc;
    CTX_STREAM(ctx, s);
    HIP_TRY(ctx, ctx->given.normals.reserve((size_t)S * 2 * nk * 8));
    HIP_TRY(ctx, ctx->given.starts.reserve((size_t)S * 8));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->given.normals.p, normals, (size_t)S * 2 * nk * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->given.starts.p, starts, (size_t)S * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));  // the caller's arrays are free again
    ctx->given.starts_host.assign(starts, starts + S);
    ctx->given.S = S;
    ctx->given.nk = nk;
    return MTG_OK;
}

MTG_API int mtg_set_simulate_pairs(mtg_ctx *ctx, int on)
{
    if (!ctx) return MTG_E_ARG;
    ctx->czt.pairs_on = on != 0;
    return MTG_OK;
}

MTG_API int64_t mtg_chain_autocorr_plans_built(const mtg_ctx *ctx) { return ctx ? ctx->acf_plans_built : -1; }

MTG_API int mtg_set_simulate_kraft(mtg_ctx *ctx, int64_t N, int K, double threshold, const double *bkg_counts, const double *bkg_rate_err,
                                   const double *median, const double *half)
{
    if (!ctx) return MTG_E_ARG;
    if (N == 0) { ctx->kraft.N = 0; return MTG_OK; }
    if (N < 0 || K < 1 || K > 4096 || !(threshold >= 0.0) || threshold > (double)K || !bkg_counts || !bkg_rate_err || !median || !half)
        return fail(ctx, MTG_E_ARG, "mtg_set_simulate_kraft: bad arguments (the tables must cover total counts 0 .. K - 1 >= threshold - 1)");
    int rc = use_device(ctx);
    if (rc) return rc;
    CTX_STREAM(ctx, s);
    HIP_TRY(ctx, ctx->kraft.bkg.reserve((size_t)N * 8));
    HIP_TRY(ctx, ctx->kraft.err.reserve((size_t)N * 8));
    HIP_TRY(ctx, ctx->kraft.med.reserve((size_t)N * K * 8));
    HIP_TRY(ctx, ctx->kraft.half.reserve((size_t)N * K * 8));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->kraft.bkg.p, bkg_counts, (size_t)N * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->kraft.err.p, bkg_rate_err, (size_t)N * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->kraft.med.p, median, (size_t)N * K * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->kraft.half.p, half, (size_t)N * K * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->kraft.N = N; ctx->kraft.K = K; ctx->kraft.threshold = threshold;
    return MTG_OK;
}

MTG_API int mtg_set_simulate_pdf(mtg_ctx *ctx, int kind, int max_iter)
{
    if (!ctx || kind < 0 || kind > 2 || max_iter < 0) return MTG_E_ARG;
    ctx->e13.kind = kind;
    ctx->e13.max_iter = max_iter;
    return MTG_OK;
}

MTG_API int mtg_set_simulate_pdf_draws(mtg_ctx *ctx, int64_t S, int64_t n, const double *draws)
{
    if (!ctx) return MTG_E_ARG;
    if (S == 0 || !draws) { ctx->e13.given_S = 0; return MTG_OK; }
    if (S < 0 || n < 2) return fail(ctx, MTG_E_ARG, "mtg_set_simulate_pdf_draws: bad shape");
    int rc = use_device(ctx);
    if (rc) return rc;
    CTX_STREAM(ctx, s);
    HIP_TRY(ctx, ctx->e13.given.reserve((size_t)S * n * 8));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->e13.given.p, draws, (size_t)S * n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->e13.given_S = S; ctx->e13.given_n = n;
    return MTG_OK;
}

MTG_API int mtg_simulate_pdf_report(const mtg_ctx *ctx, int64_t *not_converged, int *iterations)
{
    if (!ctx) return MTG_E_ARG;
    if (not_converged) *not_converged = ctx->e13.not_converged;
    if (iterations) *iterations = ctx->e13.iterations;
    return MTG_OK;
}

MTG_API int mtg_set_simulate_transform(mtg_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return MTG_E_ARG;
    ctx->sim_transform = mode;
    return MTG_OK;
}

MTG_API int mtg_set_stream_base(mtg_ctx *ctx, int64_t first_index)
{
    if (!ctx) return MTG_E_ARG;
    if (first_index < 0 || first_index > 0x7fffffffll) return fail(ctx, MTG_E_ARG, "stream base must be in [0, 2^31)");
    ctx->stream_base = first_index;
    return MTG_OK;
}

MTG_API int mtg_set_pipeline(mtg_ctx *ctx, int mode)
{
    if (!ctx) return MTG_E_ARG;
    if (mode < 0 || mode > 2) return fail(ctx, MTG_E_ARG, "pipeline mode must be 0, 1 or 2");
    ctx->pipe_mode = mode;
    return MTG_OK;
}

MTG_API int mtg_set_tp_direct(mtg_ctx *ctx, int enabled)
{
    if (!ctx) return MTG_E_ARG;
    ctx->tp_direct = enabled >= 2 ? enabled : (enabled ? 1 : 0);  // 2 (diagnostic): never fall back to the filter pass
    return MTG_OK;
}

MTG_API int mtg_set_speculation(mtg_ctx *ctx, int mode)
{
    if (!ctx) return MTG_E_ARG;
    if (mode < 0 || mode > 2)
        return fail(ctx, MTG_E_ARG, "mtg_set_speculation: mode must be 0 (never), 1 (where it pays) or 2 (as 1, splits ranked in the sampler kernel)");
    ctx->spec_mode = mode;
    return MTG_OK;
}

MTG_API int mtg_set_sort(mtg_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return MTG_E_ARG;
    ctx->sort_mode = mode;
    return MTG_OK;
}

MTG_API const char *mtg_last_solver(const mtg_ctx *ctx) { return ctx ? ctx->last_solver : ""; }

MTG_API int mtg_unpair_contexts(mtg_ctx *ctx)
{
    if (!ctx) return MTG_E_ARG;
    const std::shared_ptr<MtgPair> p = std::atomic_load(&ctx->pair);
    if (!p) return MTG_OK;
    mtg_ctx *members[2];
    {
        // A partner thread may be inside pair_launch right now (waiting for this context's half-step, or about to
        // lock): it holds a reference of its own, sees `broken` and launches alone; the rendezvous is freed by
        // whoever drops the last reference.
        std::lock_guard<std::mutex> lk(p->mu);
        p->broken = true;
        members[0] = p->members[0]; members[1] = p->members[1];
        p->members[0] = p->members[1] = nullptr;
    }
    p->cv.notify_all();
    for (mtg_ctx *m : members)
        if (m) std::atomic_store(&m->pair, std::shared_ptr<MtgPair>());
    return MTG_OK;
}

MTG_API int mtg_pair_contexts(mtg_ctx *a, mtg_ctx *b)
{
    if (!a || !b || a == b) return MTG_E_ARG;
    if (a->device != b->device) return fail(a, MTG_E_ARG, "mtg_pair_contexts: the two contexts are on different devices");
    if (std::atomic_load(&a->pair) || std::atomic_load(&b->pair))
        return fail(a, MTG_E_STATE, "mtg_pair_contexts: a context is paired already (mtg_unpair_contexts first)");
    int rc = use_device(a);
    if (rc) return rc;
    std::shared_ptr<MtgPair> p(new (std::nothrow) MtgPair());
    if (!p) return fail(a, MTG_E_HIP, "mtg_pair_contexts: out of memory");
    for (hipEvent_t *e : {&p->ready[0], &p->ready[1], &p->done})
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess)
            return fail(a, MTG_E_HIP, "mtg_pair_contexts: event creation failed");   // (~MtgPair destroys the ones made)
    p->members[0] = a; p->members[1] = b;
    // Two models that are known now and have no kernel in common -- one of them without a pipelined sweep (a DRW alone),
    // or a pair of shapes that is not compiled -- never meet: broken from the start, nobody waits for a partner that has
    // nothing to bring.  (Models set later are looked at when their half-steps meet.)
    if (a->has_model && b->has_model) {
        auto shape = [](const mtg_ctx *c) { return MtgPipeShapeId{c->model.nr0, c->model.nc0, c->model.nsho + 1, c->model.last_b0 ? 1 : 0}; };
        const MtgPipeShapeId sa = shape(a), sb = shape(b);
        if (!mtg_find_pipe_pair_solver(sa, sb) && !mtg_find_pipe_pair_solver(sb, sa)) p->broken = true;
    }
    std::atomic_store(&a->pair, p);
    std::atomic_store(&b->pair, p);
    return MTG_OK;
}

MTG_API int mtg_set_pair_patience(mtg_ctx *ctx, int milliseconds)
{
    if (!ctx || milliseconds < 1) return MTG_E_ARG;
    const std::shared_ptr<MtgPair> p = std::atomic_load(&ctx->pair);
    if (!p) return fail(ctx, MTG_E_STATE, "mtg_set_pair_patience: the context is not paired");
    std::lock_guard<std::mutex> lk(p->mu);
    p->patience_ms = milliseconds;
    return MTG_OK;
}

MTG_API int mtg_pair_stats(const mtg_ctx *ctx, int64_t *paired_launches, int64_t *solo_launches, int *broken)
{
    if (!ctx) return MTG_E_ARG;
    const std::shared_ptr<MtgPair> p = std::atomic_load(&const_cast<mtg_ctx *>(ctx)->pair);
    if (paired_launches) *paired_launches = 0;
    if (solo_launches) *solo_launches = 0;
    if (broken) *broken = 0;
    if (!p) return MTG_OK;
    std::lock_guard<std::mutex> lk(p->mu);
    if (paired_launches) *paired_launches = p->n_pair;
    if (solo_launches) *solo_launches = p->n_solo;
    if (broken) *broken = p->broken ? 1 : 0;
    return MTG_OK;
}

MTG_API int mtg_synchronize(mtg_ctx *ctx)
{
    if (!ctx) return MTG_E_ARG;
    int rc = use_device(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // ... and on the caller's stream of the last mtg_loglike_batch_device, if nothing has waited for it since
    if (ctx->foreign_pending) HIP_TRY(ctx, hipEventSynchronize(ctx->foreign_done));
    return MTG_OK;
}

MTG_API int mtg_profile_begin(mtg_ctx *ctx, int capacity)
{
    if (!ctx || capacity < 0) return MTG_E_ARG;
    int rc = use_device(ctx);
    if (rc) return rc;
    while ((int)ctx->prof_ev.size() < 3 * capacity) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->prof_ev.push_back(e);
    }
    ctx->prof_cap = capacity;
    ctx->prof_n = 0;
    return MTG_OK;
}

MTG_API int mtg_profile_read(mtg_ctx *ctx, int capacity, double *prepare_ms, double *solve_ms)
{
    if (!ctx || capacity < 0) return MTG_E_ARG;
    const int n = ctx->prof_n < capacity ? ctx->prof_n : capacity;
    for (int i = 0; i < n; ++i) {
        hipEvent_t *pe = &ctx->prof_ev[3 * (size_t)i];
        float a = 0.f, b = 0.f;
        HIP_TRY(ctx, hipEventSynchronize(pe[2]));
        HIP_TRY(ctx, hipEventElapsedTime(&a, pe[0], pe[1]));
        HIP_TRY(ctx, hipEventElapsedTime(&b, pe[1], pe[2]));
        if (prepare_ms) prepare_ms[i] = a;
        if (solve_ms) solve_ms[i] = b;
    }
    ctx->prof_cap = 0;
    return n;
}

MTG_API double mtg_last_kernel_ms(const mtg_ctx *ctx)
{
    if (!ctx || !ctx->timed) return -1.0;
    float ms = -1.0f;
    if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0;
    return (double)ms;
}

}  // extern "C"
