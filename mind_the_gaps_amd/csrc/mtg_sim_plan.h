// mtg_sim_plan.h -- how a TK95 simulation is cut into transforms, and which cached hipFFT plan serves it, decided from
// shapes alone: mtg_capi.hip's mtg_simulate_tk95 and mtg_simulate_plan ask mtg_sim_layout and follow it; the convergence
// check asks mtg_acf_slot_choose for its plan slot.  Plain C++17 without HIP, so that the rules can be read in one place
// and run on the host (tests/sim_plan_driver.cpp).
#pragma once
#include <stdint.h>

#include <initializer_list>

// transforms per execution of the simulator's hipFFT plan (lengths hipFFT transforms natively; the others take the
// chirp-z path below): a function of the length alone for a full call, so that one plan serves every such call (16
// transforms of 10^6 points fill the GPU; short transforms are batched by the hundred; `forced` > 0 overrides: the
// MTG_SIM_BATCH of a measuring build, read by the caller) -- as long as the spectrum and series buffers of one execution,
// 16 nk + 8 nfft bytes per transform, stay within 2 GiB.  A call of fewer series than that (Simulator.generate_lightcurve()
// asks for ONE) gets a plan of its own size in the context's second slot: no transforms of empty slots, and a native plan
// costs milliseconds to build.
static inline int mtg_sim_batch_for(int64_t nfft, int64_t S = INT64_MAX, int forced = 0)
{
    int64_t b = ((int64_t)1 << 24) / nfft;
    b = b < 16 ? 16 : b > 256 ? 256 : b;
    if (forced > 0) b = forced;
    const int64_t fit = ((int64_t)1 << 31) / (16 * (nfft / 2 + 1) + 8 * nfft);
    if (b > fit) b = fit;
    if (b > S) b = S;   // fewer series than a full batch: no transforms of empty slots
    return (int)(b < 1 ? 1 : b);
}

// ---- the chirp-z path (mtg_simulate.hip) ----
static inline int64_t mtg_czt_length(int64_t nfft)
{
    int64_t m = 1;
    while (m < 2 * nfft - 1) m <<= 1;
    return m;
}
// lengths hipFFT transforms natively (radices 2 .. 13) keep its Z2D plan; anything with a larger prime factor goes through
// power-of-two transforms -- while one pair's work area (16 m bytes) stays within 2 GiB.  sim_transform
// (mtg_set_simulate_transform) forces one or the other (1: the library's plan, 2: chirp-z).
static inline bool mtg_sim_wants_czt(int sim_transform, int64_t nfft)
{
    if (sim_transform == 1) return false;
    if (sim_transform == 2) return mtg_czt_length(nfft) * 16 <= ((int64_t)1 << 31);
    int64_t r = nfft;
    for (int64_t f : {2, 3, 5, 7, 11, 13})
        while (r % f == 0) r /= f;
    return r > 1 && mtg_czt_length(nfft) * 16 <= ((int64_t)1 << 31);
}
// complex transforms per execution (each carries `per` = 2 series, or 1 with pairing off): up to 1 GiB of work area, no more
// than the call needs
static inline int mtg_czt_pairs_for(int64_t m, int64_t S = INT64_MAX, int per = 2)
{
    int64_t pairs = ((int64_t)1 << 30) / (m * 16);
    pairs = pairs < 1 ? 1 : pairs > 128 ? 128 : pairs;
    const int64_t need = S == INT64_MAX ? pairs : (S + per - 1) / per;
    return (int)(pairs < need ? pairs : need);
}

// Everything a call of S series on a grid of nfft points follows (S = INT64_MAX: a full call, what mtg_simulate_plan
// prepares).  The simulations go through the plan `chunk` at a time; the last group may be short.
struct MtgSimLayout {
    bool czt;        // chirp-z on power-of-two Z2Z transforms, else hipFFT's own Z2D plan of length nfft
    int64_t m;       // chirp-z: length of the complex transforms (0 otherwise)
    int per;         // chirp-z: series per complex transform (2, or 1 with pairing off)
    int batch;       // transforms per execution of the plan: complex ones (pairs) for chirp-z, real ones otherwise
    int64_t chunk;   // series per execution: per * batch for chirp-z, batch otherwise
    int slot;        // of the two cached plans: 0 the bulk plan of a length (the batch of a full call), 1 a short call's --
                     // a short call never evicts the bulk plan
    int64_t spec_bytes, series_bytes, work_bytes;   // spectra [chunk][nfft / 2 + 1] complex, series [chunk][nfft], and the
                                                    // chirp-z work area [batch][m] complex (0 otherwise)
};

static inline MtgSimLayout mtg_sim_layout(int64_t nfft, int64_t S, int sim_transform, bool pairs_on, int forced_batch = 0)
{
    MtgSimLayout l;
    l.czt = mtg_sim_wants_czt(sim_transform, nfft);
    l.m = l.czt ? mtg_czt_length(nfft) : 0;
    l.per = pairs_on ? 2 : 1;
    if (l.czt) {
        l.batch = mtg_czt_pairs_for(l.m, S, l.per);
        l.chunk = l.per * (int64_t)l.batch;
        l.slot = l.batch == mtg_czt_pairs_for(l.m) ? 0 : 1;
    } else {
        l.batch = mtg_sim_batch_for(nfft, S, forced_batch);
        l.chunk = l.batch;
        l.slot = l.batch == mtg_sim_batch_for(nfft, INT64_MAX, forced_batch) ? 0 : 1;
    }
    l.spec_bytes = l.chunk * (nfft / 2 + 1) * 16;
    l.series_bytes = l.chunk * nfft * 8;
    l.work_bytes = l.czt ? l.batch * l.m * 16 : 0;
    return l;
}

// ---- the convergence check's plan pairs (mtg_chain_autocorr): four slots, keyed by the transforms' shape ----
#define MTG_ACF_SLOTS 4
struct MtgAcfSlot {
    bool have;
    int64_t n2, S, P;   // padded length, forward and inverse batch
    uint64_t used;      // the context's clock at the slot's last use
};
// The slot for a check of shape (n2, S, P): the one that holds it (*hit = true), else an empty one, else the least
// recently used -- which the caller remakes.
static inline int mtg_acf_slot_choose(const MtgAcfSlot (&slots)[MTG_ACF_SLOTS], int64_t n2, int64_t S, int64_t P, bool *hit)
{
    int at = -1;
    for (int i = 0; i < MTG_ACF_SLOTS; ++i)
        if (slots[i].have && slots[i].n2 == n2 && slots[i].S == S && slots[i].P == P) at = i;
    *hit = at >= 0;
    if (*hit) return at;
    at = 0;
    for (int i = 0; i < MTG_ACF_SLOTS; ++i)
        if (!slots[i].have || (slots[at].have && slots[i].used < slots[at].used)) at = i;
    return at;
}
