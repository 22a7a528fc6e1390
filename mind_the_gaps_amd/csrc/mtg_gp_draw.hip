// mtg_gp_draw.hip -- realisations of the process itself, y ~ N(mean, K) (celerite.GP.sample -> solver.dot_L), in
// O(N J^2) per draw from the semiseparable factorisation K = L diag(D) L^T, L = I + tril(U W^T): no FFT, no regular
// grid, exact for any sampling.
//
// Notation of mtg_predict_kernel (W normalised by D), q ~ N(0, I):
//   S_n = phi_n phi_n^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),   W_n = (V_n - S_n U_n) / D_n,
//   D_n = sigma_n^2 + jitter + k(0) - U_n^T S_n U_n                  (the factorisation: the data y are not read)
//   f_n = phi_n o (f_{n-1} + W_{n-1} v_{n-1}),   v_n = sqrt(D_n) q_n
//   y_n = mean(t_n) + v_n + U_n^T f_n                                 (y = mean + L sqrt(D) q)
// The phases of the generators are those of the elapsed time t_n - t_0, reduced modulo 2 pi before they are rounded
// (mtg_elapsed_sincos), never cos(d t_n) at the absolute time.  The mean is the fitted constant or line of the
// coefficient slots; the per-light-curve y_offset is left to the caller, as in mtg_predict.  tests/gp_draw_replay.py
// is the same in numpy.
//
// One lane per draw, 64-lane workgroups; a template on the rank J (as mtg_predict_at.hip, whose step functions it
// shares through mtg_factor_step.h) so that S, f and the generators live in registers: no scratch.  The split into
// NR real slots and complex pairs is a runtime value per lane (nr0 + 2 sig[e]: an SHO term on either side of Q = 1/2).
// A lane's arithmetic reads nothing of its neighbours, so a row does not depend on its position in the batch.
//
// Memory traffic.  Lane b owns row b of y[B][N] (and of the caller's normals): stored directly, a step would put 64
// lanes on 64 cache lines.  A tile of 64 rows x MTG_DRAW_T samples is staged in LDS, each lane writing its own row
// with ds_write_b64 at a row stride of MTG_DRAW_T + 1 doubles -- odd, so that the 16 lanes the LDS serves together
// land on 16 distinct bank pairs ((2 (T + 1) lane) mod 32 = 2 lane for T a multiple of 16; an even stride of 32
// doubles would put all of them on one pair) -- and is written out transposed: one store instruction covers
// 64 / MTG_DRAW_T rows x MTG_DRAW_T consecutive samples (runs of 256 bytes at T = 32), read from LDS at consecutive
// addresses.  Given normals come in the same way, transposed on their way into LDS.  T = 32: 16.5 KiB per tile, so
// four workgroups of the given-normals form (two tiles) share a compute unit's 160 KiB; T = 64 would make the runs
// 512 bytes but halve that, and the kernel lives on the latency of its recurrence, not on the stores.
//
// Device normals: Philox4x32-10 (mtg_sampler_dev.h), key = the call's seed (low word, high word), counter
//     c0 = n / 2                              sample-pair index
//     c1 = PURPOSE_GP_DRAW = 12               (1-3: the sampler; 8-10: mtg_simulate.hip; 11: mtg_e13.hip)
//     c2, c3 = low, high word of g            g = stream_base + b, the draw's index in the caller's global numbering
// One block gives u1 = 1 - u01(r0, r1) in (0, 1] and u2 = u01(r2, r3); Box-Muller: rad = sqrt(-2 ln u1),
// q_{2k} = rad cos(2 pi u2), q_{2k+1} = rad sin(2 pi u2) (sincospi).  A draw therefore depends on (seed, g, theta, its
// light curve) alone: not on B, on slabs, or on how a job is cut over GPUs (mtg_set_stream_base).
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"
#include "mtg_sampler_dev.h"

namespace {
enum { PURPOSE_GP_DRAW = 12 };
}

template <int J, bool GIVEN>
__global__ void __launch_bounds__(64) mtg_gp_draw_kernel(MtgGpDrawArgs a)
{
#pragma clang fp contract(off)
    constexpr int JA = J > 0 ? J : 1;
    constexpr int T = MTG_DRAW_T, TS = MTG_DRAW_TS;
    __shared__ double s_y[64 * TS];
    __shared__ double s_q[GIVEN ? 64 * TS : 1];
    const int lane = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;      // first row of this workgroup in the slab
    const int64_t r = r0 + lane;
    const bool row = r < a.B;
    const int64_t e = a.row0 + (row ? r : 0);         // row of the batch
    const bool live = row && a.status[e] == MTG_ST_OK;
    const int64_t N = a.N;
    const int64_t lc = a.lc_index ? a.lc_index[e] : 0;
    const double2 *yv = a.yv + lc * N, *dxt = a.dxt + lc * a.t_stride;

    PatCoef<JA> k;
    k.asum = 0.0; k.slope = 0.0; k.icpt = 0.0;
    if (live) pat_load_row<J>(a, e, k);
    PatState<JA> st;
    st.reset();
    const double t_first = dxt[0].y;
    double qa = 0.0, qb = 0.0;
    bool bad = false;
    const uint64_t g = (uint64_t)(a.draw0 + e);       // global index of this draw: random counters only

    for (int64_t n0 = 0; n0 < N; n0 += T) {
        const int nt = N - n0 < T ? (int)(N - n0) : T;
        if constexpr (GIVEN) {
            // the caller's normals of samples [n0, n0 + nt) of this workgroup's rows
            mtg_tile_load(s_q, a.normals, r0, a.B, N, n0, nt);
            __syncthreads();
        }
        if (live) {
            for (int j = 0; j < nt; ++j) {
                const int64_t n = n0 + j;
                double qn;
                if constexpr (GIVEN) {
                    qn = s_q[lane * TS + j];
                } else {
                    // T is even: pairs do not straddle tiles
                    if ((j & 1) == 0) philox_normal_pair((uint32_t)(n >> 1), PURPOSE_GP_DRAW, g, a.seed_lo, a.seed_hi, qa, qb);
                    qn = (j & 1) ? qb : qa;
                }
                const double dx = dxt[n].x, t = dxt[n].y;
                double D = yv[n].y + k.asum, uf = 0.0;
                if constexpr (J > 0) uf = st.advance(k, dx, t, t_first, D);
                bad = bad || !(D > 0.0);
                const double v = sqrt(D) * qn;
                s_y[lane * TS + j] = (k.slope * t + k.icpt) + (v + uf);
                st.leave(D, v);
            }
        } else {
            for (int j = 0; j < nt; ++j) s_y[lane * TS + j] = NAN;
        }
        __syncthreads();
        mtg_tile_store(a.y, s_y, r0, a.B, N, n0, nt);
        __syncthreads();                              // the next tile overwrites s_y (and s_q)
    }
    // a non-positive pivot is known for certain only at the end: the row reads back NaN (a rare row, stored lane-wise).
    // The tile stores to these addresses were issued by OTHER lanes of this wave, and the barrier above does not wait
    // for global stores: the fence does (device scope: every store of the wave has reached the L2 before the next one
    // is issued), so the overwrite does not rest on same-wave stores to one address retiring in order.  Once per
    // kernel, for every lane alike.
    __threadfence();
    if (row && bad) {
        a.status[e] = MTG_ST_NOTPD;
        for (int64_t n = 0; n < N; ++n) a.y[r * N + n] = NAN;
    }
}

template <int J>
struct DrawLaunch {
    static void launch(const MtgGpDrawArgs &a, hipStream_t s)
    {
        const dim3 grid((unsigned)((a.B + 63) / 64)), block(64);
        if (a.normals) hipLaunchKernelGGL((mtg_gp_draw_kernel<J, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mtg_gp_draw_kernel<J, false>), grid, block, 0, s, a);
    }
};

// rows [row0, row0 + B) of the batch; J = nr0 + 2 nc0 in 0 .. MTG_MAX_J (returns 0 otherwise)
int mtg_launch_gp_draw(const MtgGpDrawArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J != 0) return pat_dispatch_rank<DrawLaunch>(J, a, s);
    DrawLaunch<0>::launch(a, s);
    return 1;
}
