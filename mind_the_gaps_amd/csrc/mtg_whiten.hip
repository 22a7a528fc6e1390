// mtg_whiten.hip -- the one-step-ahead (whitened) residuals of a light curve under the model, q = D^-1/2 L^-1 (y - mean)
// with K = L diag(D) L^T, L = I + tril(U W^T): the exact inverse of mtg_gp_draw.hip (y = mean + L sqrt(D) q), and the
// KS and autocorrelation diagnostics of every row (mtg_whiten of include/mtg.h).  Under the model the q_n are i.i.d.
// N(0, 1), and lnL = -1/2 (q^T q + sum ln D_n + N ln 2 pi).
//
// Notation of mtg_gp_draw.hip (W normalised by D), r = y - mean(t):
//   S_n = phi_n phi_n^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),   W_n = (V_n - S_n U_n) / D_n,
//   D_n = sigma_n^2 + jitter + k(0) - U_n^T S_n U_n
//   f_n = phi_n o (f_{n-1} + W_{n-1} v_{n-1}),   v_n = r_n - U_n^T f_n,   q_n = v_n / sqrt(D_n)
// -- the forward sweep of the draw with v_n taken from the data instead of sqrt(D_n) q_n.  The phases of the generators
// are those of the elapsed time, reduced modulo 2 pi before they are rounded (mtg_elapsed_sincos).  The mean is the
// fitted constant or line of the coefficient slots; a given y, like the resident data, excludes the per-light-curve
// y_offset.  tests/whiten_replay.py is the same in numpy.
//
// mtg_whiten_kernel<J, GIVEN>: one lane per row, 64-lane workgroups, a template on the rank J (the step functions of
// mtg_factor_step.h) so that S, f and the generators live in registers: no scratch.  A lane's arithmetic reads nothing
// of its neighbours, and its eight sums (sum q, q^2, ln D, q^3, q^4, -, -, max |q|) are accumulated in sample order by
// the lane itself: a row does not depend on its position in the batch, on the slab, or on which outputs were asked for.
//
// Memory traffic: the draw's, mirrored.  A given y comes in through a tile of 64 rows x MTG_DRAW_T samples in LDS,
// transposed on its way in (one load instruction covers 64 / MTG_DRAW_T rows x MTG_DRAW_T consecutive samples), each
// lane then reading its own row at a stride of MTG_DRAW_T + 1 doubles -- odd, for the reasons at the top of
// mtg_gp_draw.hip.  q leaves through the SAME tile: lane l overwrites the y it has just read with the q of that sample,
// and the tile is written out transposed.  Without a q to store (no residuals, no KS, no ACF asked for) nothing of size
// N is stored: the kernel writes its eight sums only; the resident data are read per lane from (y, sigma^2) pairs as
// every sweep reads them.
//
// KS.  mtg_whiten_ks_kernel: one workgroup per row of the slab on a SORTED copy of the row (rocPRIM's segmented radix
// sort over the slab, keys out of place: plumbing, as in mtg_sort.hip; the caller's q is never reordered).  Against the
// standard normal, Phi(x) = 1/2 erfc(-x / sqrt 2):  D+ = max_i (i / N - Phi(q_(i))),  D- = max_i (Phi(q_(i)) - (i - 1) / N),
// i = 1 .. N.  Each lane takes i = tid + 1, tid + 257, ... and the 256 partial maxima meet in a fixed binary tree in
// LDS: the order depends on N alone (and max is exact whatever the order).
//
// ACF.  acf[k - 1] = sum_{n < N - k} q_n q_{n+k} / sum_n q_n^2, k = 1 .. K: plt.acorr's definition (no mean subtracted,
// normalised by lag 0; the denominator is the sweep's own sum).  mtg_whiten_acf_kernel: a workgroup of four waves per
// (row, block of 64 lags); lane l of every wave owns lag k0 + l; wave w sums the products of the sample chunks
// c = w, w + 4, ... (MTG_WHITEN_ACF_CHUNK samples each) in ascending n, and the four partial sums meet as
// (p0 + p1) + (p2 + p3): the order of a (row, lag) sum depends on N and k alone.  q_n is the same address for the whole
// wave and q_{n+k} 64 consecutive doubles: both come from the vector cache, the row itself (80 KB at N = 1e4) from L2.
// Cost: O(B N K) multiply-adds -- at the notebook's K = N / 4 that is 7/32 N^2 per row: 2.2e7 at N = 1e4 (4.4e10 for
// B = 2000 rows), 8.8e9 for one row of N = 2e5 -- against O(N J^2) = 1e6 for the sweep of that row; beyond N ~ 1e5 an
// FFT would win, and nothing here needs it yet.
#include "mtg_math.h"
#include "mtg_device.h"
#include "mtg_factor_step.h"

#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

template <int J, bool GIVEN>
__global__ void __launch_bounds__(64) mtg_whiten_kernel(MtgWhitenArgs a)
{
#pragma clang fp contract(off)
    constexpr int JA = J > 0 ? J : 1;
    constexpr int T = MTG_DRAW_T, TS = MTG_DRAW_TS;
    __shared__ double s_t[64 * TS];
    const int lane = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;      // first row of this workgroup in the slab
    const int64_t r = r0 + lane;
    const bool row = r < a.B;
    const int64_t e = a.row0 + (row ? r : 0);         // row of the batch
    const bool live = row && a.status[e] == MTG_ST_OK;
    const int64_t N = a.N;
    const int64_t lc = a.lc_index ? a.lc_index[e] : 0;
    const double2 *yv = a.yv + lc * N, *dxt = a.dxt + lc * a.t_stride;
    const bool store = a.q != nullptr;                // the same for every lane

    PatCoef<JA> k;
    k.asum = 0.0; k.slope = 0.0; k.icpt = 0.0;
    if (live) pat_load_row<J>(a, e, k);
    PatState<JA> sw;
    sw.reset();
    const double t_first = dxt[0].y;
    double s1 = 0.0, s2 = 0.0, sld = 0.0, s3 = 0.0, s4 = 0.0, qmax = 0.0;
    bool bad = false;

    for (int64_t n0 = 0; n0 < N; n0 += T) {
        const int nt = N - n0 < T ? (int)(N - n0) : T;
        if constexpr (GIVEN) {
            // the caller's y of samples [n0, n0 + nt) of this workgroup's rows
            mtg_tile_load(s_t, a.y, r0, a.B, N, n0, nt);
            __syncthreads();
        }
        if (live) {
            for (int j = 0; j < nt; ++j) {
                const int64_t n = n0 + j;
                double yn;
                if constexpr (GIVEN) yn = s_t[lane * TS + j];
                else yn = yv[n].x;
                const double dx = dxt[n].x, t = dxt[n].y;
                double D = yv[n].y + k.asum, uf = 0.0;
                if constexpr (J > 0) uf = sw.advance(k, dx, t, t_first, D);
                bad = bad || !(D > 0.0);
                const double v = (yn - (k.slope * t + k.icpt)) - uf;
                const double q = v / sqrt(D), q2 = q * q;
                s1 += q; s2 += q2; sld += log(D); s3 += q2 * q; s4 += q2 * q2;
                qmax = fmax(qmax, fabs(q));
                if (store) s_t[lane * TS + j] = q;
                sw.leave(D, v);
            }
        } else if (store) {
            for (int j = 0; j < nt; ++j) s_t[lane * TS + j] = NAN;
        }
        if (store) {
            __syncthreads();
            mtg_tile_store(a.q, s_t, r0, a.B, N, n0, nt);
        }
        if (GIVEN || store) __syncthreads();          // the next tile overwrites s_t
    }
    if (!row) return;
    double *st = a.stats + e * MTG_WHITEN_NSTATS;
    const bool okrow = live && !bad;
    st[0] = okrow ? s1 : NAN; st[1] = okrow ? s2 : NAN; st[2] = okrow ? sld : NAN; st[3] = okrow ? s3 : NAN;
    st[4] = okrow ? s4 : NAN; st[5] = NAN; st[6] = NAN; st[7] = okrow ? qmax : NAN;
    // a non-positive pivot is known for certain only at the end: the row reads back NaN (a rare row, stored lane-wise).
    // The tile stores to these addresses were issued by OTHER lanes of this wave: the fence orders them before the
    // overwrite, as in mtg_gp_draw_kernel.
    if (store) __threadfence();
    if (bad) {
        a.status[e] = MTG_ST_NOTPD;
        if (store)
            for (int64_t n = 0; n < N; ++n) a.q[r * N + n] = NAN;
    }
}

// ---- KS: one workgroup per row of the slab, on the sorted copy of the row ----
__global__ void __launch_bounds__(256) mtg_whiten_ks_kernel(const double *__restrict__ sorted, int64_t N, int64_t row0,
                                                             const int32_t *__restrict__ status, double *__restrict__ stats)
{
#pragma clang fp contract(off)
    __shared__ double s_p[256], s_m[256];
    const int tid = (int)threadIdx.x;
    const int64_t e = row0 + blockIdx.x;
    if (status[e] != MTG_ST_OK) return;               // the sweep has left NaN in both slots (the same for every lane)
    const double *x = sorted + (int64_t)blockIdx.x * N;
    const double dn = (double)N;
    double dp = -INFINITY, dm = -INFINITY;
    for (int64_t i = tid; i < N; i += 256) {
        const double cdf = 0.5 * erfc(-x[i] * 0.70710678118654752440);
        dp = fmax(dp, (double)(i + 1) / dn - cdf);
        dm = fmax(dm, cdf - (double)i / dn);
    }
    s_p[tid] = dp; s_m[tid] = dm;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { s_p[tid] = fmax(s_p[tid], s_p[tid + h]); s_m[tid] = fmax(s_m[tid], s_m[tid + h]); }
        __syncthreads();
    }
    if (tid == 0) { stats[e * MTG_WHITEN_NSTATS + 5] = s_p[0]; stats[e * MTG_WHITEN_NSTATS + 6] = s_m[0]; }
}

// ---- ACF: a workgroup per (row, 64 lags); grid (ceil(K / 64), rows) ----
__global__ void __launch_bounds__(256) mtg_whiten_acf_kernel(const double *__restrict__ q, int64_t N, int K, int64_t row0,
                                                              const int32_t *__restrict__ status,
                                                              const double *__restrict__ stats, double *__restrict__ acf)
{
#pragma clang fp contract(off)
    __shared__ double s_part[4][64];
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int64_t rr = blockIdx.y, e = row0 + rr;
    const int64_t kk = (int64_t)blockIdx.x * 64 + lane + 1;       // this lane's lag
    const bool ok = status[e] == MTG_ST_OK;                        // the same for the whole workgroup
    const double *x = q + rr * N;
    double sum = 0.0;
    if (ok && kk <= K) {
        const int64_t M = N - kk;                                  // products of this lag (K <= N - 1: at least one)
        for (int64_t c0 = (int64_t)w * MTG_WHITEN_ACF_CHUNK; c0 < M; c0 += 4 * MTG_WHITEN_ACF_CHUNK) {
            const int64_t c1 = c0 + MTG_WHITEN_ACF_CHUNK < M ? c0 + MTG_WHITEN_ACF_CHUNK : M;
            for (int64_t n = c0; n < c1; ++n) sum += x[n] * x[n + kk];
        }
    }
    s_part[w][lane] = sum;
    __syncthreads();
    if (w == 0 && kk <= K) {
        const double total = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
        acf[rr * K + (kk - 1)] = ok ? total / stats[e * MTG_WHITEN_NSTATS + 1] : NAN;
    }
}

namespace {

template <int J>
struct WhitenLaunch {
    static void launch(const MtgWhitenArgs &a, hipStream_t s)
    {
        const dim3 grid((unsigned)((a.B + 63) / 64)), block(64);
        if (a.y) hipLaunchKernelGGL((mtg_whiten_kernel<J, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mtg_whiten_kernel<J, false>), grid, block, 0, s, a);
    }
};

struct WhitenSegmentStart {
    unsigned N;
    __host__ __device__ unsigned operator()(unsigned b) const { return b * N; }
};
using WhitenOffsets = rocprim::transform_iterator<rocprim::counting_iterator<unsigned>, WhitenSegmentStart, unsigned>;

}  // namespace

// rows [row0, row0 + B) of the batch; J = nr0 + 2 nc0 in 0 .. MTG_MAX_J (returns 0 otherwise)
int mtg_launch_whiten(const MtgWhitenArgs &a, hipStream_t s)
{
    const int J = a.nr0 + 2 * a.nc0;
    if (J != 0) return pat_dispatch_rank<WhitenLaunch>(J, a, s);
    WhitenLaunch<0>::launch(a, s);
    return 1;
}

// temporary storage of the segmented sort of a slab of `rows` rows of N doubles (0: beyond rocPRIM's 32-bit item count)
size_t mtg_whiten_sort_temp_bytes(int64_t rows, int64_t N)
{
    if (rows * N > 0x7fffffff) return 0;
    size_t bytes = 0;
    const WhitenOffsets begin(rocprim::counting_iterator<unsigned>(0u), WhitenSegmentStart{(unsigned)N});
    (void)rocprim::segmented_radix_sort_keys(nullptr, bytes, (const double *)nullptr, (double *)nullptr, (unsigned)(rows * N),
                                             (unsigned)rows, begin, begin + 1, 0u, 64u, (hipStream_t) nullptr);
    return bytes > 0 ? bytes : 1;
}

// D+ and D- of every row of the slab into stats: q [rows][N] is sorted row by row into `sorted` (q itself is left alone)
hipError_t mtg_launch_whiten_ks(const MtgWhitenArgs &a, double *sorted, void *temp, size_t temp_bytes, hipStream_t s)
{
    if (a.B * a.N > 0x7fffffff) return hipErrorInvalidValue;
    const WhitenOffsets begin(rocprim::counting_iterator<unsigned>(0u), WhitenSegmentStart{(unsigned)a.N});
    size_t bytes = temp_bytes;
    hipError_t e = rocprim::segmented_radix_sort_keys(temp, bytes, (const double *)a.q, sorted, (unsigned)(a.B * a.N), (unsigned)a.B,
                                                      begin, begin + 1, 0u, 64u, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mtg_whiten_ks_kernel, dim3((unsigned)a.B), dim3(256), 0, s, sorted, a.N, a.row0, a.status, a.stats);
    return hipGetLastError();
}

// acf [rows][K] of the slab from q [rows][N] and the sweep's sum of squares
hipError_t mtg_launch_whiten_acf(const MtgWhitenArgs &a, int K, double *acf, hipStream_t s)
{
    if (a.B > 65535) return hipErrorInvalidValue;     // the grid's y extent: a slab is far below it (mtg_plan_whiten_slab)
    hipLaunchKernelGGL(mtg_whiten_acf_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)a.B), dim3(256), 0, s, a.q, a.N, K, a.row0,
                       a.status, a.stats, acf);
    return hipGetLastError();
}
