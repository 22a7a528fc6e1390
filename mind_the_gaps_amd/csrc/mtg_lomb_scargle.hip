// mtg_lomb_scargle.hip -- the generalised (floating-mean) Lomb-Scargle periodogram of every resident light curve at a
// list of frequencies (mtg_lomb_scargle of include/mtg.h): astropy's LombScargle(fit_mean=True, center_data=True,
// nterms=1).power.
//
// With weights w_n (sigma_n^-2 / sum sigma^-2, or 1 / N), ybar = sum w y, r = y - ybar, YY = sum w r^2 and
// c_n, s_n = cos, sin(2 pi f (t_n - t_0)):
//   C = sum w c, S = sum w s, YC = sum w r c, YS = sum w r s,
//   CC = sum w c^2 - C^2, SS = sum w s^2 - S^2, CS = sum w c s - C S,
//   p = (SS YC^2 + CC YS^2 - 2 CS YC YS) / (CC SS - CS^2)
// the tau-free form of Zechmeister & Kuerster (2009): algebraically astropy's YC_tau^2 / CC_tau + YS_tau^2 / SS_tau and
// invariant under a shift of the times, which is why the elapsed time t - t_0 serves and the y_offset of the resident
// set does not matter.  sum w s^2 is (sum w) - sum w c^2 with sum w = 1.
//
// Work: one (cos, sin) pair per (frequency, sample) and 2 FMAs per (frequency, sample, light curve) -- 6 when the
// weights differ from one light curve to the next.  One lane owns a frequency; a workgroup walks the samples in chunks
// of MTG_LS_CHUNK staged in LDS, every lane reading the same sample (a broadcast).  On shared sampling a lane carries
// the sums of a tile of R light curves, so that the pair is computed once per tile (and C, S, CC, CS too when the
// weights are 1 / N).
//
// Budget.  LDS: the 32 KiB (cos, sin) table, the chunk's elapsed times (2 KiB) and its (w, w r) pairs
// (R x 4 KiB weighted, R x 2 KiB unweighted): 66 KiB for R = 8 weighted / R = 16 unweighted, two workgroups of four waves
// on a CU's 160 KiB, two waves per SIMD.  Registers: the running totals and the chunk's partial sums, 2 x 6 R doubles
// weighted, 2 x (2 R + 4) unweighted, under the 256 VGPRs two waves per SIMD leave each lane (profiles/
// lomb_scargle_resources.txt; no scratch).
//
// Order.  Samples ascending; the sums of a chunk start from zero and are added to the running totals at its end.  The
// arithmetic of one (light curve, frequency) is the same sequence of operations in every instantiation, so that a
// power depends on (light curve, frequency, normalization, weighted) alone: not on L, the tile, F, the order of the
// frequencies, or on how the sampling is stored.
#include "mtg_device.h"
#include "mtg_math.h"
#include "mtg_ls_phase.h"

namespace {

// sum of v over the workgroup in a fixed order (thread-strided partial sums, then a binary tree): `red` holds
// MTG_LS_THREADS doubles
__device__ __forceinline__ double ls_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = MTG_LS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// Per light curve: sw = sum sigma^-2 (weighted) or N, ybar = sum w y, YY = sum w (y - ybar)^2 with w = sigma^-2 / sw
// or 1 / N -- stats[l] = (ybar, YY, sw, 0).  One workgroup per light curve, sums in an order that depends on N alone.
__global__ void __launch_bounds__(MTG_LS_THREADS)
mtg_lomb_scargle_stats_kernel(const double2 *__restrict__ yv, int64_t N, int weighted, double4 *__restrict__ stats)
{
#pragma clang fp contract(off)
    __shared__ double red[MTG_LS_THREADS];
    const int64_t l = blockIdx.x;
    const double2 *row = yv + l * N;
    const int tid = threadIdx.x;
    double sw = (double)N;
    if (weighted) {
        double a = 0.0;
        for (int64_t n = tid; n < N; n += MTG_LS_THREADS) a += 1.0 / row[n].y;
        sw = ls_block_sum(a, red);
    }
    double a = 0.0;
    for (int64_t n = tid; n < N; n += MTG_LS_THREADS) {
        const double2 v = row[n];
        const double w = weighted ? (1.0 / v.y) / sw : 1.0 / sw;
        a = __builtin_fma(w, v.x, a);
    }
    const double ybar = ls_block_sum(a, red);
    a = 0.0;
    for (int64_t n = tid; n < N; n += MTG_LS_THREADS) {
        const double2 v = row[n];
        const double w = weighted ? (1.0 / v.y) / sw : 1.0 / sw;
        const double r = v.x - ybar;
        a = __builtin_fma(w * r, r, a);
    }
    const double yy = ls_block_sum(a, red);
    if (tid == 0) stats[l] = make_double4(ybar, yy, sw, 0.0);
}

struct MtgLsArgs {
    const double2 *dxt, *yv;
    int64_t N, t_stride;     // 0 (shared sampling) or N
    int64_t l0, Ls;          // this launch takes light curves [l0, l0 + Ls)
    const double4 *stats;    // [L]
    int64_t F;
    const double *freqs;     // [F]
    int nfb;                 // workgroups along the frequencies
    int normalization;
    double *power;           // [Ls][F] of this slab
};

// the trig part of a lane's sums: C, S, sum w c^2, sum w c s
struct LsTrig {
    double c, s, cc, cs;
    __device__ __forceinline__ void zero() { c = s = cc = cs = 0.0; }
    __device__ __forceinline__ void add(double w, double co, double si)
    {
        const double wc = w * co;
        c = __builtin_fma(w, co, c);
        s = __builtin_fma(w, si, s);
        cc = __builtin_fma(wc, co, cc);
        cs = __builtin_fma(wc, si, cs);
    }
    __device__ __forceinline__ void fold(const LsTrig &o) { c += o.c; s += o.s; cc += o.cc; cs += o.cs; }
};

// R light curves per lane; WEIGHTED: weights from the light curve's own sigma (its trig sums are its own), else 1 / N
// (the trig sums are the tile's).  LDS chunk: te[CHUNK], then WEIGHTED (w, w r)[R][CHUNK], else w r as pairs of light
// curves (2j, 2j + 1)[R / 2][CHUNK] (R = 1: [CHUNK] doubles) -- one ds_read_b128 per two sums either way.
template <int R, bool WEIGHTED>
__global__ void __launch_bounds__(MTG_LS_THREADS, 2)
mtg_lomb_scargle_kernel(const MtgLsArgs a)
{
#pragma clang fp contract(off)
    constexpr int CH = MTG_LS_CHUNK;
    constexpr int NT = WEIGHTED ? R : 1;               // trig sums kept per lane
    constexpr int NP = WEIGHTED ? R : (R + 1) / 2;     // 16-byte (R = 1 unweighted: 8-byte) columns of the chunk
    __shared__ MtgLsTab tab;
    __shared__ double te_s[CH];
    __shared__ double2 col_s[NP * CH];

    const int tid = threadIdx.x, nth = blockDim.x;
    mtg_ls_fill_tab(&tab);
    const int64_t tile = blockIdx.x / a.nfb;
    const int fb = (int)(blockIdx.x - tile * a.nfb);
    const int64_t lt = a.l0 + tile * R;                 // first light curve of the tile
    const int nl = (int)(a.l0 + a.Ls - lt < R ? a.l0 + a.Ls - lt : R);   // light curves in it
    const int64_t k = (int64_t)fb * nth + tid;
    const double f = a.freqs[k < a.F ? k : a.F - 1];    // (idle lanes repeat the last frequency and store nothing)
    const double2 *dxt = a.dxt + lt * a.t_stride;
    const double t0 = dxt[0].y;
    const double w0 = 1.0 / (double)a.N;

    LsTrig tt[NT];
    double tyc[R], tys[R];
#pragma unroll
    for (int i = 0; i < NT; ++i) tt[i].zero();
#pragma unroll
    for (int i = 0; i < R; ++i) tyc[i] = tys[i] = 0.0;

    for (int64_t n0 = 0; n0 < a.N; n0 += CH) {
        const int len = (int)(a.N - n0 < CH ? a.N - n0 : CH);
        __syncthreads();   // the previous chunk has been read (first trip: nothing)
        for (int i = tid; i < len; i += nth) te_s[i] = dxt[n0 + i].y - t0;
        if (WEIGHTED) {
            for (int e = tid; e < R * CH; e += nth) {
                const int j = e / CH, i = e - j * CH;
                if (i >= len) continue;
                double2 o = make_double2(0.0, 0.0);    // a light curve beyond the tile adds zeros and is not stored
                if (j < nl) {
                    const double4 st = a.stats[lt + j];
                    const double2 v = a.yv[(lt + j) * a.N + n0 + i];
                    const double w = (1.0 / v.y) / st.z;
                    o = make_double2(w, w * (v.x - st.x));
                }
                col_s[j * CH + i] = o;
            }
        } else if (R == 1) {
            const double ybar = a.stats[lt].x;
            double *col = reinterpret_cast<double *>(col_s);
            for (int i = tid; i < len; i += nth) col[i] = w0 * (a.yv[lt * a.N + n0 + i].x - ybar);
        } else {
            for (int e = tid; e < NP * CH; e += nth) {
                const int j = e / CH, i = e - j * CH;
                if (i >= len) continue;
                double2 o = make_double2(0.0, 0.0);
                if (2 * j < nl) o.x = w0 * (a.yv[(lt + 2 * j) * a.N + n0 + i].x - a.stats[lt + 2 * j].x);
                if (2 * j + 1 < nl) o.y = w0 * (a.yv[(lt + 2 * j + 1) * a.N + n0 + i].x - a.stats[lt + 2 * j + 1].x);
                col_s[j * CH + i] = o;
            }
        }
        __syncthreads();

        LsTrig pt[NT];
        double pyc[R], pys[R];
#pragma unroll
        for (int i = 0; i < NT; ++i) pt[i].zero();
#pragma unroll
        for (int i = 0; i < R; ++i) pyc[i] = pys[i] = 0.0;
        for (int i = 0; i < len; ++i) {
            double si, co;
            mtg_cycles_sincos(f, te_s[i], &si, &co, &tab);
            if (WEIGHTED) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const double2 v = col_s[j * CH + i];
                    pt[j].add(v.x, co, si);
                    pyc[j] = __builtin_fma(v.y, co, pyc[j]);
                    pys[j] = __builtin_fma(v.y, si, pys[j]);
                }
            } else {
                pt[0].add(w0, co, si);
                if (R == 1) {
                    const double v = reinterpret_cast<const double *>(col_s)[i];
                    pyc[0] = __builtin_fma(v, co, pyc[0]);
                    pys[0] = __builtin_fma(v, si, pys[0]);
                } else {
#pragma unroll
                    for (int j = 0; j < R / 2; ++j) {
                        const double2 v = col_s[j * CH + i];
                        pyc[2 * j] = __builtin_fma(v.x, co, pyc[2 * j]);
                        pys[2 * j] = __builtin_fma(v.x, si, pys[2 * j]);
                        pyc[2 * j + 1] = __builtin_fma(v.y, co, pyc[2 * j + 1]);
                        pys[2 * j + 1] = __builtin_fma(v.y, si, pys[2 * j + 1]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) tt[i].fold(pt[i]);
#pragma unroll
        for (int i = 0; i < R; ++i) { tyc[i] += pyc[i]; tys[i] += pys[i]; }
    }

    if (k >= a.F) return;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= nl) continue;
        const LsTrig &g = tt[WEIGHTED ? j : 0];
        const double4 st = a.stats[lt + j];
        const double CC = g.cc - g.c * g.c, SS = (1.0 - g.cc) - g.s * g.s, CS = g.cs - g.c * g.s;
        const double YC = tyc[j], YS = tys[j], YY = st.y;
        const double det = CC * SS - CS * CS;
        const double num = (SS * YC) * YC + (CC * YS) * YS - 2.0 * ((CS * YC) * YS);
        double out = __builtin_nan("");
        if (det > 0.0) {
            const double p = num / det;
            switch (a.normalization) {
            case MTG_LS_STANDARD: out = p / YY; break;
            case MTG_LS_MODEL: out = p / (YY - p); break;
            case MTG_LS_LOG: out = -log(1.0 - p / YY); break;
            default: out = p * (0.5 * st.z); break;   // MTG_LS_PSD
            }
        }
        a.power[(lt - a.l0 + j) * a.F + k] = out;
    }
}

// the largest entry of every row of power[Ls][F] and the first index that attains it; NaN entries are passed over (a
// row of nothing else: NaN and -1).  One workgroup per row.
__global__ void __launch_bounds__(MTG_LS_THREADS)
mtg_lomb_scargle_peak_kernel(const double *__restrict__ power, int64_t F, double *__restrict__ peak, int64_t *__restrict__ index)
{
    __shared__ double bv[MTG_LS_THREADS];
    __shared__ int64_t bi[MTG_LS_THREADS];
    const double *row = power + (int64_t)blockIdx.x * F;
    const int tid = threadIdx.x;
    double v = 0.0;
    int64_t at = -1;
    for (int64_t k = tid; k < F; k += MTG_LS_THREADS) {
        const double x = row[k];
        if (x == x && (at < 0 || x > v)) { v = x; at = k; }
    }
    bv[tid] = v; bi[tid] = at;
    __syncthreads();
    for (int h = MTG_LS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double x = bv[tid + h];
            const int64_t xi = bi[tid + h];
            if (xi >= 0 && (bi[tid] < 0 || x > bv[tid] || (x == bv[tid] && xi < bi[tid]))) { bv[tid] = x; bi[tid] = xi; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (peak) peak[blockIdx.x] = bi[0] < 0 ? __builtin_nan("") : bv[0];
        if (index) index[blockIdx.x] = bi[0];
    }
}

template <int R, bool WEIGHTED>
void ls_launch(const MtgLsArgs &a, int64_t blocks, int threads, hipStream_t s)
{
    hipLaunchKernelGGL((mtg_lomb_scargle_kernel<R, WEIGHTED>), dim3((unsigned)blocks), dim3(threads), 0, s, a);
}

// the peaks of the slab's rows, where asked for
void ls_launch_peaks(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, hipStream_t s)
{
    if (q.peak_power || q.peak_index)
        hipLaunchKernelGGL(mtg_lomb_scargle_peak_kernel, dim3((unsigned)Ls), dim3(MTG_LS_THREADS), 0, s, q.power, q.F,
                           q.peak_power ? q.peak_power + l0 : nullptr, q.peak_index ? q.peak_index + l0 : nullptr);
}

}  // namespace

int mtg_lomb_scargle_tile(int64_t L, int shared_sampling, int weighted)
{
    if (!shared_sampling || L <= 1) return 1;
    if (L <= 4) return 4;
    return weighted ? MTG_LS_R_WEIGHTED : MTG_LS_R_UNWEIGHTED;
}

void mtg_launch_lomb_scargle_stats(const MtgLombScargleArgs &q, hipStream_t s)
{
    hipLaunchKernelGGL(mtg_lomb_scargle_stats_kernel, dim3((unsigned)q.L), dim3(MTG_LS_THREADS), 0, s, q.yv, q.N, q.weighted,
                       reinterpret_cast<double4 *>(q.stats));
}

int mtg_launch_lomb_scargle(const MtgLombScargleArgs &q, int64_t l0, int64_t Ls, hipStream_t s)
{
    if (q.nterms > 1) {   // the powers with harmonics come from mtg_lomb_scargle_multi.hip; the peaks are reduced here
        if (!mtg_launch_lomb_scargle_multi_powers(q, l0, Ls, s)) return 0;
        ls_launch_peaks(q, l0, Ls, s);
        return 1;
    }
    const int R = mtg_lomb_scargle_tile(q.L, q.t_stride == 0, q.weighted);
    // narrow frequency lists leave most of a wide workgroup idle: one or two waves then (the arithmetic of a lane is the same)
    const int threads = q.F <= 64 ? 64 : q.F <= 128 ? 128 : MTG_LS_THREADS;
    const int64_t nfb = (q.F + threads - 1) / threads, tiles = (Ls + R - 1) / R;
    if (nfb > 0x7fffffff / tiles) return 0;
    MtgLsArgs a;
    a.dxt = q.dxt; a.yv = q.yv; a.N = q.N; a.t_stride = q.t_stride; a.l0 = l0; a.Ls = Ls;
    a.stats = reinterpret_cast<const double4 *>(q.stats); a.F = q.F; a.freqs = q.freqs; a.nfb = (int)nfb;
    a.normalization = q.normalization; a.power = q.power;
    const int64_t blocks = nfb * tiles;
    if (q.weighted) {
        if (R == 1) ls_launch<1, true>(a, blocks, threads, s);
        else if (R == 4) ls_launch<4, true>(a, blocks, threads, s);
        else ls_launch<MTG_LS_R_WEIGHTED, true>(a, blocks, threads, s);
    } else {
        if (R == 1) ls_launch<1, false>(a, blocks, threads, s);
        else if (R == 4) ls_launch<4, false>(a, blocks, threads, s);
        else ls_launch<MTG_LS_R_UNWEIGHTED, false>(a, blocks, threads, s);
    }
    ls_launch_peaks(q, l0, Ls, s);
    return 1;
}
