// mtg_lomb_scargle_envelope.hip -- reductions ACROSS the light curves of a slab of Lomb-Scargle powers
// (mtg_lomb_scargle_envelope of include/mtg.h).  The powers themselves are mtg_lomb_scargle.hip's, untouched: the driver
// calls mtg_launch_lomb_scargle on a slab of frequencies for all L light curves, power[L][Fs], and this unit reduces
//   * down every column: the elements of given ranks of the column sorted ascending with NaN last, the number of
//     entries that are not NaN, and the number at or above a reference;
//   * along every row: the running (maximum, first index) of power / scale, carried from slab to slab.
//
// Order.  A double becomes a 64-bit key whose unsigned order is the order of the doubles: sign bit flipped for
// non-negative values, all bits for negative ones; every NaN becomes the one key above +inf.  Keys of equal value are
// indistinguishable, so the sorted column -- and with it every output -- depends on the column as a multiset: not on the
// order of the light curves, the slab, or the neighbours a workgroup carries.  (-0 sorts below +0 where numpy leaves
// their order open; the two compare equal.)  The counts compare the doubles themselves (x == x, x >= reference).
//
// LDS path (L <= MTG_LSE_LDS_KEYS).  A workgroup of MTG_LSE_THREADS carries C = mtg_lse_columns(L) neighbouring columns,
// each padded with the NaN key to Lp = 2^ceil(log2 L) keys: C Lp <= 16384 keys, 128 KiB, one workgroup per CU, two waves
// per SIMD.  Rows of the slab are read as runs of C doubles (lane c of a run takes column c); a bitonic network sorts
// all C columns at once, a compare-exchange per lane and step with the pairs of a column on neighbouring lanes
// (consecutive 8-byte LDS addresses).  Registers: a few dozen, no scratch (profiles/lomb_scargle_envelope_resources.txt).
//
// Beyond (L > MTG_LSE_LDS_KEYS).  The slab is transposed into keys [Fs][L] through a 32 x 33 LDS tile, rocPRIM's segmented
// radix sort orders every column (plumbing, as in mtg_sort.hip), and a lane per column reads the ranks and finds the two
// counts by binary search in the sorted keys.
#include "mtg_device.h"
#include "mtg_ls_envelope_plan.h"
#include "mtg_ls_peak.h"

#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

typedef unsigned long long lse_key;
#define MTG_LSE_NAN_KEY (~0ull)

__device__ __forceinline__ lse_key lse_encode(double x)
{
    if (!(x == x)) return MTG_LSE_NAN_KEY;
    const lse_key u = (lse_key)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double lse_decode(lse_key k)
{
    if (k == MTG_LSE_NAN_KEY) return __builtin_nan("");
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct LseColumnArgs {
    const double *slab;          // [L][Fs]
    int64_t L, Fs, k0;           // k0: the slab's first column among the call's F
    int Lp, logLp, C, logC;      // padded column, columns per workgroup (powers of two)
    int Q;
    const int64_t *ranks;        // [Q]
    double *order_stat;          // [Q][Fs]
    int64_t *valid;              // [F] or NULL
    const double *reference;     // [F] or NULL
    int64_t *exceed;             // [F] or NULL
};

__global__ void __launch_bounds__(MTG_LSE_THREADS)
mtg_ls_envelope_column_kernel(const LseColumnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) lse_key keys[];   // [C][Lp]
    __shared__ unsigned n_valid[MTG_LSE_MAX_COLS], n_exceed[MTG_LSE_MAX_COLS];
    constexpr int T = MTG_LSE_THREADS;
    const int tid = threadIdx.x, C = a.C, Lp = a.Lp;
    const int64_t kb = (int64_t)blockIdx.x * C;      // the workgroup's first column of the slab
    const int total = C << a.logLp;

    for (int e = tid; e < total; e += T) keys[e] = MTG_LSE_NAN_KEY;   // the padding, and columns beyond the slab
    if (tid < MTG_LSE_MAX_COLS) n_valid[tid] = n_exceed[tid] = 0u;
    __syncthreads();

    // T is a multiple of C: a lane stays on one column
    const int c = tid & (C - 1);
    const int64_t k = kb + c;
    if (k < a.Fs) {
        const bool cmp = a.reference != nullptr;
        const double ref = cmp ? a.reference[a.k0 + k] : 0.0;
        unsigned nv = 0u, ne = 0u;
        for (int64_t l = tid >> a.logC; l < a.L; l += T >> a.logC) {
            const double x = a.slab[l * a.Fs + k];
            nv += x == x ? 1u : 0u;
            ne += (cmp && x >= ref) ? 1u : 0u;
            keys[(c << a.logLp) + (int)l] = lse_encode(x);
        }
        atomicAdd(&n_valid[c], nv);
        atomicAdd(&n_exceed[c], ne);
    }
    __syncthreads();

    // bitonic network over every column at once: pair p of the C Lp / 2 belongs to column p / (Lp / 2)
    const int half = total >> 1;
    for (int kk = 2; kk <= Lp; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < half; p += T) {
                const int col = p >> (a.logLp - 1), q = p & ((Lp >> 1) - 1);
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));   // bit j clear
                lse_key *kc = keys + (col << a.logLp);
                const lse_key x = kc[i], y = kc[i | j];
                const bool up = (i & kk) == 0;
                if ((x > y) == up) { kc[i] = y; kc[i | j] = x; }
            }
            __syncthreads();
        }
    }

    for (int e = tid; e < a.Q << a.logC; e += T) {
        const int q = e >> a.logC, cc = e & (C - 1);
        if (kb + cc < a.Fs) a.order_stat[(int64_t)q * a.Fs + kb + cc] = lse_decode(keys[(cc << a.logLp) + (int)a.ranks[q]]);
    }
    if (tid < C && kb + tid < a.Fs) {
        if (a.valid) a.valid[a.k0 + kb + tid] = (int64_t)n_valid[tid];
        if (a.exceed) a.exceed[a.k0 + kb + tid] = (int64_t)n_exceed[tid];
    }
}

// keys[k][l] = key(slab[l][k]): 32 x 32 tiles, block (32, 8)
__global__ void __launch_bounds__(256)
mtg_ls_envelope_transpose_kernel(const double *__restrict__ slab, int64_t L, int64_t Fs, lse_key *__restrict__ keys)
{
    __shared__ lse_key tile[32][33];
    const int64_t lt = (int64_t)blockIdx.x * 32, kt = (int64_t)blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int64_t l = lt + r, k = kt + threadIdx.x;
        if (l < L && k < Fs) tile[r][threadIdx.x] = lse_encode(slab[l * Fs + k]);
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int64_t k = kt + r, l = lt + threadIdx.x;
        if (k < Fs && l < L) keys[k * L + l] = tile[threadIdx.x][r];
    }
}

// first index in sorted[0, n) whose key is not below `key`
__device__ __forceinline__ int64_t lse_lower_bound(const lse_key *sorted, int64_t n, lse_key key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a lane per column of the sorted keys [Fs][L]
__global__ void __launch_bounds__(256)
mtg_ls_envelope_select_kernel(const lse_key *__restrict__ sorted, const LseColumnArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.Fs) return;
    const lse_key *col = sorted + k * a.L;
    for (int q = 0; q < a.Q; ++q) a.order_stat[(int64_t)q * a.Fs + k] = lse_decode(col[a.ranks[q]]);
    if (!a.valid && !a.exceed) return;
    const int64_t nv = lse_lower_bound(col, a.L, MTG_LSE_NAN_KEY);
    if (a.valid) a.valid[a.k0 + k] = nv;
    if (a.exceed) {
        const double ref = a.reference[a.k0 + k];
        // x >= +-0 holds for both zeros: count from the key of -0
        a.exceed[a.k0 + k] = nv - lse_lower_bound(col, nv, lse_encode(ref == 0.0 ? -0.0 : ref));
    }
}

// Per light curve the largest power / scale of the slab and the first column that attains it (NaN passed over), folded
// into the running pair of the slabs before it: a later slab wins only with a strictly larger ratio.  One workgroup per row.
__global__ void __launch_bounds__(256)
mtg_ls_envelope_ratio_peak_kernel(const double *__restrict__ slab, int64_t Fs, int64_t k0, const double *__restrict__ scale,
                                  double *__restrict__ peak, int64_t *__restrict__ index)
{
    const double *row = slab + (int64_t)blockIdx.x * Fs;
    const double *by = scale + k0;
    double v;
    int64_t at;
    ls_block_peak<256>(Fs, [row, by](int64_t k) { return row[k] / by[k]; }, &v, &at);
    if (threadIdx.x == 0) {
        if (at >= 0) at += k0;
        if (k0 > 0) {
            const int64_t before = index[blockIdx.x];
            if (before >= 0 && !(at >= 0 && v > peak[blockIdx.x])) { v = peak[blockIdx.x]; at = before; }
        }
        peak[blockIdx.x] = at < 0 ? __builtin_nan("") : v;
        index[blockIdx.x] = at;
    }
}

struct LseSegmentStart {
    unsigned L;
    __host__ __device__ unsigned operator()(unsigned k) const { return k * L; }
};
using LseOffsets = rocprim::transform_iterator<rocprim::counting_iterator<unsigned>, LseSegmentStart, unsigned>;

int lse_log2(int64_t p)
{
    int n = 0;
    while (((int64_t)1 << n) < p) ++n;
    return n;
}

LseColumnArgs lse_column_args(const MtgLsEnvelopeArgs &q)
{
    LseColumnArgs a;
    a.slab = q.slab; a.L = q.L; a.Fs = q.Fs; a.k0 = q.k0;
    a.Lp = a.logLp = a.C = a.logC = 0;
    a.Q = q.Q; a.ranks = q.ranks; a.order_stat = q.order_stat;
    a.valid = q.valid; a.reference = q.reference; a.exceed = q.exceed;
    return a;
}

}  // namespace

size_t mtg_ls_envelope_temp_bytes(int64_t L, int64_t Fs)
{
    if (mtg_lse_in_lds(L) || L * Fs > 0x7fffffff) return 0;
    size_t bytes = 0;
    rocprim::double_buffer<lse_key> keys(nullptr, nullptr);
    const LseOffsets begin(rocprim::counting_iterator<unsigned>(0u), LseSegmentStart{(unsigned)L});
    (void)rocprim::segmented_radix_sort_keys(nullptr, bytes, keys, (unsigned)(L * Fs), (unsigned)Fs, begin, begin + 1, 0u, 64u,
                                             (hipStream_t) nullptr);
    return bytes;
}

hipError_t mtg_launch_ls_envelope_columns(const MtgLsEnvelopeArgs &q, hipStream_t s)
{
    LseColumnArgs a = lse_column_args(q);
    if (mtg_lse_in_lds(q.L)) {
        a.Lp = (int)mtg_lse_pow2(q.L); a.logLp = lse_log2(a.Lp);
        a.C = mtg_lse_columns(q.L); a.logC = lse_log2(a.C);
        const int64_t blocks = (q.Fs + a.C - 1) / a.C;
        const size_t lds = (size_t)a.C * (size_t)a.Lp * sizeof(lse_key);
        if (blocks > 0x7fffffff) return hipErrorInvalidValue;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mtg_ls_envelope_column_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MTG_LSE_LDS_KEYS * sizeof(lse_key)));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(mtg_ls_envelope_column_kernel, dim3((unsigned)blocks), dim3(MTG_LSE_THREADS), lds, s, a);
        return hipGetLastError();
    }
    // (rocPRIM counts segments' items in 32 bits; a slab within the budget is far below that)
    if (q.L * q.Fs > 0x7fffffff || (q.Fs + 31) / 32 > 65535) return hipErrorInvalidValue;
    lse_key *ka = reinterpret_cast<lse_key *>(q.keys_a), *kb = reinterpret_cast<lse_key *>(q.keys_b);
    hipLaunchKernelGGL(mtg_ls_envelope_transpose_kernel, dim3((unsigned)((q.L + 31) / 32), (unsigned)((q.Fs + 31) / 32)), dim3(32, 8), 0, s,
                       q.slab, q.L, q.Fs, ka);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    rocprim::double_buffer<lse_key> keys(ka, kb);
    const LseOffsets begin(rocprim::counting_iterator<unsigned>(0u), LseSegmentStart{(unsigned)q.L});
    size_t bytes = q.temp_bytes;
    e = rocprim::segmented_radix_sort_keys(q.temp, bytes, keys, (unsigned)(q.L * q.Fs), (unsigned)q.Fs, begin, begin + 1, 0u, 64u, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mtg_ls_envelope_select_kernel, dim3((unsigned)((q.Fs + 255) / 256)), dim3(256), 0, s, keys.current(), a);
    return hipGetLastError();
}

hipError_t mtg_launch_ls_envelope_ratio_peaks(const MtgLsEnvelopeArgs &q, hipStream_t s)
{
    hipLaunchKernelGGL(mtg_ls_envelope_ratio_peak_kernel, dim3((unsigned)q.L), dim3(256), 0, s, q.slab, q.Fs, q.k0, q.scale,
                       q.peak_ratio, q.peak_ratio_index);
    return hipGetLastError();
}
