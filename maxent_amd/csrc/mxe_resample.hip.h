// mxe_resample.hip.h -- jackknife / bootstrap resampling of binned Monte Carlo data (no counterpart in the reference)
//
//   bins, a table of multiplicities counts[r][b]   ->  the rotated data of every resample   bins_resample_kernel
//   the H rows the resamples were continued to     ->  mean, spread, functional covariances  resample_reduce_kernel
//   the same rows (resamples, or the mocks of a parametric bootstrap)  ->  percentile bands   rows_finite_kernel, resample_quantile_kernel
//
// bins_resample_kernel: one workgroup of 16 wavefronts per set, all sets in one launch.
//   1. mean over the bins: bins_mean of mxe_bins.hip.h, the code bins_eig_kernel runs -- the same bits.
//   2. deviations  D[r] = sum_b counts[r][b] (bins[b] - mean) / N_r,  N_r = sum_b counts[r][b].  A resampled mean is only
//      ever mean + D[r]: the spread of the resamples is made of the D, which are ~1/n_bins of the data, and a sum of raw
//      bins would leave them with the absolute rounding error of the data.  (n_res x n_bins) (n_bins x n_data) as
//      v_mfma_f64_16x16x4_f64 tiles: a wavefront owns a tile column and up to RS_RT tile rows and runs over ALL bins in
//      index order, so no sum is split between wavefronts; the integer multiplicities are exact, the one division by N_r
//      comes last.  Edges are padded with zeros in the operands.
//   3. T mean (one wavefront per row of T, lanes over the columns, butterfly sum), then dev = D T^T by the same tiles,
//      G = T mean + dev; rows k >= rank are written as zeros.
// A set's output depends on nothing but its own bins, T and rank and on the shared table: it is the same bits alone or
// in a batch, and from call to call.
//
// resample_reduce_kernel: one workgroup (4 wavefronts) per group of rows.
//   1. per row (one wavefront each): is it finite -- a failed alpha leaves NaN --, and its functional values F H_row
//      (lanes over omega, butterfly sum: fixed order).
//   2. per omega point one thread: the mean over the finite rows in row order, then scale * sum (H_r - mean)^2 in a second
//      pass; the same for the functional values and their covariance.  Fewer than two finite rows: NaN variances.
// No atomics, no sum whose order depends on the launch: a group's bits do not depend on the other groups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_bins.hip.h"

namespace mxe {

constexpr int RS_RT = 4;                 // tile rows (of 16 resamples) a wavefront carries through one sweep over the bins

struct ResampleParams {
    int m;                   // n_bins
    int n;                   // n_data
    int n_res;
    const double* bins;      // [set][m][n]
    const int* counts;       // [n_res][m]
    const double* Nr;        // [n_res]  row sums of counts
    const double* T;         // [set][n][n]
    const int* rank;         // [set]
    double* part;            // [set][BINS_NWAVE][n][2]  partial sums of the mean
    double* D;               // [set][n_res][n]  deviations before the rotation
    double* out_mean;        // [set][n]
    double* out_G;           // [set][n_res][n]
    double* out_dev;         // [set][n_res][n]
};

__global__ __launch_bounds__(BINS_T)
void bins_resample_kernel(const ResampleParams p)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int set = blockIdx.x;
    const int m = p.m, n = p.n, n_res = p.n_res;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, cn = lane & 15;
    const double* bins = p.bins + (size_t)set * m * n;
    const double* T = p.T + (size_t)set * n * n;
    const int rank = p.rank[set];
    double* D = p.D + (size_t)set * n_res * n;
    double* out_G = p.out_G + (size_t)set * n_res * n;
    double* out_dev = p.out_dev + (size_t)set * n_res * n;

    __shared__ double meanv[BINS_NMAX];
    __shared__ double tmean[BINS_NMAX];

    // ---- 1. mean ----
    bins_mean(bins, m, n, p.part + (size_t)set * BINS_NWAVE * n * 2, meanv, p.out_mean + (size_t)set * n);

    const int rt_n = (n_res + 15) >> 4;                  // tile rows
    const int rg_n = (rt_n + RS_RT - 1) / RS_RT;         // groups of RS_RT tile rows
    const int ct_n = (n + 15) >> 4;                      // tile columns

    // ---- 2. D = counts (bins - mean) / N_r ----
    for (int item = wave; item < ct_n * rg_n; item += BINS_NWAVE) {
        const int J = item % ct_n, rt0 = (item / ct_n) * RS_RT;
        const int j = 16 * J + cn;
        const bool jv = j < n;
        const double mj = jv ? meanv[j] : 0.0;
        d4 acc[RS_RT];
#pragma unroll
        for (int t = 0; t < RS_RT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
        for (int b0 = 0; b0 < m; b0 += 4) {
            const int b = b0 + kq;
            const bool bv = b < m;
            const double x = (bv && jv) ? bins[(size_t)b * n + j] - mj : 0.0;
#pragma unroll
            for (int t = 0; t < RS_RT; ++t)
                if (rt0 + t < rt_n) {
                    const int r = 16 * (rt0 + t) + cn;
                    const double a = (bv && r < n_res) ? (double)p.counts[(size_t)r * m + b] : 0.0;
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, x, acc[t], 0, 0, 0);
                }
        }
#pragma unroll
        for (int t = 0; t < RS_RT; ++t)
            if (rt0 + t < rt_n) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = 16 * (rt0 + t) + kq + 4 * q;
                    if (r < n_res && jv) D[(size_t)r * n + j] = acc[t][q] / p.Nr[r];
                }
            }
    }

    // ---- 3. T mean ----
    for (int k = wave; k < n; k += BINS_NWAVE) {
        double s = 0.0;
        if (k < rank)
            for (int j = lane; j < n; j += 64) s = fma(T[(size_t)k * n + j], meanv[j], s);
        s = bins_wave_sum(s);
        if (lane == 0) tmean[k] = s;
    }
    __syncthreads();                                     // (D and tmean are complete)

    // ---- dev = D T^T,  G = T mean + dev ----
    for (int item = wave; item < ct_n * rg_n; item += BINS_NWAVE) {
        const int K = item % ct_n, rt0 = (item / ct_n) * RS_RT;
        const int k = 16 * K + cn;
        const bool kv = k < rank;
        d4 acc[RS_RT];
#pragma unroll
        for (int t = 0; t < RS_RT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
        if (16 * K < rank) {
            for (int j0 = 0; j0 < n; j0 += 4) {
                const int j = j0 + kq;
                const bool jv = j < n;
                const double tb = (kv && jv) ? T[(size_t)k * n + j] : 0.0;
#pragma unroll
                for (int t = 0; t < RS_RT; ++t)
                    if (rt0 + t < rt_n) {
                        const int r = 16 * (rt0 + t) + cn;
                        const double a = (jv && r < n_res) ? D[(size_t)r * n + j] : 0.0;
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tb, acc[t], 0, 0, 0);
                    }
            }
        }
        const double tm = (kv && k < n) ? tmean[k] : 0.0;
#pragma unroll
        for (int t = 0; t < RS_RT; ++t)
            if (rt0 + t < rt_n) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = 16 * (rt0 + t) + kq + 4 * q;
                    if (r < n_res && k < n) {
                        const double dev = kv ? acc[t][q] : 0.0;
                        out_dev[(size_t)r * n + k] = dev;
                        out_G[(size_t)r * n + k] = kv ? tm + dev : 0.0;
                    }
                }
            }
    }
}

struct ReduceParams {
    const double* H;         // rows of nw values
    const int* row;          // [rows] the row of H a member is, or NULL: its own index
    const int* off;          // [n_groups + 1]
    const double* scale;     // [n_groups]
    const double* F;         // [n_f][nw], unused with n_f == 0
    int nw, n_f;
    int* ok;                 // [rows]  1: the row is finite
    double* fval;            // [rows][n_f]
    double* mean;            // [n_groups][nw]
    double* var;             // [n_groups][nw]
    double* fmean;           // [n_groups][n_f]
    double* fcov;            // [n_groups][n_f][n_f]
    int* used;               // [n_groups]
};

__global__ __launch_bounds__(256)
void resample_reduce_kernel(const ReduceParams p)
{
    const int g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = p.nw, n_f = p.n_f;
    const int r0 = p.off[g], r1 = p.off[g + 1];

    // ---- 1. per row: finite?, functional values ----
    for (int r = r0 + wave; r < r1; r += 4) {
        const double* h = p.H + (size_t)(p.row ? p.row[r] : r) * nw;
        int bad = 0;
        for (int i = lane; i < nw; i += 64) if (!(fabs(h[i]) <= 1.79769313486231570815e308)) bad = 1;
        bad = __ballot(bad) != 0;
        if (lane == 0) p.ok[r] = bad ? 0 : 1;
        for (int f = 0; f < n_f; ++f) {
            const double* Ff = p.F + (size_t)f * nw;
            double s = 0.0;
            for (int i = lane; i < nw; i += 64) s = fma(Ff[i], h[i], s);
            s = bins_wave_sum(s);
            if (lane == 0) p.fval[(size_t)r * n_f + f] = s;
        }
    }
    __syncthreads();

    // ---- 2. mean and scaled centred sum of squares over the finite rows, in row order ----
    int nu = 0;
    for (int r = r0; r < r1; ++r) nu += p.ok[r];
    const double sc = p.scale[g];
    const double nan = __builtin_nan("");
    const double dn = (double)nu;
    for (int i = tid; i < nw; i += 256) {
        double s = 0.0;
        for (int r = r0; r < r1; ++r)
            if (p.ok[r]) s += p.H[(size_t)(p.row ? p.row[r] : r) * nw + i];
        const double mean = s / dn;                      // (no finite row: 0 / 0)
        double q = 0.0;
        for (int r = r0; r < r1; ++r)
            if (p.ok[r]) { const double d = p.H[(size_t)(p.row ? p.row[r] : r) * nw + i] - mean; q = fma(d, d, q); }
        p.mean[(size_t)g * nw + i] = mean;
        p.var[(size_t)g * nw + i] = (nu >= 2) ? sc * q : nan;
    }
    double* fmean = p.fmean + (size_t)g * n_f;
    for (int f = tid; f < n_f; f += 256) {
        double s = 0.0;
        for (int r = r0; r < r1; ++r)
            if (p.ok[r]) s += p.fval[(size_t)r * n_f + f];
        fmean[f] = s / dn;
    }
    __syncthreads();
    for (int idx = tid; idx < n_f * n_f; idx += 256) {
        const int f1 = idx / n_f, f2 = idx - f1 * n_f;
        const double m1 = fmean[f1], m2 = fmean[f2];
        double q = 0.0;
        for (int r = r0; r < r1; ++r)
            if (p.ok[r]) q = fma(p.fval[(size_t)r * n_f + f1] - m1, p.fval[(size_t)r * n_f + f2] - m2, q);
        p.fcov[((size_t)g * n_f + f1) * n_f + f2] = (nu >= 2) ? sc * q : nan;
    }
    if (tid == 0) p.used[g] = nu;
}

// ---- quantiles over the rows of a group (mxe_resample_quantiles) --------------------------------------------------------
// rows_finite_kernel: one wavefront per row, the rule of resample_reduce_kernel (a row takes part iff every entry is finite).
// resample_quantile_kernel: one workgroup (4 wavefronts) per (group, tile of RQ_COLS omega columns).  A row's segment of the
// tile is one 128-byte line.  The tile goes to LDS row-major ([row][column]: the load and every stage of the sort touch 64
// successive doubles per wavefront), a row that is left out and the padding up to the power of two `padded` as +inf; the 16
// columns are sorted side by side by one bitonic network (a fixed sequence of compare-exchanges: no atomics, nothing depends
// on the other groups); the first `used` entries of a column are then its order statistics.  Quantile q is the type-7 one:
// h = (n - 1) q, lo = floor(h), t = h - lo, d = x[lo + 1] - x[lo]; x[lo] + t d for t < 1/2 and x[lo + 1] - (1 - t) d from
// there on (the nearer end, as numpy forms it: the order statistic itself where t = 0, and no step at q -> 1), every
// operation rounded on its own.
constexpr int RQ_COLS = 16;              // omega columns of a tile
constexpr int RQ_MAX_ROWS = 1024;        // rows of a group: RQ_COLS x 1024 doubles = 128 KB of the 160 KB of LDS, the next power of two does not fit

struct QuantileParams {
    const double* H;         // rows of nw values
    const int* row;          // [rows] the row of H a member is, or NULL: its own index
    const int* off;          // [n_groups + 1]
    const double* q;         // [n_q]
    int nw, n_q, rows;
    int padded;              // power of two >= the longest group (and >= 2)
    int* ok;                 // [rows]  1: the row is finite
    double* out;             // [n_groups][n_q][nw]
    int* used;               // [n_groups]
};

__global__ __launch_bounds__(256)
void rows_finite_kernel(const QuantileParams p)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.rows) return;                             // (wave-uniform)
    const double* h = p.H + (size_t)(p.row ? p.row[r] : r) * p.nw;
    int bad = 0;
    for (int i = lane; i < p.nw; i += 64) if (!(fabs(h[i]) <= 1.79769313486231570815e308)) bad = 1;
    bad = __ballot(bad) != 0;
    if (lane == 0) p.ok[r] = bad ? 0 : 1;
}

__global__ __launch_bounds__(256)
void resample_quantile_kernel(const QuantileParams p)
{
    extern __shared__ double rq_x[];                     // [padded][RQ_COLS]
    __shared__ int rq_cnt[4];
    const int g = blockIdx.x, w0 = RQ_COLS * blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = p.nw, P = p.padded;
    const int r0 = p.off[g], n = p.off[g + 1] - r0;      // (n <= P: the host checked)
    const double inf = __builtin_inf();

    // ---- the tile, and the number of rows that take part ----
    int cnt = 0;
    for (int base = 0; base < P; base += 256 / RQ_COLS) {
        const int r = base + (tid >> 4), c = tid & (RQ_COLS - 1);
        if (r < P) {
            double x = inf;
            if (r < n && p.ok[r0 + r]) {
                if (c == 0) ++cnt;
                if (w0 + c < nw) x = p.H[(size_t)(p.row ? p.row[r0 + r] : r0 + r) * nw + w0 + c];
            }
            rq_x[r * RQ_COLS + c] = x;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) rq_cnt[wave] = cnt;
    __syncthreads();
    const int nu = rq_cnt[0] + rq_cnt[1] + rq_cnt[2] + rq_cnt[3];

    // ---- bitonic network over the rows, the columns side by side ----
    const int c = tid & (RQ_COLS - 1);
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int pr = tid >> 4; pr < (P >> 1); pr += 256 / RQ_COLS) {
                const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), l = i | j;
                const double a = rq_x[i * RQ_COLS + c], b = rq_x[l * RQ_COLS + c];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { rq_x[i * RQ_COLS + c] = b; rq_x[l * RQ_COLS + c] = a; }
            }
            __syncthreads();
        }

    // ---- type-7 quantiles of the first nu entries of every column ----
    for (int idx = tid; idx < p.n_q * RQ_COLS; idx += 256) {
        const int iq = idx >> 4;
        if (w0 + c >= nw) continue;
        double v = __builtin_nan("");
        if (nu > 0) {
#pragma clang fp contract(off)                           // (every operation rounded on its own: no product may fuse with the sum behind it)
            const double h = (double)(nu - 1) * p.q[iq];
            int lo = (int)floor(h);
            lo = lo < 0 ? 0 : (lo > nu - 1 ? nu - 1 : lo);
            const int hi = lo + 1 < nu ? lo + 1 : nu - 1;
            const double t = h - (double)lo;
            const double a = rq_x[lo * RQ_COLS + c], b = rq_x[hi * RQ_COLS + c];
            const double d = b - a;
            const double u = 1.0 - t;
            v = (t < 0.5) ? a + d * t : b - d * u;
        }
        p.out[((size_t)g * p.n_q + iq) * nw + w0 + c] = v;
    }
    if (tid == 0 && blockIdx.y == 0) p.used[g] = nu;
}

} // namespace mxe
