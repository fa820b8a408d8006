// mxe_bincheck.hip.h -- may the Monte Carlo bins be used as they are?  (no counterpart in the reference)
//
//   bins in Monte Carlo order  ->  per column and block length 2^k: the squared error of the mean, skewness and excess
//                                  kurtosis of the block means                                          bins_check_kernel
//
// The covariance of the mean that mxe_bins_eig decomposes is right for uncorrelated, normally distributed bins.  The
// blocking ladder (Flyvbjerg and Petersen) tests the first: the error of the mean estimated from blocks of 2^k bins
// rises with k until the blocks are longer than the autocorrelation time.  The standardised third and fourth moments of
// the block means test the second.
//
// One workgroup of 16 wavefronts per set, all sets in one launch.  A set's work arrays are in device memory: Y0
// (n_bins x n_data) and Y1 (n_bins / 2 x n_data), the block sums of even and odd levels.
//   1. mean over the bins: bins_mean of mxe_bins.hip.h, the code bins_eig_kernel runs -- the same bits.
//   2. level 0, y[b][c] = d[b][c] = bins[b][c] - mean[c] in the data basis; in the eigen basis y[b][k] =
//      sum_j T[k][j] d[b][j] as v_mfma_f64_16x16x4_f64 tiles (operands as in bins_resample_kernel: a wavefront owns a tile
//      column and RS_RT tile rows and runs over ALL j in index order, edges padded with zeros); columns k >= rank are zeros.
//   3. per level k (b = 2^k, n_k = n_bins >> k blocks, a trailing remainder of the bins dropped at this level only):
//      wavefront w owns the blocks of chunk w (16 chunks of an even number of blocks), lanes over the columns.
//      pass 1: the chunk's sum of the block means B_q = S_q / b, and S of level k + 1 = S_2p + S_2p+1 into the other array;
//              the 16 partial sums in chunk order / n_k = the mean of the block means.
//      pass 2: the chunk's sums of (B_q - mean)^p, p = 2, 3, 4 -- powers of the explicit difference, no raw moments --;
//              the 16 partial sums in chunk order / n_k = the central moments mu_p.
//      err2 = mu_2 / (n_k - 1), skew = mu_3 / mu_2^(3/2), kurt = mu_4 / mu_2^2 - 3; mu_2 == 0: 0, NaN, NaN.
// Sums and products of the moments are not contracted into fma: two blocks then give differences that are exact
// opposites, a skewness of exactly 0 and a kurtosis of exactly -2.  Every sum has one order that depends on
// (n_bins, n_data) alone; no atomics: a set's output is the same bits alone or in a batch, and from call to call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_bins.hip.h"
#include "mxe_resample.hip.h"

namespace mxe {

struct BinCheckParams {
    int m;                   // n_bins
    int n;                   // n_data
    int L;                   // levels: floor(log2 m)
    const double* bins;      // [set][m][n]
    const double* T;         // [set][n][n], or NULL: the data basis
    const int* rank;         // [set] (with T)
    double* part;            // [set][BINS_NWAVE][n][2]  partial sums of the mean, then of the block means
    double* part2;           // [set][BINS_NWAVE][n][3]  partial sums of the powers
    double* Y0;              // [set][m][n]      block sums of the even levels
    double* Y1;              // [set][m / 2][n]  block sums of the odd levels
    double* out_mean;        // [set][n]
    double* out_err2;        // [set][L][n]
    double* out_skew;        // [set][L][n]
    double* out_kurt;        // [set][L][n]
};

__global__ __launch_bounds__(BINS_T)
void bins_check_kernel(const BinCheckParams p)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int set = blockIdx.x;
    const int m = p.m, n = p.n, L = p.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* bins = p.bins + (size_t)set * m * n;
    double* part = p.part + (size_t)set * BINS_NWAVE * n * 2;
    double* part2 = p.part2 + (size_t)set * BINS_NWAVE * n * 3;
    double* cur = p.Y0 + (size_t)set * m * n;
    double* nxt = p.Y1 + (size_t)set * (m >> 1) * n;

    __shared__ double meanv[BINS_NMAX];
    __shared__ double barv[BINS_NMAX];

    // ---- 1. mean ----
    bins_mean(bins, m, n, part, meanv, p.out_mean + (size_t)set * n);

    // ---- 2. level 0 ----
    if (p.T == nullptr) {
        for (int b = wave; b < m; b += BINS_NWAVE)
            for (int j = lane; j < n; j += 64) cur[(size_t)b * n + j] = bins[(size_t)b * n + j] - meanv[j];
    } else {
        const double* T = p.T + (size_t)set * n * n;
        const int rank = p.rank[set];
        const int kq = lane >> 4, cn = lane & 15;
        const int rt_n = (m + 15) >> 4;                      // tile rows (of 16 bins)
        const int rg_n = (rt_n + RS_RT - 1) / RS_RT;         // groups of RS_RT tile rows
        const int ct_n = (n + 15) >> 4;                      // tile columns
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
                    const double mj = jv ? meanv[j] : 0.0;
#pragma unroll
                    for (int t = 0; t < RS_RT; ++t)
                        if (rt0 + t < rt_n) {
                            const int b = 16 * (rt0 + t) + cn;
                            const double a = (jv && b < m) ? bins[(size_t)b * n + j] - mj : 0.0;
                            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tb, acc[t], 0, 0, 0);
                        }
                }
            }
#pragma unroll
            for (int t = 0; t < RS_RT; ++t)
                if (rt0 + t < rt_n) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int b = 16 * (rt0 + t) + kq + 4 * q;
                        if (b < m && k < n) cur[(size_t)b * n + k] = kv ? acc[t][q] : 0.0;
                    }
                }
        }
    }
    __syncthreads();

    // ---- 3. the ladder ----
    double* out_err2 = p.out_err2 + (size_t)set * L * n;
    double* out_skew = p.out_skew + (size_t)set * L * n;
    double* out_kurt = p.out_kurt + (size_t)set * L * n;
    double inv = 1.0;                                        // 1 / 2^level, exact
    for (int level = 0; level < L; ++level) {
#pragma clang fp contract(off)
        const int nk = m >> level;
        const int ch = (((nk + BINS_NWAVE - 1) / BINS_NWAVE) + 1) & ~1;   // blocks of a chunk: even, pairs do not straddle chunks
        const int q0 = min(wave * ch, nk), q1 = min(q0 + ch, nk);
        const bool more = level + 1 < L;
        const double dnk = (double)nk;

        // pass 1: sums of the block means; the block sums of the next level
        for (int j = lane; j < n; j += 64) {
            double s = 0.0;
            int q = q0;
#pragma unroll 4
            for (; q + 1 < q1; q += 2) {
                const double a = cur[(size_t)q * n + j], b = cur[(size_t)(q + 1) * n + j];
                s += a * inv;
                s += b * inv;
                if (more) nxt[(size_t)(q >> 1) * n + j] = a + b;
            }
            if (q < q1) s += cur[(size_t)q * n + j] * inv;
            part[(size_t)wave * n + j] = s;
        }
        __syncthreads();
        for (int j = tid; j < n; j += BINS_T) {
            double s = 0.0;
            for (int w = 0; w < BINS_NWAVE; ++w) s += part[(size_t)w * n + j];
            barv[j] = s / dnk;
        }
        __syncthreads();

        // pass 2: powers of the explicit differences
        for (int j = lane; j < n; j += 64) {
            const double bar = barv[j];
            double s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll 4
            for (int q = q0; q < q1; ++q) {
                const double d = cur[(size_t)q * n + j] * inv - bar;
                const double d2 = d * d;
                s2 += d2;
                s3 += d2 * d;
                s4 += d2 * d2;
            }
            double* o = part2 + ((size_t)wave * n + j) * 3;
            o[0] = s2; o[1] = s3; o[2] = s4;
        }
        __syncthreads();
        for (int j = tid; j < n; j += BINS_T) {
            double s2 = 0.0, s3 = 0.0, s4 = 0.0;
            for (int w = 0; w < BINS_NWAVE; ++w) {
                const double* o = part2 + ((size_t)w * n + j) * 3;
                s2 += o[0]; s3 += o[1]; s4 += o[2];
            }
            const double mu2 = s2 / dnk, mu3 = s3 / dnk, mu4 = s4 / dnk;
            const bool flat = !(mu2 > 0.0);
            const double nan = __builtin_nan("");
            out_err2[(size_t)level * n + j] = flat ? 0.0 : mu2 / (dnk - 1.0);
            out_skew[(size_t)level * n + j] = flat ? nan : mu3 / (mu2 * sqrt(mu2));
            out_kurt[(size_t)level * n + j] = flat ? nan : mu4 / (mu2 * mu2) - 3.0;
        }
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
        inv *= 0.5;
    }
}

} // namespace mxe
