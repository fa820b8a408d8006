// mxe_shrink.hip.h -- shrinkage covariance of binned Monte Carlo data (no counterpart in the reference)
//
//   bins  ->  lambda* (Schaefer & Strimmer 2005, target "diagonal, unequal variances"), then the eigenbasis of
//       C* = (1 - lambda) X^T X + lambda diag(c),   X = (bins - mean) / sqrt(m (m - 1)),  c_j = (X^T X)_jj
//
// With few bins the small eigenvalues of the sample covariance X^T X are biased low and chi^2 overweights the directions
// whose errors are known worst; C* keeps the variances and shrinks the correlations towards zero by the intensity
//       lambda_raw = sum_{i != j} Var(r_ij) / sum_{i != j} r_ij^2,      lambda* = min(1, max(0, lambda_raw)),
//       z_kj = x_kj / s_j,  G1 = Z^T Z,  G2 = (Z o Z)^T (Z o Z),
//       r_ij = G1_ij / (m - 1),  Var(r_ij) = m / (m - 1)^3 (G2_ij - G1_ij^2 / m)
//   =>  lambda_raw = m / (m - 1) * sum_{i != j} (G2_ij - G1_ij^2 / m) / sum_{i != j} G1_ij^2.
// Four kernels, no host round trip between them:
//   shrink_prep_kernel    one workgroup of 16 wavefronts per set.  The mean by bins_mean of mxe_bins.hip.h (the bits of
//                         bins_eig_kernel) and, from the same partial sums, its low part: x = (b - mean) - mean_lo has the
//                         relative accuracy of b however far the data lie from zero.  s_j^2: one thread per column, the
//                         bins in index order.  Z = x / s_j goes to a workspace [mp][np], mp = m rounded up to 4, np = n
//                         rounded up to 16, the padding and the columns with s_j = 0 as zeros: the tiles read no edge.
//   shrink_gram_kernel    one wavefront per 16 x 16 tile (I <= J) of the two Gram matrices, v_mfma_f64_16x16x4_f64 over
//                         all bins in index order (no sum is split); four tiles per workgroup, the workgroups of all sets
//                         in one grid: 512 columns are 528 tiles in 132 workgroups, 256 sets of 65 columns 1024 workgroups
//                         of 4 wavefronts.  Epilogue: the two sums over i != j of the tile (lane sums in register order,
//                         butterfly over the lanes, tiles above the diagonal counted twice) to partial[set][tile].
//   shrink_lambda_kernel  one wavefront per set: lane 0 adds the tile partials in tile order, forms lambda.
//   bins_eig_shrunk_kernel  bins_eig_body<true> of mxe_bins.hip.h: mean, centring, pivoted QR, Jacobi and selection of
//                         bins_eig_kernel on Y = [sqrt(1 - lambda) X ; sqrt(lambda) diag(sqrt(c))], Y^T Y = C* exactly.
// No atomics on floating-point values, no sum whose order depends on the launch: a set's bits depend on nothing but its
// own bins.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_bins.hip.h"

namespace mxe {

constexpr int SHRINK_TW = 4;             // tiles (wavefronts) of a workgroup of shrink_gram_kernel

struct ShrinkParams {
    int m;                   // n_bins
    int n;                   // n_data
    int mp;                  // m rounded up to a multiple of 4
    int np;                  // n rounded up to a multiple of 16
    int nt;                  // tiles of a set: ct (ct + 1) / 2, ct = np / 16
    int wgs;                 // workgroups of a set in shrink_gram_kernel: ceil(nt / SHRINK_TW)
    const double* bins;      // [set][m][n]
    double* part;            // [set][BINS_NWAVE][n][2]  partial sums of the mean
    double* Z;               // [set][mp][np]  standardised deviations, zero padded
    double* tpart;           // [set][nt][2]  per tile: sum (G2 - G1^2 / m), sum G1^2 over i != j
    double* out_mean;        // [set][n]
    double* lambda;          // [set]  lambda*
    double* lambda_raw;      // [set]
};

__global__ __launch_bounds__(BINS_T)
void shrink_prep_kernel(const ShrinkParams p)
{
    const int set = blockIdx.x;
    const int m = p.m, n = p.n, mp = p.mp, np = p.np;
    const int tid = threadIdx.x;
    const double* bins = p.bins + (size_t)set * m * n;
    double* part = p.part + (size_t)set * BINS_NWAVE * n * 2;
    double* Z = p.Z + (size_t)set * mp * np;

    __shared__ double meanv[BINS_NMAX];
    __shared__ double meanlo[BINS_NMAX];
    __shared__ double sdev[BINS_NMAX];

    bins_mean(bins, m, n, part, meanv, p.out_mean + (size_t)set * n);

    // the low part of the mean: the sums of bins_mean again, what its rounded quotient leaves
    for (int j = tid; j < n; j += BINS_T) {
        double s = 0.0, c = 0.0;
        for (int q = 0; q < BINS_NWAVE; ++q) {
            double e;
            bins_two_sum(s, part[((size_t)q * n + j) * 2], s, e);
            c += e + part[((size_t)q * n + j) * 2 + 1];
        }
        double hi, lo;
        bins_two_sum(s, c, hi, lo);
        const double mm = (double)m;
        const double mean = meanv[j];
        meanlo[j] = (fma(-mean, mm, hi) + lo) / mm;
    }
    __syncthreads();

    // s_j: one thread per column, the bins in index order
    for (int j = tid; j < n; j += BINS_T) {
        const double mh = meanv[j], ml = meanlo[j];
        double ss = 0.0;
        for (int k = 0; k < m; ++k) {
            const double x = (bins[(size_t)k * n + j] - mh) - ml;
            ss = fma(x, x, ss);
        }
        sdev[j] = sqrt(ss / (double)(m - 1));
    }
    __syncthreads();

    for (size_t idx = tid; idx < (size_t)mp * np; idx += BINS_T) {
        const int k = (int)(idx / np), j = (int)(idx - (size_t)k * np);
        double z = 0.0;
        if (k < m && j < n && sdev[j] > 0.0) z = ((bins[(size_t)k * n + j] - meanv[j]) - meanlo[j]) / sdev[j];
        Z[idx] = z;
    }
}

__global__ __launch_bounds__(64 * SHRINK_TW)
void shrink_gram_kernel(const ShrinkParams p)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int set = blockIdx.x / p.wgs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = (blockIdx.x - set * p.wgs) * SHRINK_TW + wave;
    if (t >= p.nt) return;                               // (wave-uniform; no barrier below)
    const int kq = lane >> 4, cn = lane & 15;
    const int mp = p.mp, np = p.np;
    // tile t = J (J + 1) / 2 + I, I <= J
    int J = 0;
    while ((J + 1) * (J + 2) / 2 <= t) ++J;
    const int I = t - J * (J + 1) / 2;
    const double* zi = p.Z + (size_t)set * mp * np + 16 * I + cn;
    const double* zj = p.Z + (size_t)set * mp * np + 16 * J + cn;

    d4 g1 = d4{0.0, 0.0, 0.0, 0.0}, g2 = d4{0.0, 0.0, 0.0, 0.0};
    for (int b0 = 0; b0 < mp; b0 += 4) {
        const size_t o = (size_t)(b0 + kq) * np;
        const double a = zi[o], b = zj[o];
        g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, g1, 0, 0, 0);
        g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a * a, b * b, g2, 0, 0, 0);
    }

    // entry q of a lane: row 16 I + kq + 4 q, column 16 J + cn (padded rows and columns are zeros and add nothing)
    const double mm = (double)p.m;
    double pn = 0.0, pd = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 16 * I + kq + 4 * q, j = 16 * J + cn;
        if (i != j) {
            const double g = g1[q];
            const double gg = g * g;
            pn += g2[q] - gg / mm;
            pd += gg;
        }
    }
    pn = bins_wave_sum(pn);
    pd = bins_wave_sum(pd);
    if (lane == 0) {
        const double w = (I < J) ? 2.0 : 1.0;            // (i, j) and (j, i)
        double* tp = p.tpart + ((size_t)set * p.nt + t) * 2;
        tp[0] = w * pn;
        tp[1] = w * pd;
    }
}

__global__ __launch_bounds__(64)
void shrink_lambda_kernel(const ShrinkParams p)
{
    const int set = blockIdx.x;
    if (threadIdx.x != 0) return;
    const double* tp = p.tpart + (size_t)set * p.nt * 2;
    double num = 0.0, den = 0.0;
    for (int t = 0; t < p.nt; ++t) { num += tp[2 * t]; den += tp[2 * t + 1]; }
    const double mm = (double)p.m;
    double raw = __builtin_nan(""), lam = 1.0;           // no off-diagonal correlation at all: C* = C whatever lambda
    if (den > 0.0) {
        raw = (mm / (mm - 1.0)) * num / den;
        lam = (raw >= 1.0) ? 1.0 : ((raw > 0.0) ? raw : 0.0);
    }
    p.lambda[set] = lam;
    p.lambda_raw[set] = raw;
}

__global__ __launch_bounds__(BINS_T)
void bins_eig_shrunk_kernel(const BinsParams p, const double* lam, double* diag)
{
    bins_eig_body<true>(p, lam, diag);
}

} // namespace mxe
