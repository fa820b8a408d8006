// mxe_bins.hip.h -- binned Monte Carlo data into the whitened problem, on the device (no counterpart in the reference)
//
//   bins (n_bins estimates of n_data values)  ->  mean, eigenvalues and eigenvectors of the covariance of the mean
//       C = X^T X,   X = (bins - mean) / sqrt(n_bins (n_bins - 1))
//
// C is never formed: its eigenvectors are the right singular vectors of X and its eigenvalues the squares of X's
// singular values, and a one-sided Jacobi SVD resolves those down to eps * s_max where eigh(C) stops at
// eps * lambda_max = (sqrt(eps) s_max)^2.  One workgroup of 16 wavefronts per set, all sets in one launch; a set's
// working arrays are in device memory: X^T (n_data x n_bins: 1.6 MB at 1024 x 200) for the QR stage, R (n_data x
// n_data: 0.3 MB at 200, 2 MB at 512) for the Jacobi stage.  With one set per CU, 32 sets share the 4 MB L2 of an XCD:
// R of all of them fits (Jacobi runs out of the L2), X^T does not -- every Householder step reads the trailing matrix
// twice and writes it once, about n_data^2 n_bins / 2 * 24 B = 0.5 GB per set at 1024 x 200 through the L2 and beyond.
//
//   1. mean over the bins: per column 16 row chunks, each summed serially in double-double (two-sum), the 16 partial
//      sums added in chunk order, divided in double-double: the error does not grow with n_bins (~ eps^2 n_bins), the
//      order is fixed.  A constant column has exactly its value as the mean and becomes an exact zero column of X.
//   2. X = (bins - mean) * scale.  n_bins > n_data: stored transposed (one column = one contiguous run, through a
//      64 x 64 LDS tile), then Householder QR with column pivoting as in mxe_svd.hip.h (stopped at the first step whose
//      largest remaining column norm is below eps * the largest of X): X P = Q R, R of r <= n_data rows.  Q is never
//      needed.  n_bins <= n_data (the covariance is rank deficient): the n_bins rows of X take the place of R.
//   3. one-sided Jacobi (Hestenes) on the rows of R, round-robin pairs, one wavefront per pair, both rows of a pair
//      held in registers between the inner products and the rotation: J^T R = diag(s) W^T.  The rotations are not
//      accumulated: the rows themselves are what is asked for, row k / s_k = the eigenvector of lambda_k = s_k^2.
//   4. kept: lambda_k >= threshold and lambda_k > (max(n_bins, n_data) eps)^2 lambda_max (the noise floor of s_k: a
//      null direction of a rank-deficient X comes out at rounding level, not at zero).  Ascending like eigh, each
//      eigenvector with its component of largest magnitude (lowest index on ties) positive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxe {

constexpr int BINS_T = 1024;             // threads of a set's workgroup
constexpr int BINS_NWAVE = BINS_T / 64;
constexpr int BINS_NMAX = 512;           // most data points (columns) of a set
constexpr int BINS_NC = BINS_NMAX / 64;  // values of a row one lane holds
constexpr int BINS_MAX_SWEEPS = 60;      // Jacobi sweeps before a set is given up (status 1)

struct BinsParams {
    int m;               // n_bins
    int n;               // n_data
    int rcap;            // rows of Rm per set: min(m, n) rounded up to even
    double scale;        // 1 / sqrt(m (m - 1))
    double threshold;    // absolute cut on the eigenvalues
    double floor2;       // (max(m, n) eps)^2
    const double* bins;  // [set][m][n]
    // per set (stride = set index):
    double* A;           // [n][m]  X^T, destroyed (m > n only)
    double* Rm;          // [rcap][n]  R (or X), then diag(s) W^T
    double* vk;          // [m]  current Householder vector
    double* part;        // [BINS_NWAVE][n][2]  partial sums of the mean (high, low)
    double* cn2;         // [n]  remaining squared column norms
    int* perm;           // [n]
    double* out_mean;    // [n]
    double* out_var;     // [n]
    double* out_T;       // [n][n]
    int* out_info;       // [4]: rank kept, rows of R, Jacobi sweeps, status (0 ok, 1 sweeps exhausted or not finite)
};

__device__ __forceinline__ double bins_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// s + e = a + b exactly
__device__ __forceinline__ void bins_two_sum(double a, double b, double& s, double& e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// The mean over the m bins of one set (n columns), by the whole workgroup of BINS_T threads: wavefront w sums the rows
// of chunk w serially in double-double, lanes over the columns; the BINS_NWAVE partial sums are added in chunk order and
// divided in double-double.  ``part``: [BINS_NWAVE][n][2] of device memory, ``meanv``: [n] of LDS; both hold the result
// (and ``out_mean``) behind the barrier this ends with.  Shared by bins_eig_kernel and bins_resample_kernel
// (mxe_resample.hip.h): their means are the same bits.
__device__ __forceinline__ void bins_mean(const double* bins, int m, int n, double* part, double* meanv, double* out_mean)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const int ch = (m + BINS_NWAVE - 1) / BINS_NWAVE;
        const int i0 = min(wave * ch, m), i1 = min(i0 + ch, m);
        for (int j = lane; j < n; j += 64) {
            double s = 0.0, c = 0.0;
            for (int i = i0; i < i1; ++i) {
                double e;
                bins_two_sum(s, bins[(size_t)i * n + j], s, e);
                c += e;
            }
            part[((size_t)wave * n + j) * 2] = s;
            part[((size_t)wave * n + j) * 2 + 1] = c;
        }
    }
    __syncthreads();
    for (int j = tid; j < n; j += BINS_T) {
        double s = 0.0, c = 0.0;
        for (int q = 0; q < BINS_NWAVE; ++q) {
            double e;
            bins_two_sum(s, part[((size_t)q * n + j) * 2], s, e);
            c += e + part[((size_t)q * n + j) * 2 + 1];
        }
        double hi, lo;
        bins_two_sum(s, c, hi, lo);
        // (hi + lo) / m, the remainder of the first quotient exact in one fma
        const double mm = (double)m;
        const double q0 = hi / mm;
        const double rem = fma(-q0, mm, hi) + lo;
        const double mean = q0 + rem / mm;
        meanv[j] = mean;
        out_mean[j] = mean;
    }
    __syncthreads();
}

// The stages of a set's decomposition, by its workgroup of BINS_T threads.  SHRUNK = false: bins_eig_kernel, as described
// above.  SHRUNK = true (bins_eig_shrunk_kernel, mxe_shrink.hip.h): the matrix whose right singular vectors are asked for
// is Y = [sqrt(1 - lambda) X ; sqrt(lambda) diag(sqrt(c))], c_j = sum_k X_kj^2 (written to ``diag``), lambda = *lam read
// from device memory: Y^T Y = (1 - lambda) X^T X + lambda diag(c).  The n diagonal rows are appended to the columns of
// X^T (M = m + n rows; A: [n][M], vk: [M]) and Y always goes through the QR stage.  With SHRUNK = false M is m and every
// operation is the one bins_eig_kernel has always done: its outputs keep their bits.
template <bool SHRUNK>
__device__ __forceinline__ void bins_eig_body(const BinsParams& p, const double* lam, double* diag)
{
    const int set = blockIdx.x;
    const int m = p.m, n = p.n;
    const int M = SHRUNK ? m + n : m;                    // rows of the matrix the QR stage works on
    const bool tall = SHRUNK || m > n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* bins = p.bins + (size_t)set * m * n;
    double* A = p.A + (tall ? (size_t)set * n * M : 0);
    double* Rm = p.Rm + (size_t)set * p.rcap * n;
    double* vk = p.vk + (size_t)set * M;
    double* part = p.part + (size_t)set * BINS_NWAVE * n * 2;
    double* cn2 = p.cn2 + (size_t)set * n;
    int* perm = p.perm + (size_t)set * n;
    double* out_mean = p.out_mean + (size_t)set * n;
    double* out_var = p.out_var + (size_t)set * n;
    double* out_T = p.out_T + (size_t)set * n * n;
    int* out_info = p.out_info + (size_t)set * 4;

    __shared__ double tile[64][65];
    __shared__ double meanv[BINS_NMAX];
    __shared__ double s2[BINS_NMAX];
    __shared__ int order[BINS_NMAX];
    __shared__ double redv[BINS_NWAVE];
    __shared__ int redi[BINS_NWAVE];
    __shared__ int sh_piv, sh_stop, sh_rot;
    __shared__ double sh_nrm0;

    // ---- 1. mean ----
    bins_mean(bins, m, n, part, meanv, out_mean);

    // ---- 2. X = (bins - mean) * scale ----
    int r = 0;
    if (tall) {
        // transposed into A (column j = m contiguous values) through a 64 x 64 tile: reads and writes along the fast index
        const int tx = tid & 63, ty = tid >> 6;
        for (int i0 = 0; i0 < m; i0 += 64) {
            for (int j0 = 0; j0 < n; j0 += 64) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + ty + 16 * q, j = j0 + tx;
                    if (i < m && j < n) tile[ty + 16 * q][tx] = (bins[(size_t)i * n + j] - meanv[j]) * p.scale;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + ty + 16 * q, i = i0 + tx;
                    if (i < m && j < n) A[(size_t)j * M + i] = tile[tx][ty + 16 * q];
                }
                __syncthreads();
            }
        }
        // column norms
        for (int j = wave; j < n; j += BINS_NWAVE) {
            double s = 0.0;
            for (int i = lane; i < m; i += 64) { const double x = A[(size_t)j * M + i]; s = fma(x, x, s); }
            s = bins_wave_sum(s);
            if (lane == 0) { cn2[j] = s; perm[j] = j; }
        }
        __syncthreads();
        if constexpr (SHRUNK) {
            // Y: the rows of X times sqrt(1 - lambda), below them sqrt(lambda c_j) on the diagonal; the column norms again
            const double lm = lam[set];
            const double wx = sqrt(1.0 - lm), wd = sqrt(lm);
            for (int j = wave; j < n; j += BINS_NWAVE) {
                double* col = A + (size_t)j * M;
                const double cj = cn2[j];
                double s = 0.0;
                for (int i = lane; i < M; i += 64) {
                    const double x = (i < m) ? wx * col[i] : ((i - m == j) ? wd * sqrt(cj) : 0.0);
                    col[i] = x;
                    s = fma(x, x, s);
                }
                s = bins_wave_sum(s);
                if (lane == 0) { diag[(size_t)set * n + j] = cj; cn2[j] = s; }
            }
            __syncthreads();
        }

        // ---- Householder QR with column pivoting, early stop (mxe_svd.hip.h, without its cap on the rows of R) ----
        for (int k = 0; k < n; ++k) {
            double best = -1.0; int bi = k;
            for (int j = k + tid; j < n; j += BINS_T) { const double c = cn2[j]; if (c > best) { best = c; bi = j; } }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (lane == 0) { redv[wave] = best; redi[wave] = bi; }
            __syncthreads();
            if (tid == 0) {
                double bb = redv[0]; int ii = redi[0];
                for (int w2 = 1; w2 < BINS_NWAVE; ++w2)
                    if (redv[w2] > bb || (redv[w2] == bb && redi[w2] < ii)) { bb = redv[w2]; ii = redi[w2]; }
                if (k == 0) sh_nrm0 = bb;
                const double eps = 2.220446049250313e-16;
                sh_stop = !(bb > eps * eps * sh_nrm0) || !(bb > 0.0);
                sh_piv = ii;
            }
            __syncthreads();
            if (sh_stop) break;
            const int piv = sh_piv;
            if (piv != k) {
                for (int i = tid; i < M; i += BINS_T) {
                    const double x = A[(size_t)k * M + i];
                    A[(size_t)k * M + i] = A[(size_t)piv * M + i];
                    A[(size_t)piv * M + i] = x;
                }
                if (tid == 0) {
                    const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
                    cn2[piv] = cn2[k];
                }
            }
            __syncthreads();
            // Householder vector of column k, rows k..m-1 (wave 0)
            if (wave == 0) {
                double s = 0.0;
                for (int i = k + lane; i < M; i += 64) { const double x = A[(size_t)k * M + i]; s = fma(x, x, s); }
                s = bins_wave_sum(s);
                const double x0 = A[(size_t)k * M + k];
                const double nrm = sqrt(s);
                const double alpha = (x0 >= 0.0) ? -nrm : nrm;
                const double vn = sqrt(2.0 * (s - alpha * x0));       // |x - alpha e0|
                const double inv = (vn > 0.0) ? 1.0 / vn : 0.0;
                for (int i = k + lane; i < M; i += 64) {
                    vk[i] = ((i == k) ? (x0 - alpha) : A[(size_t)k * M + i]) * inv;
                    A[(size_t)k * M + i] = (i == k) ? alpha : 0.0;
                }
            }
            __syncthreads();
            // H_k = I - 2 v v^T on the columns j > k: one wavefront per column, four columns in flight per wavefront
            for (int j0 = k + 1 + wave; j0 < n; j0 += 4 * BINS_NWAVE) {
                double s[4], rem[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s[q] = 0.0;
                    const int j = min(j0 + q * BINS_NWAVE, n - 1);
                    const double* col = A + (size_t)j * M;
                    for (int i = k + lane; i < M; i += 64) s[q] = fma(vk[i], col[i], s[q]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] = 2.0 * bins_wave_sum(s[q]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    rem[q] = 0.0;
                    const int j = j0 + q * BINS_NWAVE;
                    if (j < n) {
                        double* col = A + (size_t)j * M;
                        for (int i = k + lane; i < M; i += 64) {
                            const double x = fma(-s[q], vk[i], col[i]);
                            col[i] = x;
                            if (i > k) rem[q] = fma(x, x, rem[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    rem[q] = bins_wave_sum(rem[q]);
                    const int j = j0 + q * BINS_NWAVE;
                    if (lane == 0 && j < n) cn2[j] = rem[q];
                }
            }
            __syncthreads();
            r = k + 1;
        }
        __syncthreads();
        // R (r x n, row-major, columns in pivot order); a zero row pads an odd r
        const int rr0 = (r + 1) & ~1;
        for (int idx = tid; idx < rr0 * n; idx += BINS_T) {
            const int kk = idx / n, j = idx - kk * n;
            Rm[idx] = (kk < r && j >= kk) ? A[(size_t)j * M + kk] : 0.0;
        }
    } else {
        // the short side: the m rows of X are the rows to orthogonalise (row-major, as the bins come)
        r = m;
        const int rr0 = (r + 1) & ~1;
        for (int idx = tid; idx < rr0 * n; idx += BINS_T) {
            const int i = idx / n, j = idx - i * n;
            Rm[idx] = (i < m) ? (bins[(size_t)i * n + j] - meanv[j]) * p.scale : 0.0;
        }
        for (int j = tid; j < n; j += BINS_T) perm[j] = j;
        if (tid == 0) sh_nrm0 = 0.0;
    }
    __syncthreads();

    // ---- 3. one-sided Jacobi on the rows of R, round-robin pairs, one wavefront per pair ----
    const int rr = (r + 1) & ~1;
    int sweeps = 0, status = 0;
    if (rr >= 2) {
        status = 1;
        for (int sweep = 0; sweep < BINS_MAX_SWEEPS; ++sweep) {
            if (tid == 0) sh_rot = 0;
            __syncthreads();
            for (int round = 0; round < rr - 1; ++round) {
                for (int pi = wave; pi < rr / 2; pi += BINS_NWAVE) {
                    int a, b;
                    if (pi == 0) { a = rr - 1; b = round % (rr - 1); }
                    else { a = (round + pi) % (rr - 1); b = (round - pi + 2 * (rr - 1)) % (rr - 1); }
                    const int pp = min(a, b), qq = max(a, b);
                    double* x = Rm + (size_t)pp * n;
                    double* y = Rm + (size_t)qq * n;
                    double xv[BINS_NC], yv[BINS_NC];
                    double aa = 0.0, bb = 0.0, gg = 0.0;
#pragma unroll
                    for (int c = 0; c < BINS_NC; ++c) {
                        const int j = lane + 64 * c;
                        xv[c] = 0.0; yv[c] = 0.0;
                        if (j < n) { xv[c] = x[j]; yv[c] = y[j]; }
                        aa = fma(xv[c], xv[c], aa); bb = fma(yv[c], yv[c], bb); gg = fma(xv[c], yv[c], gg);
                    }
                    aa = bins_wave_sum(aa); bb = bins_wave_sum(bb); gg = bins_wave_sum(gg);
                    const double eps = 2.220446049250313e-16;
                    // (sqrt(aa) sqrt(bb), not sqrt(aa bb): the product of two squared norms is a fourth power of the data)
                    if (aa > 0.0 && bb > 0.0 && fabs(gg) > eps * (sqrt(aa) * sqrt(bb))) {
                        const double zeta = (bb - aa) / (2.0 * gg);
                        // |zeta| beyond 1e150: zeta^2 would overflow; t = 1 / (2 zeta) there to rounding
                        const double az = fabs(zeta);
                        const double t = ((zeta >= 0.0) ? 1.0 : -1.0) / ((az < 1.0e150) ? az + sqrt(1.0 + zeta * zeta) : 2.0 * az);
                        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                        if constexpr (SHRUNK) {
                            // x - sn (y + tau x), tau = sn / (1 + cs) = (1 - cs) / sn: below |t| ~ 1e-8 cs rounds to 1 and
                            // (cs, sn) stretches the pair by 1 + t^2 -- always up, and a row sees n - 1 such rotations per
                            // late sweep (measured: eigenvalues high by 1.7e-13 at 512 rows).  This form carries 1 - cs
                            // as a term of its own.  bins_eig_kernel keeps the form (and the bits) it has always had.
                            const double tau = sn / (1.0 + cs);
#pragma unroll
                            for (int c = 0; c < BINS_NC; ++c) {
                                const int j = lane + 64 * c;
                                if (j < n) {
                                    x[j] = xv[c] - sn * fma(tau, xv[c], yv[c]);
                                    y[j] = yv[c] + sn * fma(-tau, yv[c], xv[c]);
                                }
                            }
                        } else {
#pragma unroll
                            for (int c = 0; c < BINS_NC; ++c) {
                                const int j = lane + 64 * c;
                                if (j < n) {
                                    // (the fused forms this kernel has always been compiled to, spelled out: its bits
                                    // do not hang on which product the compiler picks to fuse)
                                    x[j] = fma(cs, xv[c], -(sn * yv[c]));
                                    y[j] = fma(sn, xv[c], cs * yv[c]);
                                }
                            }
                        }
                        if (lane == 0) atomicAdd(&sh_rot, 1);
                    }
                }
                __syncthreads();
            }
            sweeps = sweep + 1;
            const int nrot = sh_rot;
            __syncthreads();
            if (nrot == 0) { status = 0; break; }
        }
    }

    // ---- 4. eigenvalues, order, selection ----
    for (int kk = wave; kk < rr; kk += BINS_NWAVE) {
        double s = 0.0;
        for (int j = lane; j < n; j += 64) { const double x = Rm[(size_t)kk * n + j]; s = fma(x, x, s); }
        s = bins_wave_sum(s);
        if (lane == 0) s2[kk] = s;
    }
    __syncthreads();
    if (tid < rr) {
        const double mine = s2[tid];
        int rank = 0;
        for (int l = 0; l < rr; ++l) { const double o = s2[l]; if (o > mine || (o == mine && l < tid)) ++rank; }
        order[rank] = tid;          // descending
    }
    __syncthreads();
    bool bad = false;
    for (int kk = 0; kk < rr; ++kk) if (!(s2[kk] >= 0.0 && s2[kk] <= 1.7976931348623157e308)) bad = true;
    int ns = 0;
    if (!bad && rr > 0) {
        const double lmax = s2[order[0]];
        for (int kk = 0; kk < rr; ++kk) {
            const double lam = s2[order[kk]];
            if (lam >= p.threshold && lam > p.floor2 * lmax && lam > 0.0) ns = kk + 1; else break;
        }
    }
    if (bad) { ns = 0; status = 1; }
    if (ns > n) ns = n;             // (cannot happen: at most min(m, n) rows are nonzero)

    // outputs: ascending, row k of T = row order[ns - 1 - k] of diag(s) W^T over s, largest component positive
    for (int k = tid; k < n; k += BINS_T) out_var[k] = (k < ns) ? s2[order[ns - 1 - k]] : 0.0;
    for (int k = wave; k < n; k += BINS_NWAVE) {
        double* trow = out_T + (size_t)k * n;
        if (k >= ns) {
            for (int j = lane; j < n; j += 64) trow[j] = 0.0;
            continue;
        }
        const int row = order[ns - 1 - k];
        const double* rrow = Rm + (size_t)row * n;
        double big = -1.0; int bj = 0; double bval = 0.0;
        for (int j = lane; j < n; j += 64) {
            const double v = rrow[j]; const int jo = perm[j];
            if (fabs(v) > big || (fabs(v) == big && jo < bj)) { big = fabs(v); bj = jo; bval = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(big, o, 64); const int oj = __shfl_xor(bj, o, 64);
            const double ov = __shfl_xor(bval, o, 64);
            if (ob > big || (ob == big && oj < bj)) { big = ob; bj = oj; bval = ov; }
        }
        const double inv = ((bval < 0.0) ? -1.0 : 1.0) / sqrt(s2[row]);
        for (int j = lane; j < n; j += 64) trow[perm[j]] = rrow[j] * inv;
    }
    if (tid == 0) { out_info[0] = ns; out_info[1] = r; out_info[2] = sweeps; out_info[3] = status; }
}

__global__ __launch_bounds__(BINS_T)
void bins_eig_kernel(const BinsParams p)
{
    bins_eig_body<false>(p, nullptr, nullptr);
}

} // namespace mxe
