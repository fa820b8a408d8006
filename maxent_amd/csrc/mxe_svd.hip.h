// mxe_svd.hip.h -- kernel matrix staging on the device
//
//   TauKernel._fill_values      kernels.py:244-271   -> tau_kernel_fill
//   IOmegaKernel._fill_values   kernels.py:312-331   -> iomega_kernel_fill  (stacked real [Re K ; Im K])
//   BosonicTauKernel, BosonicIOmegaKernel (no counterpart in the reference) -> boson_tau_kernel_fill, boson_iomega_kernel_fill
//   LegendreKernel (G_l; no counterpart in the reference) -> legendre_kernel_fill
//   DataKernel (a caller's matrix)  kernels.py:183-207 -> data_kernel_transpose
//   get_preblur                 preblur.py:31-58     -> preblur_rows / preblur_cols / preblur_matrix
//   PreblurKernel._fill_values  kernels.py:384-393   -> preblur_product   (K' = K diag(delta) B)
//   KernelSVD.svd + reduce_singular_space kernels.py:53-122 -> svd_kernel
//
// One launch serves a whole batch of blur widths b (a "b-scan", doc/guide/preblur_example.py): one
// workgroup of 16 wavefronts per b does the decomposition, everything it touches (0.8 MB of K^T,
// 0.25 MB of R) stays in the L2 of its XCD.
//
// SVD algorithm (Drmac / Veselic style preconditioned one-sided Jacobi, all binary64):
//   1. Householder QR with column pivoting of K (n_tau x n_omega), stopped at the first step whose
//      largest remaining column norm is below eps * (largest column norm of K): K P = Q R with R of
//      r ~ 60 rows (the kernel's singular values decay exponentially; what is left is rounding noise,
//      LAPACK's singular values below eps * sigma_max are noise too).
//   2. one-sided Jacobi (Hestenes) on the r rows of R in round-robin order, r/2 disjoint pairs per
//      round, one wavefront per pair: R = J diag(S) W^T.  Rows of R are graded by the pivoting, which
//      is what makes Jacobi converge in ~10 sweeps here (on K itself: > 30, measured with the numpy model).
//   3. U = Q J, V = P W, sorted by S, truncated at S >= threshold (absolute, like the reference).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxe {

constexpr int SVD_T = 1024;          // threads of the decomposition workgroup
constexpr int SVD_NWAVE = SVD_T / 64;
constexpr int SVD_RCAP = 128;        // most rows of R kept (= the solver's n_s limit)
#ifndef MXE_X_SVD_SWEEPS
#define MXE_X_SVD_SWEEPS 40
#endif
constexpr int SVD_MAX_SWEEPS = MXE_X_SVD_SWEEPS;

// K^T[j][i] = K(tau_i, omega_j)  (column-major K: one column = one contiguous run of n_tau values)
__global__ __launch_bounds__(256)
void tau_kernel_fill(const double* __restrict__ tau, const double* __restrict__ omega, double beta,
                     int n_tau, int n_omega, double* __restrict__ Kt)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_tau * n_omega) return;
    const int j = idx / n_tau, i = idx - j * n_tau;
    const double w = omega[j], t = tau[i];
    // two algebraically equal forms, each overflow-free on its half-axis (kernels.py:256-263)
    Kt[idx] = (w >= 0.0) ? -exp(-w * t) / (exp(-beta * w) + 1.0)
                         : -exp(w * (beta - t)) / (1.0 + exp(beta * w));
}

// K^T[j][r] of IOmegaKernel, stacked real: K(i w_n, w) = 1 / (i w_n - w) = (-w - i w_n) / (w_n^2 + w^2),
// rows r < n_iw the real parts -w / d, rows n_iw + r the imaginary parts -w_n / d, both from ONE
// d = w_n^2 + w^2.  Column-major like tau_kernel_fill: column j is a contiguous run of 2 n_iw values.
// One thread per (w_n, w) pair writes both parts.
__global__ __launch_bounds__(256)
void iomega_kernel_fill(const double* __restrict__ iomega, const double* __restrict__ omega,
                        int n_iw, int n_omega, double* __restrict__ Kt)
{
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_iw * n_omega) return;
    const int j = idx / n_iw, i = idx - j * n_iw;
    const double w = omega[j], wn = iomega[i];
    const double d = wn * wn + w * w;              // (not contracted to an fma: the host's rounding, bit for bit)
    double* col = Kt + (size_t)j * 2 * n_iw;
    col[i] = -w / d;
    col[n_iw + i] = -wn / d;
}

// exp(a * b) with the rounding of the product given back: p = fl(a b), e = a b - p exactly (one fma), and
// exp(p + e) = exp(p) (1 + e) to first order in e (|e| <= ulp(p) / 2).  The error of the result is then a few ulp
// whatever the size of the argument; a plain exp(a * b) is off by |a b| 2^-53 relative.  ``extra``: a further small
// addend of the argument (the rounding of beta - tau times omega).
__device__ __forceinline__ double exp_of_product(double a, double b, double extra)
{
    const double p = a * b;
    const double e = fma(a, b, -p) + extra;
    const double x = exp(p);
    return fma(x, e, x);
}

// Series cut of the bosonic tau kernel: below |beta omega| = BOSON_SERIES_CUT the factor (beta omega) / (1 - e^{-beta omega})
// is 1 + x/2 + x^2/12 (next term x^4/720 < 2e-23); this also covers omega = 0 exactly (K = 1/beta) and products
// beta omega that underflow.
constexpr double BOSON_SERIES_CUT = 1.0e-5;

// K^T[j][i] of BosonicTauKernel, K(tau, omega) = omega e^{-tau omega} / (1 - e^{-beta omega}), K(tau, 0) = 1/beta,
// column-major like tau_kernel_fill.  The branches of the host fill (kernels.py, BosonicTauKernel._fill_values):
//   |beta omega| < cut : (1/beta) (1 + x/2 + x^2/12) e^{-tau omega}
//   omega > 0          : omega e^{-tau omega} / (-expm1(-beta omega))
//   omega < 0          : omega e^{(beta - tau) omega} / expm1(beta omega)       (no overflow on either half-axis)
// symmetric (omega >= 0 only): K(tau, omega) + K(tau, -omega)
//   = omega (e^{-tau omega} + e^{-(beta - tau) omega}) / (-expm1(-beta omega)),  2/beta at omega = 0.
__global__ __launch_bounds__(256)
void boson_tau_kernel_fill(const double* __restrict__ tau, const double* __restrict__ omega, double beta,
                           int symmetric, int n_tau, int n_omega, double* __restrict__ Kt)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_tau * n_omega) return;
    const int j = idx / n_tau, i = idx - j * n_tau;
    const double w = omega[j], t = tau[i];
    const double x = beta * w;
    // beta - tau = bt + bt_lo exactly (two-sum)
    const double bt = beta - t;
    const double bb = bt - beta;
    const double bt_lo = (beta - (bt - bb)) + (-t - bb);
    double val;
    if (fabs(x) < BOSON_SERIES_CUT) {
        const double ep = exp_of_product(-t, w, 0.0);
        const double sp = 1.0 + 0.5 * x + x * x / 12.0;
        if (symmetric) {
            const double em = exp_of_product(t, w, 0.0);
            const double sn = 1.0 - 0.5 * x + x * x / 12.0;
            val = sp * ep / beta + sn * em / beta;
        } else {
            val = sp * ep / beta;
        }
    } else if (symmetric) {
        const double ep = exp_of_product(-t, w, 0.0);
        const double em = exp_of_product(-bt, w, -bt_lo * w);
        val = w * (ep + em) / (-expm1(-x));
    } else if (w > 0.0) {
        val = w * exp_of_product(-t, w, 0.0) / (-expm1(-x));
    } else {
        val = w * exp_of_product(bt, w, bt_lo * w) / expm1(x);
    }
    Kt[idx] = val;
}

// K^T of BosonicIOmegaKernel, K(i nu_n, w) = w / (w - i nu_n) = (w^2 + i w nu_n) / (w^2 + nu_n^2), 1 at w = nu_n = 0.
// Stacked (symmetric = 0): 2 n_inu rows, Re K = w^2 / d above Im K = w nu_n / d, both from ONE d = nu_n^2 + w^2 with
// contraction off (the host's rounding, bit for bit), as iomega_kernel_fill.  symmetric: n_inu rows of
// K(i nu_n, w) + K(i nu_n, -w) = 2 w^2 / d (real; 2 at w = nu_n = 0).
__global__ __launch_bounds__(256)
void boson_iomega_kernel_fill(const double* __restrict__ inu, const double* __restrict__ omega, int symmetric,
                              int n_inu, int n_omega, double* __restrict__ Kt)
{
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_inu * n_omega) return;
    const int j = idx / n_inu, i = idx - j * n_inu;
    const double w = omega[j], nu = inu[i];
    const double w2 = w * w;
    const double d = nu * nu + w2;
    const bool origin = !(d > 0.0);                 // (w = nu_n = 0, or both squares underflow)
    if (symmetric) {
        Kt[(size_t)j * n_inu + i] = origin ? 2.0 : 2.0 * w2 / d;
    } else {
        double* col = Kt + (size_t)j * 2 * n_inu;
        col[i] = origin ? 1.0 : w2 / d;
        col[n_inu + i] = origin ? 0.0 : w * nu / d;
    }
}

// LegendreKernel (not in the reference): the cuts of the host fill (kernels.py, LEGENDRE_*).
// Below a = beta |omega| / 2 = LEGENDRE_SERIES_CUT the scaled e^{-a} i_0(a) = (1 - e^{-2a}) / (2a) is its series
// 1 - a + 2 a^2 / 3 (next term a^3 / 3 < 4e-19); it covers omega = 0 exactly (no 0 / 0).  The backward recurrence of the
// ratios starts at L = m + LEGENDRE_START_PAD + floor(LEGENDRE_START_SQRT sqrt(m)), m = max(l_max, floor(a)): the wrong
// start r_L = 0 reaches order l multiplied by prod r_{k-1} r_k over k = l+1..L, below e^-72 for the sqrt term alone and
// below 2^-80 for the constant alone (kernels.py, _legendre_start).  LEGENDRE_L_MAX, LEGENDRE_A_MAX: the largest order and
// the largest a the entry takes (the work of a column grows like max(l_max, a)).
constexpr double LEGENDRE_SERIES_CUT = 1.0e-6;
constexpr double LEGENDRE_START_PAD = 40.0;
constexpr double LEGENDRE_START_SQRT = 6.0;
constexpr int LEGENDRE_L_MAX = 4096;
constexpr double LEGENDRE_A_MAX = 1.0e6;

// K^T[j][i] of LegendreKernel, K(l, omega) = -beta sqrt(2l+1) (-sgn omega)^l i_l(a) / (2 cosh a), a = beta |omega| / 2
// (i_l: modified spherical Bessel function of the first kind), column-major like tau_kernel_fill.  One thread owns a
// column and runs the host's recurrences (kernels.py, LegendreKernel._scaled_bessel) with contraction off:
//   down:  r_{k-1} = a / (2k + 1 + a r_k) from r_L = 0                     (r_k = i_{k+1} / i_k; a = 0 gives 0, no 0 / 0)
//   s_0 = e^{-a} i_0(a) = -expm1(-2a) / (2a), its series below the cut
//   up:    s_{k+1} = s_k r_k,   K = -beta sqrt(2l+1) (-sgn omega)^l s_l / (1 + e^{-2a})
// No exponent is positive: nothing overflows, small entries underflow to 0.  The column itself is the only storage: on
// the way down the slot of the q-th smallest order lam_q receives the product of the ratios r_k, lam_{q-1} <= k < lam_q
// (lam_{-1} = 0), on the way up s is multiplied by it and the slot receives K.  For l = 0..n-1 in any order every
// product is ONE ratio and the operations are the host's, one for one; a subset multiplies the same ratios in groups.
// lgrid: the n_l orders (integer-valued, 0 <= l <= l_max), then the n_l row indices sorted by ascending order.
__global__ __launch_bounds__(256)
void legendre_kernel_fill(const double* __restrict__ lgrid, const double* __restrict__ omega, double beta,
                          int l_max, int n_l, int n_omega, double* __restrict__ Kt)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_omega) return;
    const double* order = lgrid + n_l;
    double* col = Kt + (size_t)j * n_l;
    const double w = omega[j];
    const double a = beta * fabs(w) / 2.0;
    const double mm = fmax((double)l_max, floor(a));
    const int L = (int)(mm + LEGENDRE_START_PAD + floor(LEGENDRE_START_SQRT * sqrt(mm)));
    // down: group q holds the ratios r_k, lo <= k < hi
    int q = n_l - 1;
    int slot = (int)order[q];
    int hi = (int)lgrid[slot];
    int lo = q > 0 ? (int)lgrid[(int)order[q - 1]] : 0;
    double r = 0.0, prod = 1.0;
    for (int k = L; k >= 1 && q >= 0; --k) {
        r = a / ((double)(2 * k + 1) + a * r);              // r_{k-1}
        const int kk = k - 1;
        if (kk < hi) prod = prod * r;
        while (q >= 0 && kk == lo) {                        // (more than once: an order given twice has an empty group)
            col[slot] = prod;
            prod = 1.0;
            if (--q >= 0) {
                slot = (int)order[q];
                hi = lo;
                lo = q > 0 ? (int)lgrid[(int)order[q - 1]] : 0;
            }
        }
    }
    // up
    double s = (a < LEGENDRE_SERIES_CUT) ? 1.0 - a + 2.0 * a * a / 3.0 : -expm1(-2.0 * a) / (2.0 * a);
    const double den = 1.0 + exp(-2.0 * a);
    for (q = 0; q < n_l; ++q) {
        slot = (int)order[q];
        const double l = lgrid[slot];
        s = s * col[slot];
        const double v = -beta * sqrt(2.0 * l + 1.0) * s / den;
        col[slot] = (((int)l & 1) && w > 0.0) ? -v : v;    // (-sgn omega)^l
    }
}

// K^T[j][i] = K[i][j]: a caller-supplied matrix (row-major, n_rows x n_omega) into the column-major working layout of
// the decomposition (mxe_kernel_svd_data).  32 x 32 tiles through the LDS (33 columns: no bank conflicts), reads and
// writes both along the fast index; grid = (ceil(n_omega / 32), ceil(n_rows / 32)), block = (32, 8).
__global__ __launch_bounds__(256)
void data_kernel_transpose(const double* __restrict__ K, int n_rows, int n_omega, double* __restrict__ Kt)
{
    __shared__ double tile[32][33];
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i < n_rows && j < n_omega) tile[r][threadIdx.x] = K[(size_t)i * n_omega + j];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < n_rows && j < n_omega) Kt[(size_t)j * n_rows + i] = tile[threadIdx.x][r];
    }
}

__device__ __forceinline__ double gauss_blur(double wi, double wj, double b)
{
    const double d = wj - wi;
    return exp(-d * d / 2.0 / (b * b)) / sqrt(2.0 * 3.141592653589793 * b * b);
}

// r1[i] = sum_k delta_k G[k][i]   (first normalisation of get_preblur: rows)
__global__ __launch_bounds__(256)
void preblur_rows(const double* __restrict__ omega, const double* __restrict__ delta, double b,
                  int n_omega, double* __restrict__ r1)
{
    __shared__ double red[256];
    const int i = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < n_omega; k += 256) s += delta[k] * gauss_blur(omega[k], omega[i], b);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) r1[i] = red[0];
}

// d[j] = sum_c B1[j][c] delta_c with B1[j][c] = G[j][c] / r1[j]   (second normalisation: columns)
__global__ __launch_bounds__(256)
void preblur_cols(const double* __restrict__ omega, const double* __restrict__ delta, double b,
                  int n_omega, const double* __restrict__ r1, double* __restrict__ dcol)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int c = threadIdx.x; c < n_omega; c += 256) s += gauss_blur(omega[j], omega[c], b) / r1[j] * delta[c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) dcol[j] = red[0];
}

// B[j][l] = G[j][l] / r1[j] / d[l]   (the matrix get_preblur returns)
__global__ __launch_bounds__(256)
void preblur_matrix(const double* __restrict__ omega, double b, int n_omega,
                    const double* __restrict__ r1, const double* __restrict__ dcol, double* __restrict__ B)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_omega * n_omega) return;
    const int j = idx / n_omega, l = idx - j * n_omega;
    B[idx] = gauss_blur(omega[j], omega[l], b) / r1[j] / dcol[l];
}

// K'^T[l][i] = sum_j K^T[j][i] delta_j B[j][l]; block = one l, threads over i (coalesced K^T rows,
// the B column is block uniform)
__global__ __launch_bounds__(256)
void preblur_product(const double* __restrict__ Kt, const double* __restrict__ delta,
                     const double* __restrict__ B, int n_tau, int n_omega, double* __restrict__ Kbt)
{
    extern __shared__ double bcol[];          // [n_omega]  delta_j B[j][l]
    const int l = blockIdx.x;
    for (int j = threadIdx.x; j < n_omega; j += blockDim.x) bcol[j] = delta[j] * B[(size_t)j * n_omega + l];
    __syncthreads();
    for (int i = threadIdx.x; i < n_tau; i += blockDim.x) {
        double a0 = 0.0, a1 = 0.0;
        int j = 0;
        for (; j + 1 < n_omega; j += 2) {
            a0 = fma(Kt[(size_t)j * n_tau + i], bcol[j], a0);
            a1 = fma(Kt[(size_t)(j + 1) * n_tau + i], bcol[j + 1], a1);
        }
        if (j < n_omega) a0 = fma(Kt[(size_t)j * n_tau + i], bcol[j], a0);
        Kbt[(size_t)l * n_tau + i] = a0 + a1;
    }
}

__device__ __forceinline__ double svd_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

struct SvdParams {
    int m;              // n_tau   (rows of K)
    int n;              // n_omega (columns of K)
    int ns_max;         // capacity of the outputs
    double threshold;   // absolute cut on S
    // per batch item (stride = item index):
    double* A;          // [n][m]   K^T, destroyed (columns reduced in place)
    double* Vh;         // [RCAP][m] unit Householder vectors
    double* Rm;         // [RCAP][n] R, then diag(S) W^T
    double* Jt;         // [RCAP][RCAP] accumulated rotations (rows)
    double* Qc;         // [RCAP][m] columns of Q
    double* cn2;        // [n] remaining squared column norms
    int* perm;          // [n]
    double* out_U;      // [m][ns_max]
    double* out_S;      // [ns_max]
    double* out_V;      // [n][ns_max]
    int* out_info;      // [4]: n_s, rank of the QR stage, Jacobi sweeps, status (0 ok, 1 sweeps exhausted, 2 n_s > ns_max,
                        //      3 the QR stage reached SVD_RCAP rows with columns left above its stop cut: the numerical
                        //      rank of K exceeds SVD_RCAP and U, S, V are those of a rank-SVD_RCAP approximation, not of K)
};

__global__ __launch_bounds__(SVD_T)
void svd_kernel(const SvdParams p)
{
    extern __shared__ double sm[];
    const int item = blockIdx.x;
    const int m = p.m, n = p.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* A  = p.A  + (size_t)item * n * m;
    double* Vh = p.Vh + (size_t)item * SVD_RCAP * m;
    double* Rm = p.Rm + (size_t)item * SVD_RCAP * n;
    double* Jt = p.Jt + (size_t)item * SVD_RCAP * SVD_RCAP;
    double* Qc = p.Qc + (size_t)item * SVD_RCAP * m;
    double* cn2 = p.cn2 + (size_t)item * n;
    int* perm = p.perm + (size_t)item * n;
    double* out_U = p.out_U + (size_t)item * m * p.ns_max;
    double* out_S = p.out_S + (size_t)item * p.ns_max;
    double* out_V = p.out_V + (size_t)item * n * p.ns_max;
    int* out_info = p.out_info + (size_t)item * 4;

    double* vk = sm;                        // [m] current Householder vector
    double* redv = vk + m;                  // [SVD_NWAVE] reduction values
    int* redi = reinterpret_cast<int*>(redv + SVD_NWAVE);   // [SVD_NWAVE] reduction indices
    double* s2 = reinterpret_cast<double*>(redi + SVD_NWAVE);   // [RCAP] squared singular values
    int* order = reinterpret_cast<int*>(s2 + SVD_RCAP);     // [RCAP]
    __shared__ int sh_piv, sh_stop, sh_rot;
    __shared__ double sh_nrm0;

    // ---- column norms ----
    for (int j = wave; j < n; j += SVD_NWAVE) {
        double s = 0.0;
        for (int i = lane; i < m; i += 64) { const double x = A[(size_t)j * m + i]; s = fma(x, x, s); }
        s = svd_wave_sum(s);
        if (lane == 0) { cn2[j] = s; perm[j] = j; }
    }
    __syncthreads();

    // ---- 1. Householder QR with column pivoting, early stop ----
    const int kmax = min(min(m, n), SVD_RCAP);
    // a matrix with more rows and columns than SVD_RCAP gets one more pivot search after the last step: columns
    // still above the stop cut mean that R (SVD_RCAP rows) is not K to rounding, and its singular triplets not K's
    const int ksearch = kmax + ((kmax < min(m, n)) ? 1 : 0);
    int r = 0, capped = 0;
    for (int k = 0; k < ksearch; ++k) {
        // pivot = argmax_{j >= k} cn2[j] (lowest index on ties)
        double best = -1.0; int bi = k;
        for (int j = k + tid; j < n; j += SVD_T) { const double c = cn2[j]; if (c > best) { best = c; bi = j; } }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { redv[wave] = best; redi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            double bb = redv[0]; int ii = redi[0];
            for (int w2 = 1; w2 < SVD_NWAVE; ++w2)
                if (redv[w2] > bb || (redv[w2] == bb && redi[w2] < ii)) { bb = redv[w2]; ii = redi[w2]; }
            if (k == 0) sh_nrm0 = bb;
            const double eps = 2.220446049250313e-16;
            sh_stop = !(bb > eps * eps * sh_nrm0) || !(bb > 0.0);
            sh_piv = ii;
        }
        __syncthreads();
        if (sh_stop) break;
        if (k == kmax) { capped = 1; break; }
        const int piv = sh_piv;
        if (piv != k) {
            for (int i = tid; i < m; i += SVD_T) {
                const double x = A[(size_t)k * m + i];
                A[(size_t)k * m + i] = A[(size_t)piv * m + i];
                A[(size_t)piv * m + i] = x;
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
            for (int i = k + lane; i < m; i += 64) { const double x = A[(size_t)k * m + i]; s = fma(x, x, s); }
            s = svd_wave_sum(s);
            const double x0 = A[(size_t)k * m + k];
            const double nrm = sqrt(s);
            const double alpha = (x0 >= 0.0) ? -nrm : nrm;
            // v = x - alpha e0 ; |v|^2 = s - 2 alpha x0 + alpha^2 = 2 (s - alpha x0)
            const double vn = sqrt(2.0 * (s - alpha * x0));
            const double inv = (vn > 0.0) ? 1.0 / vn : 0.0;
            for (int i = lane; i < m; i += 64) {
                double v = 0.0;
                if (i >= k) v = ((i == k) ? (x0 - alpha) : A[(size_t)k * m + i]) * inv;
                vk[i] = v;
                Vh[(size_t)k * m + i] = v;
            }
            for (int i = k + lane; i < m; i += 64) A[(size_t)k * m + i] = (i == k) ? alpha : 0.0;
        }
        __syncthreads();
        // apply H_k = I - 2 v v^T to the columns j > k, one wavefront per column, four columns in
        // flight per wavefront (the loads of a column come from L2: latency, not bandwidth);
        // new remaining norms
        for (int j0 = k + 1 + wave; j0 < n; j0 += 4 * SVD_NWAVE) {
            constexpr int MR = 16;                       // rows per lane held in registers: m <= 64 * MR
            double s[4], rem[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s[q] = 0.0;
                const int j = min(j0 + q * SVD_NWAVE, n - 1);
                const double* col = A + (size_t)j * m;
                for (int i = k + lane; i < m; i += 64) s[q] = fma(vk[i], col[i], s[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] = 2.0 * svd_wave_sum(s[q]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rem[q] = 0.0;
                const int j = j0 + q * SVD_NWAVE;
                if (j < n) {
                    double* col = A + (size_t)j * m;
                    for (int i = k + lane; i < m; i += 64) {
                        const double x = fma(-s[q], vk[i], col[i]);
                        col[i] = x;
                        if (i > k) rem[q] = fma(x, x, rem[q]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rem[q] = svd_wave_sum(rem[q]);
                const int j = j0 + q * SVD_NWAVE;
                if (lane == 0 && j < n) cn2[j] = rem[q];
            }
            (void)MR;
        }
        __syncthreads();
        r = k + 1;
    }
    __syncthreads();

    // ---- R (r x n, row-major) and J^T = I ----
    const int rr = (r + 1) & ~1;              // even number of rows (a zero row pads an odd r)
    for (int idx = tid; idx < rr * n; idx += SVD_T) {
        const int kk = idx / n, j = idx - kk * n;
        Rm[idx] = (kk < r && j >= kk) ? A[(size_t)j * m + kk] : 0.0;
    }
    for (int idx = tid; idx < rr * SVD_RCAP; idx += SVD_T) {
        const int kk = idx / SVD_RCAP, l = idx - kk * SVD_RCAP;
        Jt[idx] = (kk == l) ? 1.0 : 0.0;
    }
    __syncthreads();

    // ---- 2. one-sided Jacobi on the rows of R, round-robin pairs, one wavefront per pair ----
    int sweeps = 0, status = 0;
    if (rr >= 2) {
        status = 1;
        for (int sweep = 0; sweep < SVD_MAX_SWEEPS; ++sweep) {
            if (tid == 0) sh_rot = 0;
            __syncthreads();
            for (int round = 0; round < rr - 1; ++round) {
                for (int pi = wave; pi < rr / 2; pi += SVD_NWAVE) {
                    int a, b;
                    if (pi == 0) { a = rr - 1; b = round % (rr - 1); }
                    else { a = (round + pi) % (rr - 1); b = (round - pi + 2 * (rr - 1)) % (rr - 1); }
                    const int pp = min(a, b), qq = max(a, b);
                    double* x = Rm + (size_t)pp * n;
                    double* y = Rm + (size_t)qq * n;
                    double aa = 0.0, bb = 0.0, gg = 0.0;
                    for (int j = lane; j < n; j += 64) {
                        const double xv = x[j], yv = y[j];
                        aa = fma(xv, xv, aa); bb = fma(yv, yv, bb); gg = fma(xv, yv, gg);
                    }
                    aa = svd_wave_sum(aa); bb = svd_wave_sum(bb); gg = svd_wave_sum(gg);
                    const double eps = 2.220446049250313e-16;
                    if (aa > 0.0 && bb > 0.0 && fabs(gg) > eps * sqrt(aa * bb)) {
                        const double zeta = (bb - aa) / (2.0 * gg);
                        const double t = ((zeta >= 0.0) ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                        for (int j = lane; j < n; j += 64) {
                            const double xv = x[j], yv = y[j];
                            x[j] = cs * xv - sn * yv;
                            y[j] = sn * xv + cs * yv;
                        }
                        double* jx = Jt + (size_t)pp * SVD_RCAP;
                        double* jy = Jt + (size_t)qq * SVD_RCAP;
                        for (int l = lane; l < r; l += 64) {
                            const double xv = jx[l], yv = jy[l];
                            jx[l] = cs * xv - sn * yv;
                            jy[l] = sn * xv + cs * yv;
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

    // ---- 3. singular values, order, truncation ----
    for (int kk = wave; kk < rr; kk += SVD_NWAVE) {
        double s = 0.0;
        for (int j = lane; j < n; j += 64) { const double x = Rm[(size_t)kk * n + j]; s = fma(x, x, s); }
        s = svd_wave_sum(s);
        if (lane == 0) s2[kk] = s;
    }
    __syncthreads();
    if (tid < rr) {
        const double mine = s2[tid];
        int rank = 0;
        for (int l = 0; l < rr; ++l) { const double o = s2[l]; if (o > mine || (o == mine && l < tid)) ++rank; }
        order[rank] = tid;
    }
    __syncthreads();
    int ns = 0;
    for (int kk = 0; kk < rr; ++kk) if (sqrt(s2[order[kk]]) >= p.threshold && s2[order[kk]] > 0.0) ns = kk + 1; else break;
    if (ns > p.ns_max) { ns = p.ns_max; status = 2; }
    if (capped) status = 3;
    // non-finite input: a NaN is never the pivot, spreads over its column of R and makes every comparison above false
    // (``order`` is then not a permutation); an Inf, or squares that overflow, stop the QR stage at its first step.
    // Nothing is returned for such a matrix.
    bool bad = !(sh_nrm0 >= 0.0 && sh_nrm0 <= 1.7976931348623157e308);
    for (int kk = 0; kk < rr; ++kk) if (s2[kk] != s2[kk]) bad = true;
    if (bad) { ns = 0; status = 1; }

    // Q = H_0 ... H_{r-1} [I_r ; 0], columns in Qc[l][i]
    for (int idx = tid; idx < r * m; idx += SVD_T) {
        const int l = idx / m, i = idx - l * m;
        Qc[idx] = (i == l) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int k = r - 1; k >= 0; --k) {
        for (int i = tid; i < m; i += SVD_T) vk[i] = Vh[(size_t)k * m + i];
        __syncthreads();
        for (int l = wave; l < r; l += SVD_NWAVE) {
            double* col = Qc + (size_t)l * m;
            double s = 0.0;
            for (int i = k + lane; i < m; i += 64) s = fma(vk[i], col[i], s);
            s = 2.0 * svd_wave_sum(s);
            for (int i = k + lane; i < m; i += 64) col[i] = fma(-s, vk[i], col[i]);
        }
        __syncthreads();
    }
    // outputs
    for (int kk = tid; kk < p.ns_max; kk += SVD_T) out_S[kk] = (kk < ns) ? sqrt(s2[order[kk]]) : 0.0;
    for (int idx = tid; idx < n * p.ns_max; idx += SVD_T) {
        const int j = idx / p.ns_max, kk = idx - j * p.ns_max;
        double val = 0.0;
        if (kk < ns) { const int row = order[kk]; val = Rm[(size_t)row * n + j] / sqrt(s2[row]); }
        out_V[(size_t)perm[j] * p.ns_max + kk] = val;
    }
    for (int idx = tid; idx < m * p.ns_max; idx += SVD_T) {
        const int i = idx / p.ns_max, kk = idx - i * p.ns_max;
        double val = 0.0;
        if (kk < ns) {
            const double* jrow = Jt + (size_t)order[kk] * SVD_RCAP;
            for (int l = 0; l < r; ++l) val = fma(Qc[(size_t)l * m + i], jrow[l], val);
        }
        out_U[idx] = val;
    }
    if (tid == 0) { out_info[0] = ns; out_info[1] = r; out_info[2] = sweeps; out_info[3] = status; }
}

} // namespace mxe
