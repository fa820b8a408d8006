// mxe_fullmatrix_logdet.hip.h -- the evidence of alpha of the whole-matrix continuation (nothing of the reference: it has
// neither the solver nor a probability of alpha for it).  DESIGN 4zb; the matrix analogue of mxe_logdet.
//
//   u of one (data set, alpha) pair  ->  log det(I_d + c W c / alpha) and the number of good data      fullmatrix_logdet_kernel<M, C>
//
// In the coordinates h_p,i = Tr(E_p H_i) the entropy has the Hessian -L^-1 (mxe_fullmatrix_postvar.hip.h), and the Gaussian
// integral around the minimiser of Q = chi2 / 2 - alpha S gives, as in the scalar case,
//   log p(alpha | G) = -1/2 log det(I_d + c W c / alpha) - Q - log alpha
//   log det(I_d + c W c / alpha) = sum_j log(l_jj^2 / alpha),   B = alpha I_d + c W c = L_B L_B^T,   d = P n_s
//   N_g = tr(c W c B^-1) = d - alpha |L_B^-1|_F^2
// Every pivot l_jj^2 of alpha I plus a positive semi-definite matrix is >= alpha: the sum has terms >= 0 only (up to the
// rounding of a pivot) and is formed as written, pivot by pivot -- never as log det B - d log alpha, which cancels at large alpha.
//
// One workgroup of 256 threads per job; the jobs are independent.  The parts:
//   1 - 3. fmpv_factor of mxe_fullmatrix_postvar.hip.h: the evaluation at u, L, B = alpha I + c W c on
//      v_mfma_f64_16x16x4_f64, the blocked Cholesky with its panel in the LDS;
//   4. the log-determinant: thread t adds the terms j = t, t + 256, ... in order, thread 0 adds the 256 sums in order;
//   5. (want_ngood) |L_B^-1|_F^2: the identity through fmpv_forward in blocks of 16 columns; the block of the columns
//      j0 ... j0 + 15 starts at row j0, the rows above being zero, so the pass costs sum_blocks 16 (d - j0)^2 / 2 = d^3 / 6
//      multiply-adds, as many as the Cholesky; the 16 sums |z_j|^2 of a block are added in order by thread 0.
// No atomics; every sum has one order that depends on d alone: the bits of a job do not depend on the batch or on the number
// of scratch slices, and logdet is written before part 5 starts, so its bits do not depend on want_ngood.
// A job whose u or H is not finite or whose B is not positive definite writes NaN to its outputs.
// Workgroup b takes the jobs b, b + gridDim.x, ... and works in slice b of the scratch (fmld_scratch_doubles each).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_fullmatrix_postvar.hip.h"

namespace mxe {

struct FullMatrixLogdetParams {
    int n_job, n_omega, n_s, want_ngood;
    const double* V;         // [n_omega][n_s]
    const double* c;         // [n_s]
    const double* D;         // [n_omega]
    const double* alpha;     // [n_job]
    const double* u;         // [n_job][P][n_s]
    double* scratch;         // [gridDim.x][fmld_scratch_doubles]
    double* out_logdet;      // [n_job]
    double* out_ngood;       // [n_job]   (want_ngood)
};

__host__ __device__ inline size_t fmld_scratch_doubles(int m, bool cplx, int nw, int ns)
{
    const size_t P = fm_P(m, cplx), d = P * ns, npair = P * (P + 1) / 2, mm = (size_t)m * m;
    // Gamma coordinates, H coordinates | W_i | D phi | L | B
    return 2 * P * nw + (cplx ? 2 : 1) * mm * nw + mm * nw + npair * nw + d * d;
}
// the dynamic LDS is that of the variance kernel, fmpv_lds_doubles(d): the panel, then the columns of the identity
// [d][FM_LDP] | partial sums [2][256] | sums [32] | flags

template <int M, bool C>
__global__ __launch_bounds__(FM_T)
void fullmatrix_logdet_kernel(const FullMatrixLogdetParams p)
{
    constexpr int P = C ? M * M : M * (M + 1) / 2, NPAIR = P * (P + 1) / 2, MM = M * M, WPL = C ? 2 : 1;
    extern __shared__ double fmld_smem[];
    const int tid = threadIdx.x;
    const int nw = p.n_omega, ns = p.n_s, d = P * ns;
    const double nan = __builtin_nan("");

    // ---- the LDS ----
    double* Ysh = fmld_smem;                         // [d][FM_LDP]: the panel, then columns of the identity
    double* part = Ysh + (size_t)d * FM_LDP;         // [2][256] partial sums
    double* fsh = part + 2 * FM_T;                   // [16] |z_j|^2 of a block
    int* flag = (int*)(fsh + 32);                    // [0] the job is bad, [1] B is positive definite so far

    // ---- the workgroup's slice of the scratch ----
    double* sc = p.scratch + (size_t)blockIdx.x * fmld_scratch_doubles(M, C, nw, ns);
    double* gam = sc;          sc += (size_t)P * nw;         // [P][nw] Gamma coordinates
    double* hc = sc;           sc += (size_t)P * nw;         // [P][nw] H coordinates
    double* Wv = sc;           sc += (size_t)WPL * MM * nw;  // [nw][WPL][M][M]
    double* phiD = sc;         sc += (size_t)MM * nw;        // [nw][M][M]
    double* Lp = sc;           sc += (size_t)NPAIR * nw;     // [NPAIR][nw]
    double* Bm = sc;                                         // [d][d]

    for (int job = blockIdx.x; job < p.n_job; job += gridDim.x) {
        const double alpha = p.alpha[job];

        // ================= 1 to 3. evaluation at u, L, B = alpha I + c W c = L_B L_B^T =================
        const bool job_ok = fmpv_factor<M, C>(p.V, p.c, p.D, p.u + (size_t)job * d, alpha, nw, ns, gam, hc, Wv, phiD, Lp, Bm,
                                              Ysh, flag);
        if (!job_ok) {
            if (tid == 0) {
                p.out_logdet[job] = nan;
                if (p.want_ngood) p.out_ngood[job] = nan;
            }
            __syncthreads();
            continue;
        }

        // ================= 4. log det(I + c W c / alpha) = sum_j log(l_jj^2 / alpha) =================
        {
            double s = 0.0;
            for (int j = tid; j < d; j += FM_T) {
                const double l = Bm[(size_t)j * d + j];
                s += log(l * l / alpha);
            }
            part[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int t = 0; t < FM_T; ++t) s += part[t];
            p.out_logdet[job] = s;
        }
        __syncthreads();

        // ================= 5. N_g = d - alpha |L_B^-1|_F^2 =================
        if (p.want_ngood) {
            double tr = 0.0;                                 // (thread 0)
            for (int j0 = 0; j0 < d; j0 += FMPV_NF) {
                for (int idx = tid; idx < (d - j0) * 16; idx += FM_T) {
                    const int j = idx & 15, row = j0 + (idx >> 4);
                    Ysh[row * FM_LDP + j] = row == j0 + j ? 1.0 : 0.0;
                }
                __syncthreads();
                const double q = fmpv_forward(Bm, d, Ysh, part, tid, j0);
                if (tid < 16) fsh[tid] = j0 + tid < d ? q : 0.0;
                __syncthreads();
                if (tid == 0)
                    for (int t = 0; t < 16; ++t) tr += fsh[t];
                __syncthreads();
            }
            if (tid == 0) {
                const double ng = (double)d - alpha * tr;    // (a NaN stays one: not fmax)
                p.out_ngood[job] = ng < 0.0 ? 0.0 : ng;
            }
        }
        __syncthreads();
    }
}

} // namespace mxe
