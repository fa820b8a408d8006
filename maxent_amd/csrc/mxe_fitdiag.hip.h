// mxe_fitdiag.hip.h -- diagnostics of a fit: leverages, number of good data, whitened residuals
//
//   nothing of the reference (it offers no diagnostics)          -> fitdiag_kernel   (mxe_fit_diagnostics)
//
// The hat matrix of a MaxEnt fit is the derivative of the fitted whitened data Sigma^-1/2 K H with respect to the
// whitened data Sigma^-1/2 G.  Differentiating the stationarity condition of Q = eta chi2 / 2 - alpha~ S at the minimiser
// gives (eta K^T Sigma^-1 K + alpha~ diag(1/w)) dH = eta K^T Sigma^-1 dG, and in the whitened singular basis
// (Sigma^-1/2 K = U^ c V'^T, a = alpha~ / eta) it collapses onto the matrix mxe_logdet factorises:
//
//   Hat   = U^ (I - a B^-1) U^^T,     B = c W c + a I = L L^T,   W = V'^T diag(w) V'
//   h_i   = |U^_i|^2 - a |L^-1 U^_i^T|^2                               (leverage of data point i)
//   N_g   = tr Hat = sum_i h_i = sum_k lambda_k / (lambda_k + a)       (number of good data; lambda: eigenvalues of c W c)
//   r_i   = sum_k U^_ik rho_k - rperp_i,   rho = c o V'^T H - g^,   rperp = G~ - U^ g^
//         = [Sigma^-1/2 (K H - G)]_i,      sum_i r_i^2 = |rho|^2 + c_perp = chi2
//
// (w = H for the normal entropy, sqrt(H^2 + 4 D^2) for the plus-minus one).  B^-1 is never formed.
//
// One workgroup (4 waves) per problem:
//   1. w, W, B and its Cholesky factor in LDS: factor_B (mxe_factor.hip.h), shared with logdet_kernel, postvar_kernel and
//      postsample_kernel;
//   2. h' = V'^T H: 256 / NP threads per singular direction over interleaved omega points, their partial sums added in
//      order; rho into LDS;
//   3. the data points in blocks of 16: the rows of U^ as the columns of a block of right-hand sides (pv_y), |U^_i|^2 and
//      sum_k U^_ik rho_k by one thread per data point in index order, then pv_forward_solve and the leverage, formed as
//      written (a difference that rounding makes negative is returned as 0; a NaN stays one);
//   4. N_g and chi2: lane 0 adds the 16 values of a block in index order (they sit in the lanes 0..15 of wave 0).
// LDS: logdet_kernel's plus NP doubles for rho.  No atomics; the bits of a problem do not depend on the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_factor.hip.h"

namespace mxe {

struct FitDiagParams : FactorParams {
    const double* ghat;         // [n_elem][NP]
    const double* U;            // U^ of every data set: [rows][n_s] at ds_off[3 ds]
    const long long* ds_off;    // [n_ds][3]: offset of U^, (offset of err), rows
    const double* rperp;        // rperp of every element: [rows] at elem_roff[e]
    const long long* elem_roff; // [n_elem]
    double* out_ngood;          // [P]
    double* out_chi2;           // [P]
    double* out_resid;          // [P][ld]
    double* out_lev;            // [P][ld]
    int ld;
};

inline size_t fitdiag_lds_bytes(int NP, int nwp) { return logdet_lds_bytes(NP, nwp) + (size_t)NP * sizeof(double); }

template <int NT>
__global__ __launch_bounds__(256)
void fitdiag_kernel(FitDiagParams p)
{
    constexpr int NP = 16 * NT, PARTS = 256 / NP;
    extern __shared__ double sm[];
    double* Bm = sm;                     // [NP][NP + 1]
    double* wsh = Bm + NP * (NP + 1);    // [nwp]
    double* flag = wsh + p.nwp;          // [4]
    double* rho = flag + 4;              // [NP]
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nw = p.nw, ns = p.ns, ld = p.ld;
    const size_t prob = blockIdx.x;
    const FactorProblem fp = resolve_problem<NP>(p, prob);
    const int e = p.elem[prob];
    const long long* o = p.ds_off + 3 * (size_t)p.elem_ds[e];
    const double* U = p.U + o[0];
    const int rows = (int)o[2];
    const double* rp = p.rperp + p.elem_roff[e];
    const double a = fp.a;
    double* resid = p.out_resid + prob * (size_t)ld;
    double* lev = p.out_lev + prob * (size_t)ld;
    for (int i = rows + tid; i < ld; i += 256) { resid[i] = 0.0; lev[i] = 0.0; }     // (behind the data set's rows)
    const bool ok = factor_B<NT>(fp, nw, p.nwp, ns, Bm, wsh, flag);
    if (!ok) {                                       // (uniform)
        const double nan = __builtin_nan("");
        for (int i = tid; i < rows; i += 256) { resid[i] = nan; lev[i] = nan; }
        if (tid == 0) { p.out_ngood[prob] = nan; p.out_chi2[prob] = nan; }
        return;
    }

    // ---- h' = V'^T H and rho = c o h' - g^ -----------------------------------------------------------------
    {
        const int k = tid % NP, part = tid / NP;
        double s = 0.0;
        for (int i = part; i < nw; i += PARTS) s = fma(fp.V[(size_t)i * NP + k], fp.Hp[i], s);
        Bm[pv_y<NP>(k, part)] = s;
    }
    __syncthreads();
    if (tid < NP) {
        double hk = 0.0;
#pragma unroll
        for (int part = 0; part < PARTS; ++part) hk += Bm[pv_y<NP>(tid, part)];
        rho[tid] = tid < ns ? fp.cc[tid] * hk - p.ghat[(size_t)e * NP + tid] : 0.0;
    }
    __syncthreads();

    // ---- the data points, 16 at a time ----------------------------------------------------------------------
    double ngood = 0.0, chi2 = 0.0;                  // (lane 0 of wave 0)
    for (int i0 = 0; i0 < rows; i0 += 16) {
        for (int idx = tid; idx < ns * 16; idx += 256) {     // (k fastest: neighbouring lanes read neighbouring doubles of a row of U^)
            const int j = idx / ns, k = idx - j * ns;
            Bm[pv_y<NP>(k, j)] = (i0 + j < rows) ? U[(size_t)(i0 + j) * ns + k] : 0.0;
        }
        __syncthreads();
        double u2 = 0.0, ur = 0.0;
        if (tid < 16) {
            for (int k = 0; k < ns; ++k) {
                const double u = Bm[pv_y<NP>(k, tid)];
                u2 = fma(u, u, u2);
                ur = fma(u, rho[k], ur);
            }
        }
        const double q = pv_forward_solve<NP>(Bm, ns, tid);
        if (wave == 0) {                             // (uniform per wave: the lanes 16..63 carry zeros)
            const bool valid = tid < 16 && i0 + tid < rows;
            const double d = u2 - a * q;             // (a NaN stays one: not fmax)
            const double h = valid ? (d < 0.0 ? 0.0 : d) : 0.0;
            const double r = valid ? ur - rp[i0 + tid] : 0.0;
            if (valid) { lev[i0 + tid] = h; resid[i0 + tid] = r; }
            const double r2 = r * r;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                ngood += __shfl(h, j);
                chi2 += __shfl(r2, j);
            }
        }
        // (pv_forward_solve ended with a barrier and nothing reads the block after it: the next one may be loaded)
    }
    if (tid == 0) { p.out_ngood[prob] = ngood; p.out_chi2[prob] = chi2; }
}

} // namespace mxe
