// mxe_postvar.hip.h -- posterior (Gaussian) variances of linear functionals of the hidden image
//
//   nothing of the reference (it offers no error bars)          -> postvar_kernel   (mxe_posterior_var)
//
// Around the minimiser of Q = eta chi2 / 2 - alpha~ S the posterior covariance of H is the inverse Hessian
// (Bryan 1990; Jarrell & Gubernatis 1996, section 5).  With the whitened singular basis (K^T Sigma^-1 K = V' c^2 V'^T)
// and a = alpha~ / eta it collapses onto the matrix mxe_logdet factorises:
//
//   Gamma      = (K^T Sigma^-1 K + a diag(1/w))^-1 = (1/a) [ diag(w) - diag(w) V' c B^-1 c V'^T diag(w) ]
//   B          = c W c + a I,   W = V'^T diag(w) V',   B = L L^T
//   var(f^T H) = (1/a) [ sum_i w_i f_i^2 - |L^-1 y|^2 ],   y = c o V'^T (w o f)
//   Gamma_ii   = (w_i / a) [ 1 - w_i |L^-1 (c o V'_i)|^2 ]
//
// (w = H for the normal entropy, sqrt(H^2 + 4 D^2) for the plus-minus one).  Both are differences of two sums of
// non-negative terms; B^-1 is never formed.  For eta != 1 the caller divides the result by eta.
//
// One workgroup (4 waves) per problem:
//   1. w from the H row, W by v_mfma_f64_16x16x4_f64, B and its Cholesky factor in LDS: factor_B (mxe_factor.hip.h),
//      shared with logdet_kernel and postsample_kernel;
//   2. the functionals in blocks of 16 (F is streamed from device memory, never held): Y = c o V'^T (w o F^T) as one
//      sweep of f64 MFMAs over the omega rows (one 16 x 16 tile of Y per tile row of V'), the prior sums
//      sum_i w_i f_i^2, then the blocked forward substitution L Z = Y in LDS -- the 16 x 16 diagonal block of a tile
//      row by one thread per functional, the rows below it by all threads -- and |z|^2;
//   3. for the diagonal the same substitution on blocks of 16 columns c o V'_i, loaded as they are.
// No column of Y lives in registers, so the 128-row build needs no more of them than the 64-row one.  A block of 16
// right-hand sides lives in LDS that B leaves free (pv_y, mxe_factor.hip.h).  The kernel so needs logdet_kernel's LDS
// plus 2.3 KB and keeps its four workgroups per CU at NP = 64.
//
// Bits do not depend on the batch, on n_f or on a functional's place in F: the omega rows go to the four waves
// round-robin and the waves' partial tiles are added in wave order; every other sum runs in index order in one thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_factor.hip.h"

namespace mxe {

struct PostVarParams : FactorParams {
    const double* F;            // [n_f][n_omega], may be NULL with n_f == 0
    double* out_var;            // [P][n_f]
    double* out_prior;          // [P][n_f] or NULL
    double* out_diag;           // [P][n_omega] or NULL
    int n_f;
};

inline size_t postvar_lds_bytes(int NP, int nwp)
{
    return ((size_t)NP * (NP + 1) + (size_t)nwp + 256 + 32) * sizeof(double);
}

template <int NT>
__global__ __launch_bounds__(256)
void postvar_kernel(PostVarParams p)
{
    constexpr int NP = 16 * NT;
    extern __shared__ double sm[];
    double* Bm = sm;                     // [NP][NP + 1]
    double* wsh = Bm + NP * (NP + 1);    // [nwp]
    double* part = wsh + p.nwp;          // [16][16] partial prior sums
    double* fsh = part + 256;            // [16] prior sums | [16] flag
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.nw, ns = p.ns, n_f = p.n_f;
    const size_t prob = blockIdx.x;
    const FactorProblem fp = resolve_problem<NP>(p, prob);
    const double* V = fp.V;
    const double* cc = fp.cc;
    const double a = fp.a;
    const bool ok = factor_B<NT>(fp, nw, p.nwp, ns, Bm, wsh, fsh + 16);
    const int kq = lane >> 4, cn = lane & 15;
    const int n_groups = (nw + 3) >> 2;          // (the rows of V' behind n_omega are zero)
    const int ntile = (ns + 15) >> 4;
    const double nan = __builtin_nan("");
    if (!ok) {                                       // (uniform)
        for (int j = tid; j < n_f; j += 256) {
            p.out_var[prob * n_f + j] = nan;
            if (p.out_prior) p.out_prior[prob * n_f + j] = nan;
        }
        if (p.out_diag) for (int i = tid; i < nw; i += 256) p.out_diag[prob * nw + i] = nan;
        return;
    }

    // ---- the functionals, 16 at a time --------------------------------------------------------------------
    for (int f0 = 0; f0 < n_f; f0 += 16) {
        for (int i = tid; i < NP * 16; i += 256) Bm[pv_y<NP>(i >> 4, i & 15)] = 0.0;
        const int jf = f0 + cn;
        const bool jv = jf < n_f;
        const double* Fr = p.F + (size_t)(jv ? jf : 0) * nw;
        d4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
        for (int g = wave; g < n_groups; g += 4) {
            const int i = 4 * g + kq;
            const double b = (jv && i < nw) ? wsh[i] * Fr[i] : 0.0;
            const double* row = V + (size_t)i * NP + cn;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * t], b, acc[t], 0, 0, 0);
        }
        {   // prior sums: 16 threads per functional over interleaved omega points, added in order below
            const int j = tid & 15, pt = tid >> 4;
            const int jj = f0 + j;
            double s = 0.0;
            if (jj < n_f) {
                const double* Fj = p.F + (size_t)jj * nw;
                for (int i = pt; i < nw; i += 16) { const double f = Fj[i]; s = fma(wsh[i] * f, f, s); }
            }
            part[pt * 16 + j] = s;
        }
        __syncthreads();
        add_tiles_in_wave_order<NT>(Bm, acc, 0, ntile, wave, [=](int t, int r) { return pv_y<NP>(16 * t + kq + 4 * r, cn); });
        for (int idx = tid; idx < ns * 16; idx += 256) Bm[pv_y<NP>(idx >> 4, idx & 15)] *= cc[idx >> 4];
        if (tid < 16) {
            double s = 0.0;
            for (int pt = 0; pt < 16; ++pt) s += part[pt * 16 + tid];
            fsh[tid] = s;
        }
        __syncthreads();
        const double q = pv_forward_solve<NP>(Bm, ns, tid);
        if (tid < 16 && f0 + tid < n_f) {
            const double prior = fsh[tid];
            const double d = prior - q;                  // (a NaN stays one: not fmax)
            p.out_var[prob * n_f + f0 + tid] = (d < 0.0 ? 0.0 : d) / a;
            if (p.out_prior) p.out_prior[prob * n_f + f0 + tid] = prior / a;
        }
        __syncthreads();
    }

    // ---- the diagonal: the columns c o V'_i through the same L ---------------------------------------------
    if (p.out_diag) {
        for (int i0 = 0; i0 < nw; i0 += 16) {
            for (int idx = tid; idx < ns * 16; idx += 256) {     // (k fastest: neighbouring lanes read neighbouring doubles of a row of V')
                const int j = idx / ns, k = idx - j * ns;
                Bm[pv_y<NP>(k, j)] = (i0 + j < nw) ? cc[k] * V[(size_t)(i0 + j) * NP + k] : 0.0;
            }
            __syncthreads();
            const double q = pv_forward_solve<NP>(Bm, ns, tid);
            if (tid < 16 && i0 + tid < nw) {
                const double w = wsh[i0 + tid];
                const double d = 1.0 - w * q;
                p.out_diag[prob * nw + i0 + tid] = (w / a) * (d < 0.0 ? 0.0 : d);
            }
            __syncthreads();
        }
    }
}

} // namespace mxe
