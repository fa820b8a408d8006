// mxe_response.hip.h -- the linear response of the minimiser: resolution operator, response to the data
//
//   nothing of the reference (it offers chi2(alpha) only)          -> response_kernel   (mxe_response)
//
// Differentiating the stationarity condition of Q = eta chi2 / 2 - alpha~ S at the minimiser gives
// (eta K^T Sigma^-1 K + alpha~ diag(1/w)) dH = eta K^T Sigma^-1 dG, and in the whitened singular basis
// (Sigma^-1/2 K = U^ c V'^T, a = alpha~ / eta) it collapses onto the matrix mxe_logdet factorises:
//
//   B  = c W c + a I = L L^T,   W = V'^T diag(w) V'
//   dH = diag(w) V' c B^-1 U^^T dG~                        response to a whitened perturbation of the data (space 1)
//   dH = R f,   R = diag(w) S,   S = V' c B^-1 c V'^T      response to a perturbation f of the true H (space 0); S is
//                                                          symmetric, tr R = sum_k lambda_k / (lambda_k + a) = N_g
//
// (w = H for the normal entropy, sqrt(H^2 + 4 D^2) for the plus-minus one).  Only a enters, so eta needs no scaling of
// the result.  The response to the default model is (I - R)(H o dlnD): the caller subtracts.
//
// One workgroup (4 waves) per problem:
//   1. w, W, B and its Cholesky factor in LDS: factor_B (mxe_factor.hip.h), shared with logdet_kernel, postvar_kernel,
//      postsample_kernel and fitdiag_kernel;
//   2. the right-hand sides in blocks of 16 (pv_y; a short last block is padded with zero columns):
//        a. space 0: Y = c o V'^T F^T as one sweep of f64 MFMAs over the omega rows -- they go to the four waves round-robin
//           in groups of 4, the waves' partial tiles are added in wave order;
//           space 1: Y = U^^T F^T, one thread per (singular direction, right-hand side), the data rows in index order;
//        b. pv_forward_solve, then ps_backward_solve: x = L^-T L^-1 y (B^-1 is never formed);
//        c. c o x in the block;
//        d. X = V' (c o x) by block_times_Vt, a tile of 16 right-hand sides x 16 omega points each, times w_i when
//           `weighted`.
// LDS: logdet_kernel's, nothing more.  No atomics; the bits of a column depend on neither the other problems, nor n_rhs,
// nor the column's place among the right-hand sides: a column of a tile never meets another column's, a tile's k-sum
// runs inside one MFMA chain, every other sum runs in index order in one thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_factor.hip.h"

namespace mxe {

struct ResponseParams : FactorParams {
    const double* F;            // [P][n_rhs][ld]
    const double* U;            // U^ of every data set: [rows][n_s] at ds_off[3 ds]  (space 1)
    const long long* ds_off;    // [n_ds][3]: offset of U^, (offset of err), rows      (space 1)
    double* out;                // [P][n_rhs][n_omega]
    int n_rhs, ld, space, weighted;
};

inline size_t response_lds_bytes(int NP, int nwp) { return logdet_lds_bytes(NP, nwp); }

template <int NT>
__global__ __launch_bounds__(256)
void response_kernel(ResponseParams p)
{
    constexpr int NP = 16 * NT;
    extern __shared__ double sm[];
    double* Bm = sm;                     // [NP][NP + 1]
    double* wsh = Bm + NP * (NP + 1);    // [nwp]
    double* flag = wsh + p.nwp;          // [4]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.nw, ns = p.ns, n_rhs = p.n_rhs, ld = p.ld;
    const size_t prob = blockIdx.x;
    const FactorProblem fp = resolve_problem<NP>(p, prob);
    const double* V = fp.V;
    const double* cc = fp.cc;
    const bool ok = factor_B<NT>(fp, nw, p.nwp, ns, Bm, wsh, flag);
    const int kq = lane >> 4, cn = lane & 15;
    const int n_groups = (nw + 3) >> 2;          // (the rows of V' behind n_omega are zero)
    const int ntile = (ns + 15) >> 4;
    double* out = p.out + prob * (size_t)n_rhs * nw;
    if (!ok) {                                       // (uniform)
        const double nan = __builtin_nan("");
        for (size_t i = tid; i < (size_t)n_rhs * nw; i += 256) out[i] = nan;
        return;
    }
    const double* Fp = p.F + prob * (size_t)n_rhs * ld;
    const double* U = nullptr;
    int rows = 0;
    if (p.space) {
        const long long* o = p.ds_off + 3 * (size_t)p.elem_ds[p.elem[prob]];
        U = p.U + o[0];
        rows = (int)o[2];
    }
    const int n_wtiles = (nw + 15) >> 4;
    const int kgroups = 4 * ntile;                   // groups of 4 singular directions (columns behind n_s: zero)

    // ---- the right-hand sides, 16 at a time ----------------------------------------------------------------
    for (int r0 = 0; r0 < n_rhs; r0 += 16) {
        for (int idx = tid; idx < NP * 16; idx += 256) Bm[pv_y<NP>(idx >> 4, idx & 15)] = 0.0;
        __syncthreads();
        if (p.space == 0) {
            // a. y = c o V'^T f
            const int j = r0 + cn;
            const bool jv = j < n_rhs;
            const double* Fr = Fp + (size_t)(jv ? j : 0) * ld;
            d4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
            for (int g = wave; g < n_groups; g += 4) {
                const int i = 4 * g + kq;
                const double b = (jv && i < nw) ? Fr[i] : 0.0;
                const double* row = V + (size_t)i * NP + cn;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * t], b, acc[t], 0, 0, 0);
            }
            add_tiles_in_wave_order<NT>(Bm, acc, 0, ntile, wave, [=](int t, int r) { return pv_y<NP>(16 * t + kq + 4 * r, cn); });
            for (int idx = tid; idx < ntile * 256; idx += 256) {         // (rows behind n_s stay zero whatever V' holds there)
                const int k = idx >> 4;
                Bm[pv_y<NP>(k, idx & 15)] = k < ns ? Bm[pv_y<NP>(k, idx & 15)] * cc[k] : 0.0;
            }
        } else {
            // a. y = U^^T g~ (k fastest: neighbouring lanes read neighbouring doubles of a row of U^)
            for (int idx = tid; idx < ns * 16; idx += 256) {
                const int j = idx / ns, k = idx - j * ns;
                double s = 0.0;
                if (r0 + j < n_rhs) {
                    const double* Fr = Fp + (size_t)(r0 + j) * ld;
                    for (int i = 0; i < rows; ++i) s = fma(U[(size_t)i * ns + k], Fr[i], s);
                }
                Bm[pv_y<NP>(k, j)] = s;
            }
        }
        __syncthreads();
        // b. x = L^-T L^-1 y
        pv_forward_solve<NP>(Bm, ns, tid);
        ps_backward_solve<NP>(Bm, ns, tid);
        // c. c o x
        for (int idx = tid; idx < ns * 16; idx += 256) Bm[pv_y<NP>(idx >> 4, idx & 15)] *= cc[idx >> 4];
        __syncthreads();
        // d. X = V' (c o x), times w when weighted
        for (int T = wave; T < n_wtiles; T += 4) {
            const int i = 16 * T + cn;               // this lane's omega point; its right-hand sides are r0 + kq + 4 r
            const bool iv = i < nw;
            const d4 acc = block_times_Vt<NP>(Bm, V, i, iv, kgroups, kq, cn);
            if (iv) {
                const double w = p.weighted ? wsh[i] : 1.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = r0 + kq + 4 * r;
                    if (j < n_rhs) out[(size_t)j * nw + i] = w * acc[r];
                }
            }
        }
        __syncthreads();                             // (the block is free again)
    }
}

} // namespace mxe
