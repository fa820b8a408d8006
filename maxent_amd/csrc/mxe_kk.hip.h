// mxe_kk.hip.h -- the broadened Kramers-Kronig (Cauchy / Hilbert) sum of get_G_w_from_A_w
//
//   get_G_w_from_A_w   maxent_util.py:43-132   -> kk_partial + kk_combine   (mxe_kramers_kronig)
//
//   G[s][o] = sum_j  A[s][j] * weight[j] / (w_out[o] - w[j] + i eta[j])
//
// with c_oj = weight[j] / (x + i eta[j]) = weight[j] (x - i eta[j]) / (x^2 + eta[j]^2), x = w_out[o] - w[j]: one
// binary64 division per (o, j), IEEE-correct (hipcc's v_div_scale / v_rcp / Newton / v_div_fixup sequence, no fast
// math).  One thread owns one output point o and TS spectra of a tile: it generates each c_oj exactly once for its
// workgroup and applies it to all TS spectra (2 FMAs per spectrum); the TS values A[s][j] of a j-chunk are staged
// in LDS and read back as broadcasts.
//
// Bits do not depend on batching: the j range is cut into slices of KK_SLICE values, a function of n_w alone.  The
// sum of one slice runs over j in increasing order from 0 (fma(A, c, acc)); the slices' partial sums are added in
// increasing slice order, starting from slice 0's.  Whether one workgroup adds them as it goes (COMBINE: many
// spectra, enough workgroups without splitting) or one workgroup per slice writes its partial and kk_combine adds
// them (few spectra: the slices are the parallelism), every spectrum goes through the same operations in the same
// order -- alone, at any place of any batch, in any launch.  No atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxe {

constexpr int KK_T = 256;          // threads of a workgroup = output points of its tile
constexpr int KK_SLICE = 256;      // j values of a slice (the unit of the fixed-order reduction)
constexpr int KK_CHUNK = 64;       // j values staged in LDS at a time (KK_SLICE is a multiple)

struct KKParams {
    const double* w;          // n_w
    const double* weight;     // n_w
    const double* eta;        // n_w
    const double* w_out;      // n_out
    const double* A;          // n_spec x n_w
    double* out;              // COMBINE: n_spec x n_out x 2 (the result); else n_slice x n_spec x n_out x 2 (partials)
    int n_w, n_out, n_spec, n_slice;
};

// grid: (ceil(n_spec / TS), ceil(n_out / KK_T), COMBINE ? 1 : n_slice)
template <int TS, bool COMBINE>
__global__ __launch_bounds__(KK_T) void kk_partial(KKParams p)
{
    __shared__ __align__(16) double sA[KK_CHUNK * TS];           // [j][s]: the TS values of one j side by side
    __shared__ double sw[KK_CHUNK], swt[KK_CHUNK], seta[KK_CHUNK];
    const int t = threadIdx.x;
    const int o = blockIdx.y * KK_T + t;
    const int s0 = blockIdx.x * TS;
    const double x0 = o < p.n_out ? p.w_out[o] : 0.0;
    double tot_re[TS], tot_im[TS];
#pragma unroll
    for (int k = 0; k < TS; ++k) { tot_re[k] = 0.0; tot_im[k] = 0.0; }
    const int sl_first = COMBINE ? 0 : (int)blockIdx.z;
    const int sl_end = COMBINE ? p.n_slice : (int)blockIdx.z + 1;
    for (int sl = sl_first; sl < sl_end; ++sl) {
        double acc_re[TS], acc_im[TS];
#pragma unroll
        for (int k = 0; k < TS; ++k) { acc_re[k] = 0.0; acc_im[k] = 0.0; }
        const int jb = sl * KK_SLICE;
        const int je = min(jb + KK_SLICE, p.n_w);
        for (int j0 = jb; j0 < je; j0 += KK_CHUNK) {
            const int nj = min(KK_CHUNK, je - j0);
            __syncthreads();                       // (the previous chunk's readers are done)
            for (int i = t; i < KK_CHUNK * TS; i += KK_T) {
                const int s = i / KK_CHUNK, jj = i - s * KK_CHUNK;
                double a = 0.0;
                if (jj < nj && s0 + s < p.n_spec) a = p.A[(size_t)(s0 + s) * p.n_w + j0 + jj];
                sA[jj * TS + s] = a;
            }
            if (t < nj) { sw[t] = p.w[j0 + t]; swt[t] = p.weight[j0 + t]; seta[t] = p.eta[j0 + t]; }
            __syncthreads();
            for (int jj = 0; jj < nj; ++jj) {
                const double x = x0 - sw[jj];
                const double e = seta[jj];
                const double r = swt[jj] / __fma_rn(x, x, e * e);
                const double c_re = x * r, c_im = -(e * r);
                const double2* a2 = reinterpret_cast<const double2*>(sA + jj * TS);
#pragma unroll
                for (int k = 0; k < TS / 2; ++k) {
                    const double2 a = a2[k];
                    acc_re[2 * k] = __fma_rn(a.x, c_re, acc_re[2 * k]);
                    acc_im[2 * k] = __fma_rn(a.x, c_im, acc_im[2 * k]);
                    acc_re[2 * k + 1] = __fma_rn(a.y, c_re, acc_re[2 * k + 1]);
                    acc_im[2 * k + 1] = __fma_rn(a.y, c_im, acc_im[2 * k + 1]);
                }
            }
        }
        if (sl == 0) {
#pragma unroll
            for (int k = 0; k < TS; ++k) { tot_re[k] = acc_re[k]; tot_im[k] = acc_im[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < TS; ++k) { tot_re[k] += acc_re[k]; tot_im[k] += acc_im[k]; }
        }
    }
    if (o >= p.n_out) return;
    // (split: slice sl's partials at out[sl][s][o]; combined: the result at out[s][o])
    const size_t base = COMBINE ? 0 : (size_t)blockIdx.z * p.n_spec;
#pragma unroll
    for (int k = 0; k < TS; ++k)
        if (s0 + k < p.n_spec)
            reinterpret_cast<double2*>(p.out)[(base + s0 + k) * p.n_out + o] = make_double2(tot_re[k], tot_im[k]);
}

// the partials of kk_partial<TS, false> (n_slice x n) added in slice order: out[i] = ((P0[i] + P1[i]) + P2[i]) + ...
// n = n_spec * n_out complex values
__global__ __launch_bounds__(256) void kk_combine(const double2* __restrict__ part, int n_slice, size_t n,
                                                  double2* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double2 v = part[i];
    for (int sl = 1; sl < n_slice; ++sl) {
        const double2 q = part[(size_t)sl * n + i];
        v.x += q.x;
        v.y += q.y;
    }
    out[i] = v;
}

} // namespace mxe
