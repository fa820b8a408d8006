// mxe_mock.hip.h -- mock data of a parametric bootstrap (no counterpart in the reference, whose users loop run() by hand)
//
//   a hidden image H0 per set, the job's kernel K, the job's error bars   ->  G[s][k] = (T_s) K H0_s + err_s o z_k   mock_data_kernel
//
// What is sampled: data from N(K H0, diag(err^2)) in the data space of the job (the eigenbasis of a covariance, the stacked
// real form of Matsubara data: whatever K and err of the job are in), NOT a posterior.  z_k is sample k of the stream
// (seed, stream[s]) of normal_pair (mxe_postsample.hip.h): what mxe_normals(seed, stream[s], n_mock, n_data) returns.
//
// One workgroup (4 wavefronts) per (tile of 16 sets, chunk of MOCK_CHUNK mocks), all sets of a job in one launch:
//   1. m = K H0 of the 16 sets: (n_data x n_omega) (n_omega x 16) as v_mfma_f64_16x16x4_f64 tiles.  A wavefront owns a tile of
//      16 data rows and runs over ALL omega in index order: no sum is split between wavefronts.  Edges are padded with zeros
//      in the operands.  Every chunk of mocks forms m again -- the same instructions on the same numbers, the same bits --
//      rather than wait for another workgroup: K is a few hundred KB and stays in L2.
//   2. with a rotation: m <- T_s m, one wavefront per row of T_s, lanes over the columns, butterfly sum (the "T mean" of
//      bins_resample_kernel); rows >= rank are zeros.
//   3. the epilogue: one thread per Box-Muller pair, G = fma(err, z, m); rows >= rank are written as zeros.
// A set's column of a tile never meets another set's: its output depends on nothing but its own H0, err, T, rank and stream
// and on the shared K -- the same bits alone or in a batch, and from call to call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_bins.hip.h"
#include "mxe_postsample.hip.h"

namespace mxe {

constexpr int MOCK_T = 256;              // threads of a workgroup
constexpr int MOCK_CHUNK = 8;            // mocks a workgroup writes (at least: the launch keeps gridDim.y <= 1024)

struct MockParams {
    int n_sets, n_mock, n_data, nw;
    int chunk;               // mocks per workgroup
    const double* K;         // [n_data][nw]
    const double* H0;        // [n_sets][nw]
    const double* err;       // [n_sets][n_data]
    const double* T;         // [n_sets][n_data][n_data] or NULL
    const int* rank;         // [n_sets] or NULL
    const uint64_t* stream;  // [n_sets]
    uint64_t seed;
    double* kh;              // [gridDim.y][n_sets][n_data]  K H0 before the rotation (unused without T)
    double* mdl;             // [gridDim.y][n_sets][n_data]  the model as this workgroup formed it
    double* out_model;       // [n_sets][n_data]
    double* out_G;           // [n_sets][n_mock][n_data]
};

__global__ __launch_bounds__(MOCK_T)
void mock_data_kernel(const MockParams p)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int n = p.n_data, nw = p.nw, n_sets = p.n_sets;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, cn = lane & 15;
    const int s0 = 16 * blockIdx.x;
    const int ns_here = min(16, n_sets - s0);
    double* kh = p.kh + (size_t)blockIdx.y * n_sets * n;
    double* mdl = p.mdl + (size_t)blockIdx.y * n_sets * n;

    // ---- 1. m = K H0 ----
    {
        double* dst = p.T ? kh : mdl;
        const int ct_n = (n + 15) >> 4;
        const int sb = s0 + cn;
        const bool sv = sb < n_sets;
        const double* hrow = p.H0 + (size_t)(sv ? sb : s0) * nw;
        for (int I = wave; I < ct_n; I += MOCK_T / 64) {
            const int ra = 16 * I + cn;
            const bool rv = ra < n;
            const double* krow = p.K + (size_t)(rv ? ra : 0) * nw;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int w0 = 0; w0 < nw; w0 += 4) {
                const int w = w0 + kq;
                const bool wv = w < nw;
                const double a = (rv && wv) ? krow[w] : 0.0;
                const double b = (sv && wv) ? hrow[w] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 16 * I + kq + 4 * q;
                if (i < n && sv) dst[(size_t)sb * n + i] = acc[q];
            }
        }
    }
    __syncthreads();                                     // (the products are complete; other wavefronts read them)

    // ---- 2. m <- T m ----
    if (p.T) {
        for (int item = wave; item < ns_here * n; item += MOCK_T / 64) {
            const int s = s0 + item / n, k = item % n;
            const int rank = p.rank[s];
            const double* Trow = p.T + ((size_t)s * n + k) * n;
            const double* x = kh + (size_t)s * n;
            double sum = 0.0;
            if (k < rank)
                for (int j = lane; j < n; j += 64) sum = fma(Trow[j], x[j], sum);
            sum = bins_wave_sum(sum);
            if (lane == 0) mdl[(size_t)s * n + k] = (k < rank) ? sum : 0.0;
        }
        __syncthreads();
    }
    if (blockIdx.y == 0)
        for (int idx = tid; idx < ns_here * n; idx += MOCK_T)
            p.out_model[(size_t)s0 * n + idx] = mdl[(size_t)s0 * n + idx];

    // ---- 3. G = m + err z ----
    const int k0 = blockIdx.y * p.chunk;
    const int nk = min(p.chunk, p.n_mock - k0);
    const int npair = (n + 1) >> 1;
    const int per_set = nk * npair;
    for (int idx = tid; idx < ns_here * per_set; idx += MOCK_T) {
        const int sl = idx / per_set, rem = idx - sl * per_set;
        const int k = k0 + rem / npair, j = rem % npair;
        const int s = s0 + sl;
        const int rank = p.rank ? p.rank[s] : n;
        const int i = 2 * j;
        double za = 0.0, zb = 0.0;
        if (i < rank) normal_pair(p.seed, p.stream[s], (uint32_t)k, (uint32_t)j, za, zb);
        const double* m = mdl + (size_t)s * n;
        const double* e = p.err + (size_t)s * n;
        double* g = p.out_G + ((size_t)s * p.n_mock + k) * n;
        g[i] = (i < rank) ? fma(e[i], za, m[i]) : 0.0;
        if (i + 1 < n) g[i + 1] = (i + 1 < rank) ? fma(e[i + 1], zb, m[i + 1]) : 0.0;
    }
}

} // namespace mxe
