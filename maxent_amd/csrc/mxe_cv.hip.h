// mxe_cv.hip.h -- out-of-sample chi2 of hidden images against held-out data: k-fold cross-validation of alpha over Monte
// Carlo bins (no counterpart in the reference, which has no bins)
//
//   the H rows of the training scans, the job's kernel K, per group a rotation T, validation data and weights
//       ->  z[r][k] = sqrt(w[g][k]) ((T_g K H_r)[k] - Gval[g][k]),  score[r] = sum_k z[r][k]^2      cv_score_kernel
//   the finite rows of every group                                                                  cv_used_kernel
//
// A group is one (matrix element, fold); its rows are the alphas of that fold's training scan.
//
// cv_score_kernel: one workgroup (4 wavefronts) per tile of 16 rows of ONE group (the host lists the tiles; a tile never
// spans two groups, so one T, Gval and w serve it).
//   1. is a row finite -- a failed alpha leaves NaN --: one wavefront per row, the rule of resample_reduce_kernel.  A row that
//      is not enters the products below as zeros and is written as NaN at the end: it never meets its neighbours.
//   2. m = K H of the 16 rows: (n_data x n_omega) (n_omega x 16) as v_mfma_f64_16x16x4_f64 tiles.  A wavefront owns up to CV_RT
//      tiles of 16 data rows, loads the H operand once for them, and runs over ALL omega in index order: no sum is split
//      between wavefronts.  Edges are padded with zeros in the operands.  With a rotation m goes to a scratch in device
//      memory: rows x n_data doubles for the call, as large as z beside it, of which a workgroup writes and reads the
//      stretch of 16 x n_data doubles of its tile alone, which stays in the cache (the LDS would cap n_data, registers
//      cannot hand a column to the wavefront that owns another tile row).
//   3. with a rotation: y = T_g m, the same tiles over the n_data sum in index order; tiles of rows >= rank are skipped.
//   4. the epilogue of either product: z = sqrt(w) (y - Gval) for k < rank, 0 behind it.
//   5. score = sum_k z_k^2: one wavefront per row, lane l adds k = l, l + 64, ... by fused multiply-adds, then the butterfly
//      over the lanes.  Entries behind rank are zeros that take part: the order depends on n_data alone.
// No atomics.  A row is one column of every tile: its bits depend on its own H, on K and on T, Gval, w and rank of its group,
// not on the other rows, the other groups, where in a tile it sits or where H lies; they repeat from call to call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_bins.hip.h"

namespace mxe {

constexpr int CV_T = 256;                // threads of a workgroup
constexpr int CV_RT = 4;                 // tiles of 16 data rows a wavefront carries through one sweep

struct CvParams {
    int n, nw, n_groups;     // n_data, n_omega
    const double* K;         // [n][nw]
    const double* H;         // rows of nw values
    const int* row;          // [rows] the row of H a member is, or NULL: its own index
    const int* off;          // [n_groups + 1]
    const int* tile_g;       // [tiles] the group of a tile
    const int* tile_r0;      // [tiles] its first row
    const double* T;         // [n_groups][n][n] or NULL
    const int* rank;         // [n_groups] (n_data everywhere without T)
    const double* Gval;      // [n_groups][n]
    const double* w;         // [n_groups][n]
    double* kh;              // [rows][n]  K H before the rotation (unused without T)
    double* z;               // [rows][n]
    double* score;           // [rows]
    int* ok;                 // [rows]  1: the row is finite
    int* used;               // [n_groups]
};

// z of entry k of a row: acc is (T) K H there
__device__ __forceinline__ double cv_z(const CvParams& p, int g, int rank, int k, bool okrow, double acc)
{
    if (!okrow) return __builtin_nan("");
    if (k >= rank) return 0.0;
    const size_t i = (size_t)g * p.n + k;
    return sqrt(p.w[i]) * (acc - p.Gval[i]);
}

__global__ __launch_bounds__(CV_T)
void cv_score_kernel(const CvParams p)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    __shared__ int okv[16];
    const int n = p.n, nw = p.nw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, cn = lane & 15;
    const int g = p.tile_g[blockIdx.x], r0 = p.tile_r0[blockIdx.x];
    const int nr = min(16, p.off[g + 1] - r0);           // (>= 1: the host lists no empty tile)
    const int rank = p.rank[g];

    // ---- 1. finite rows ----
    for (int c = wave; c < nr; c += CV_T / 64) {
        const double* h = p.H + (size_t)(p.row ? p.row[r0 + c] : r0 + c) * nw;
        int bad = 0;
        for (int i = lane; i < nw; i += 64) if (!(fabs(h[i]) <= 1.79769313486231570815e308)) bad = 1;
        bad = __ballot(bad) != 0;
        if (lane == 0) { okv[c] = bad ? 0 : 1; p.ok[r0 + c] = bad ? 0 : 1; }
    }
    __syncthreads();

    const int rb = r0 + (cn < nr ? cn : 0);              // the row of this lane's column
    const bool cv = cn < nr;                             // the column is a row of the tile
    const bool sv = cv && okv[cn];                       //   and finite
    const int ct_n = (n + 15) >> 4;                      // tiles of data rows
    const int cg_n = (ct_n + CV_RT - 1) / CV_RT;         // groups of CV_RT of them

    // ---- 2. m = K H ----
    {
        const double* hrow = p.H + (size_t)(p.row ? p.row[rb] : rb) * nw;
        for (int item = wave; item < cg_n; item += CV_T / 64) {
            const int I0 = item * CV_RT;
            d4 acc[CV_RT];
#pragma unroll
            for (int t = 0; t < CV_RT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
            for (int w0 = 0; w0 < nw; w0 += 4) {
                const int w = w0 + kq;
                const bool wv = w < nw;
                const double b = (sv && wv) ? hrow[w] : 0.0;
#pragma unroll
                for (int t = 0; t < CV_RT; ++t)
                    if (I0 + t < ct_n) {
                        const int ra = 16 * (I0 + t) + cn;
                        const double a = (ra < n && wv) ? p.K[(size_t)ra * nw + w] : 0.0;
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int t = 0; t < CV_RT; ++t)
                if (I0 + t < ct_n) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int i = 16 * (I0 + t) + kq + 4 * q;
                        if (i < n && cv) {
                            if (p.T) p.kh[(size_t)rb * n + i] = acc[t][q];
                            else p.z[(size_t)rb * n + i] = cv_z(p, g, rank, i, sv, acc[t][q]);
                        }
                    }
                }
        }
    }
    __syncthreads();                                     // (the products are complete; other wavefronts read them)

    // ---- 3. y = T m, 4. z ----
    if (p.T) {
        const double* Tg = p.T + (size_t)g * n * n;
        for (int item = wave; item < cg_n; item += CV_T / 64) {
            const int K0 = item * CV_RT;
            d4 acc[CV_RT];
#pragma unroll
            for (int t = 0; t < CV_RT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
            if (16 * K0 < rank) {
                for (int j0 = 0; j0 < n; j0 += 4) {
                    const int j = j0 + kq;
                    const bool jv = j < n;
                    const double b = (sv && jv) ? p.kh[(size_t)rb * n + j] : 0.0;
#pragma unroll
                    for (int t = 0; t < CV_RT; ++t)
                        if (16 * (K0 + t) < rank) {
                            const int k = 16 * (K0 + t) + cn;
                            const double a = (k < rank && jv) ? Tg[(size_t)k * n + j] : 0.0;
                            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
                        }
                }
            }
#pragma unroll
            for (int t = 0; t < CV_RT; ++t)
                if (K0 + t < ct_n) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = 16 * (K0 + t) + kq + 4 * q;
                        if (k < n && cv) p.z[(size_t)rb * n + k] = cv_z(p, g, rank, k, sv, acc[t][q]);
                    }
                }
        }
        __syncthreads();
    }

    // ---- 5. score ----
    for (int c = wave; c < nr; c += CV_T / 64) {
        const double* zr = p.z + (size_t)(r0 + c) * n;
        double s = 0.0;
        for (int k = lane; k < n; k += 64) s = fma(zr[k], zr[k], s);
        s = bins_wave_sum(s);
        if (lane == 0) p.score[r0 + c] = okv[c] ? s : __builtin_nan("");
    }
}

// the finite rows of every group: one thread per group (an empty group has no tile above and counts 0 here)
__global__ __launch_bounds__(256)
void cv_used_kernel(const CvParams p)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= p.n_groups) return;
    int nu = 0;
    for (int r = p.off[g]; r < p.off[g + 1]; ++r) nu += p.ok[r];
    p.used[g] = nu;
}

} // namespace mxe
