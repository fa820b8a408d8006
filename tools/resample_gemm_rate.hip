// bins_resample_kernel (v_mfma_f64_16x16x4_f64 tiles, mxe_resample.hip.h) against a plain-FMA kernel of the same two
// products, at the size of a resampling job: n_sets sets of n_bins x n_data bins, n_res resamples.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/resample_gemm_rate.hip -o tools/resample_gemm_rate
//   tools/resample_gemm_rate [n_sets 256] [n_bins 1024] [n_data 200] [n_res 17]
// Prints the device time of each (median of 5 after a warm-up) and the largest difference of their out_dev.
#include "../maxent_amd/csrc/mxe_resample.hip.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

// the same arithmetic per output -- one thread per (resample, column), every sum serially in index order -- without tiles
__global__ __launch_bounds__(mxe::BINS_T)
void plain_resample_kernel(const mxe::ResampleParams p)
{
    using namespace mxe;
    const int set = blockIdx.x, m = p.m, n = p.n, n_res = p.n_res, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* bins = p.bins + (size_t)set * m * n;
    const double* T = p.T + (size_t)set * n * n;
    const int rank = p.rank[set];
    double* D = p.D + (size_t)set * n_res * n;
    __shared__ double meanv[BINS_NMAX];
    __shared__ double tmean[BINS_NMAX];
    bins_mean(bins, m, n, p.part + (size_t)set * BINS_NWAVE * n * 2, meanv, p.out_mean + (size_t)set * n);
    for (int idx = tid; idx < n_res * n; idx += BINS_T) {
        const int r = idx / n, j = idx - r * n;
        double s = 0.0;
        for (int b = 0; b < m; ++b) s = fma((double)p.counts[(size_t)r * m + b], bins[(size_t)b * n + j] - meanv[j], s);
        D[idx] = s / p.Nr[r];
    }
    for (int k = wave; k < n; k += BINS_NWAVE) {
        double s = 0.0;
        if (k < rank) for (int j = lane; j < n; j += 64) s = fma(T[(size_t)k * n + j], meanv[j], s);
        s = bins_wave_sum(s);
        if (lane == 0) tmean[k] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < n_res * n; idx += BINS_T) {
        const int r = idx / n, k = idx - r * n;
        double s = 0.0;
        if (k < rank) for (int j = 0; j < n; ++j) s = fma(T[(size_t)k * n + j], D[(size_t)r * n + j], s);
        p.out_dev[(size_t)set * n_res * n + idx] = s;
        p.out_G[(size_t)set * n_res * n + idx] = (k < rank) ? tmean[k] + s : 0.0;
    }
}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv)
{
    const int ns = argc > 1 ? atoi(argv[1]) : 256, m = argc > 2 ? atoi(argv[2]) : 1024, n = argc > 3 ? atoi(argv[3]) : 200,
              nr = argc > 4 ? atoi(argv[4]) : 17;
    if (ns < 1 || m < 2 || n < 1 || n > mxe::BINS_NMAX || nr < 1) { printf("bad sizes\n"); return 1; }
    std::vector<double> bins((size_t)ns * m * n), T((size_t)ns * n * n, 0.0), Nr(nr);
    std::vector<int> counts((size_t)nr * m, 1), rank(ns, n);
    srand(7);
    for (auto& x : bins) x = 1.0 + 1e-3 * (rand() / (double)RAND_MAX - 0.5);
    for (int s = 0; s < ns; ++s) for (int k = 0; k < n; ++k) {          // a banded T (any finite matrix times the same)
        T[((size_t)s * n + k) * n + k] = 0.8; T[((size_t)s * n + k) * n + (k + 1) % n] = 0.6;
    }
    const int block = std::max(1, m / std::max(nr - 1, 1));
    for (int r = 1; r < nr; ++r) for (int b = (r - 1) * block; b < std::min(r * block, m); ++b) counts[(size_t)r * m + b] = 0;
    for (int r = 0; r < nr; ++r) { long long s = 0; for (int b = 0; b < m; ++b) s += counts[(size_t)r * m + b]; Nr[r] = (double)s; }
    mxe::ResampleParams p;
    p.m = m; p.n = n; p.n_res = nr;
    double *dbins, *dNr, *dT, *dev2; int *dcounts, *drank;
    CHK(hipMalloc(&dbins, bins.size() * 8)); CHK(hipMalloc(&dNr, nr * 8)); CHK(hipMalloc(&dT, T.size() * 8));
    CHK(hipMalloc(&dcounts, counts.size() * 4)); CHK(hipMalloc(&drank, ns * 4));
    CHK(hipMalloc(&p.part, (size_t)ns * mxe::BINS_NWAVE * n * 2 * 8)); CHK(hipMalloc(&p.D, (size_t)ns * nr * n * 8));
    CHK(hipMalloc(&p.out_mean, (size_t)ns * n * 8)); CHK(hipMalloc(&p.out_G, (size_t)ns * nr * n * 8));
    CHK(hipMalloc(&p.out_dev, (size_t)ns * nr * n * 8)); CHK(hipMalloc(&dev2, (size_t)ns * nr * n * 8));
    CHK(hipMemcpy(dbins, bins.data(), bins.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dNr, Nr.data(), nr * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dT, T.data(), T.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dcounts, counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
    CHK(hipMemcpy(drank, rank.data(), ns * 4, hipMemcpyHostToDevice));
    p.bins = dbins; p.counts = dcounts; p.Nr = dNr; p.T = dT; p.rank = drank;
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    double med[2];
    std::vector<double> out[2];
    for (int which = 0; which < 2; ++which) {
        std::vector<float> ms;
        for (int it = 0; it < 6; ++it) {
            CHK(hipEventRecord(e0, 0));
            if (which == 0) hipLaunchKernelGGL(mxe::bins_resample_kernel, dim3(ns), dim3(mxe::BINS_T), 0, 0, p);
            else hipLaunchKernelGGL(plain_resample_kernel, dim3(ns), dim3(mxe::BINS_T), 0, 0, p);
            CHK(hipGetLastError());
            CHK(hipEventRecord(e1, 0));
            CHK(hipEventSynchronize(e1));
            float t; CHK(hipEventElapsedTime(&t, e0, e1));
            if (it) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        med[which] = ms[ms.size() / 2];
        out[which].resize((size_t)ns * nr * n);
        CHK(hipMemcpy(out[which].data(), p.out_dev, out[which].size() * 8, hipMemcpyDeviceToHost));
    }
    double worst = 0.0, big = 0.0;
    for (size_t i = 0; i < out[0].size(); ++i) { worst = std::max(worst, std::fabs(out[0][i] - out[1][i])); big = std::max(big, std::fabs(out[1][i])); }
    printf("{\"n_sets\": %d, \"n_bins\": %d, \"n_data\": %d, \"n_res\": %d, \"mfma_ms\": %.4f, \"plain_fma_ms\": %.4f, \"max_abs_diff\": %.3e, \"max_abs_dev\": %.3e}\n",
           ns, m, n, nr, med[0], med[1], worst, big);
    return 0;
}
