// mxe_postsample.hip.h -- draws of the hidden image from the Gaussian posterior around the minimiser
//
//   nothing of the reference (it offers no error bars, and no samples)   -> postsample_kernel   (mxe_posterior_sample)
//                                                                           normals_kernel      (mxe_normals)
//
// mxe_posterior_var integrates the posterior covariance Gamma over linear functionals; error bars of what is not linear
// in A (a peak position, a gap edge, Sigma(omega)) need draws from N(0, Gamma).  In the notation of mxe_postvar.hip.h
// (w, V', c, a = alpha~ / eta, B = c W c + a I = L L^T):
//
//   Gamma = (eta K^T Sigma^-1 K + alpha~ diag(1/w))^-1 = (1 / alpha~) [ diag(w) - diag(w) V' c B^-1 c V'^T diag(w) ]
//
// and with z1 (n_omega) and z2 (n_s) independent standard normals
//
//   q_i     = sqrt(a w_i) z1_i + w_i V'_i . (c o z2)         (q = w o r, cov r = a diag(1/w) + V' c^2 V'^T; no division by w)
//   y       = c o V'^T q
//   x       = L^-T L^-1 y                                      (B^-1 is never formed)
//   delta_i = (1/a) [ q_i - w_i V'_i . (c o x) ] / sqrt(eta)
//
// has cov delta = Gamma exactly; a row with w_i = 0 gives delta_i = 0.  Like the variance, delta_i is a difference of two
// terms and is formed as written.
//
// One workgroup (4 waves) per problem:
//   1. w, W, B and the Cholesky factor in LDS: factor_B (mxe_factor.hip.h), shared with logdet_kernel and postvar_kernel;
//   2. the samples in blocks of 16; the block of right-hand sides lives where postvar_kernel keeps its Y block (pv_y).
//      Three sweeps over the omega rows of V' by v_mfma_f64_16x16x4_f64, a tile of 16 samples x 16 omega points each:
//        a. c o z2 into the block; q (block_times_Vt), written to the output rows themselves as scratch (a tile row belongs to one wave);
//        b. y = c o V'^T q: the omega rows go to the four waves round-robin in groups of 4, the waves' partial tiles
//           are added in wave order;
//        c. after the blocked forward substitution of postvar_kernel and a blocked backward substitution with L^T,
//           c o x in the block; delta (block_times_Vt again) overwrites q (every lane reads back what it wrote itself in sweep a).
// The normals are read from device memory ([P][n_samples][n_omega + n_s]): handed in by the caller, or filled before the
// launch by normals_kernel with the generator below, so both ways run the same code on the same numbers.
//
// Bits do not depend on the batch, on n_samples or on the sample's block: a tile's k-sum runs inside one MFMA chain, the
// sums over omega are added in wave order, every other sum runs in index order in one thread; a sample's column of a
// tile never meets another sample's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_postvar.hip.h"

namespace mxe {

// ---- Philox4x32-10 (Salmon et al. 2011, the Random123 constants) and Box-Muller ------------------------------------
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the pair (z_2j, z_2j+1) of sample s of the stream: counter (j, s, stream), key seed
__device__ inline void normal_pair(uint64_t seed, uint64_t stream, uint32_t s, uint32_t j, double& za, double& zb)
{
    uint32_t x[4];
    philox4x32_10(j, s, (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), x);
    const double u1 = ((double)((((uint64_t)x[0] << 32) | x[1]) >> 11) + 0.5) * 0x1p-53;
    const double u2 = ((double)((((uint64_t)x[2] << 32) | x[3]) >> 11) + 0.5) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
    za = r * cos(t);
    zb = r * sin(t);
}

// out[(p * n_samples + s) * n + .] for the stream of problem p (stream0 for every p when stream is NULL); one thread per pair
__global__ __launch_bounds__(256)
void normals_kernel(uint64_t seed, const uint64_t* stream, uint64_t stream0, int P, int n_samples, int n, double* out)
{
    const int npair = (n + 1) >> 1;
    const size_t per = (size_t)n_samples * npair;
    for (size_t p = blockIdx.y; p < (size_t)P; p += gridDim.y)
        for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < per; idx += (size_t)gridDim.x * 256) {
            const uint32_t s = (uint32_t)(idx / npair), j = (uint32_t)(idx % npair);
            double za, zb;
            normal_pair(seed, stream ? stream[p] : stream0, s, j, za, zb);
            double* o = out + (p * n_samples + s) * (size_t)n;
            o[2 * j] = za;
            if (2 * (int)j + 1 < n) o[2 * j + 1] = zb;
        }
}

struct PostSampleParams : FactorParams {
    const double* z;            // [P][n_samples][nw + ns]
    double* out;                // [P][n_samples][nw]
    double scale;               // 1 / sqrt(eta)
    int n_samples;
};

template <int NT>
__global__ __launch_bounds__(256)
void postsample_kernel(PostSampleParams p)
{
    constexpr int NP = 16 * NT;
    extern __shared__ double sm[];
    double* Bm = sm;                     // [NP][NP + 1]
    double* wsh = Bm + NP * (NP + 1);    // [nwp]
    double* fsh = wsh + p.nwp + 256;     // [16] unused | [16] flag (the places of postvar_kernel)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.nw, ns = p.ns, n_samples = p.n_samples;
    const size_t prob = blockIdx.x;
    const FactorProblem fp = resolve_problem<NP>(p, prob);
    const double* V = fp.V;
    const double* cc = fp.cc;
    const double a = fp.a;
    const bool ok = factor_B<NT>(fp, nw, p.nwp, ns, Bm, wsh, fsh + 16);
    const int kq = lane >> 4, cn = lane & 15;
    const int n_groups = (nw + 3) >> 2;          // (the rows of V' behind n_omega are zero)
    const int ntile = (ns + 15) >> 4;
    double* out = p.out + prob * (size_t)n_samples * nw;
    if (!ok) {                                       // (uniform)
        const double nan = __builtin_nan("");
        for (size_t i = tid; i < (size_t)n_samples * nw; i += 256) out[i] = nan;
        return;
    }

    // ---- the samples, 16 at a time -------------------------------------------------------------------------
    const int nz = nw + ns;
    const double* zp = p.z + prob * (size_t)n_samples * nz;
    const int n_wtiles = (nw + 15) >> 4;
    const int kgroups = 4 * ntile;                   // groups of 4 singular directions (columns behind n_s: zero)
    const double inv_a = 1.0 / a;
    for (int s0 = 0; s0 < n_samples; s0 += 16) {
        // a. c o z2 of the block (zero behind n_s and behind the last sample), then q
        for (int idx = tid; idx < NP * 16; idx += 256) {
            const int k = idx % NP, j = idx / NP;    // (k fastest: neighbouring lanes read neighbouring normals)
            Bm[pv_y<NP>(k, j)] = (k < ns && s0 + j < n_samples) ? cc[k] * zp[(size_t)(s0 + j) * nz + nw + k] : 0.0;
        }
        __syncthreads();
        for (int T = wave; T < n_wtiles; T += 4) {
            const int i = 16 * T + cn;               // this lane's omega point; its samples are s0 + kq + 4 r
            const bool iv = i < nw;
            const d4 acc = block_times_Vt<NP>(Bm, V, i, iv, kgroups, kq, cn);
            if (iv) {
                const double w = wsh[i], sw = sqrt(a * w);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = s0 + kq + 4 * r;
                    if (s < n_samples) out[(size_t)s * nw + i] = fma(sw, zp[(size_t)s * nz + i], w * acc[r]);
                }
            }
        }
        __syncthreads();                             // (q is read by other waves than wrote it; the block is free again)
        // b. y = c o V'^T q
        for (int idx = tid; idx < NP * 16; idx += 256) Bm[pv_y<NP>(idx >> 4, idx & 15)] = 0.0;
        {
            const int s = s0 + cn;
            const bool sv = s < n_samples;
            const double* qrow = out + (size_t)(sv ? s : 0) * nw;
            d4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
            for (int g = wave; g < n_groups; g += 4) {
                const int i = 4 * g + kq;
                const double b = (sv && i < nw) ? qrow[i] : 0.0;
                const double* row = V + (size_t)i * NP + cn;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * t], b, acc[t], 0, 0, 0);
            }
            __syncthreads();
            add_tiles_in_wave_order<NT>(Bm, acc, 0, ntile, wave, [=](int t, int r) { return pv_y<NP>(16 * t + kq + 4 * r, cn); });
        }
        for (int idx = tid; idx < ntile * 256; idx += 256) {         // (rows behind n_s stay zero whatever V' holds there)
            const int k = idx >> 4;
            Bm[pv_y<NP>(k, idx & 15)] = k < ns ? Bm[pv_y<NP>(k, idx & 15)] * cc[k] : 0.0;
        }
        __syncthreads();
        pv_forward_solve<NP>(Bm, ns, tid);
        ps_backward_solve<NP>(Bm, ns, tid);
        for (int idx = tid; idx < ns * 16; idx += 256) Bm[pv_y<NP>(idx >> 4, idx & 15)] *= cc[idx >> 4];
        __syncthreads();
        // c. delta over q
        for (int T = wave; T < n_wtiles; T += 4) {
            const int i = 16 * T + cn;
            const bool iv = i < nw;
            const d4 acc = block_times_Vt<NP>(Bm, V, i, iv, kgroups, kq, cn);
            if (iv) {
                const double w = wsh[i];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = s0 + kq + 4 * r;
                    if (s < n_samples) {
                        double* o = out + (size_t)s * nw + i;
                        *o = (inv_a * fma(-w, acc[r], *o)) * p.scale;
                    }
                }
            }
        }
        __syncthreads();
    }
}

} // namespace mxe
