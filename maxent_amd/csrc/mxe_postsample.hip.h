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
//   1. w, W, B and the Cholesky factor in LDS: the steps of postvar_kernel, operation for operation (repeated, not shared:
//      that kernel's code and time stay as they are);
//   2. the samples in blocks of 16; the block of right-hand sides lives where postvar_kernel keeps its Y block (pv_y).
//      Three sweeps over the omega rows of V' by v_mfma_f64_16x16x4_f64, a tile of 16 samples x 16 omega points each:
//        a. c o z2 into the block; q, written to the output rows themselves as scratch (a tile row belongs to one wave);
//        b. y = c o V'^T q: the omega rows go to the four waves round-robin in groups of 4, the waves' partial tiles
//           are added in wave order;
//        c. after the blocked forward substitution of postvar_kernel and a blocked backward substitution with L^T,
//           c o x in the block; delta overwrites q (every lane reads back what it wrote itself in sweep a).
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

struct PostSampleParams {
    const double* V;            // [n_ds][nwp][NP]
    const double* c;            // [n_ds][NP]
    const int* elem_ds;         // [n_elem]
    const int* elem_kind;       // [n_elem]
    const double* D;            // [n_elem][nwp]
    const int* elem;            // [P] element of a problem
    const double* alpha;        // [P] alpha~ / eta
    const double* H;            // rows of n_omega values
    const int* row;             // [P] row of H that belongs to a problem, or NULL: row p
    const double* z;            // [P][n_samples][nw + ns]
    double* out;                // [P][n_samples][nw]
    double scale;               // 1 / sqrt(eta)
    int nw, nwp, ns, n_samples;
};

inline size_t postsample_lds_bytes(int NP, int nwp) { return postvar_lds_bytes(NP, nwp); }

// L^T X = Z for the block of 16 right-hand sides (pv_y), in place
template <int NP>
__device__ inline void ps_backward_solve(double* Bm, int ns, int tid)
{
    constexpr int LD = NP + 1;
    const int ntile = (ns + 15) >> 4;
    for (int J = ntile - 1; J >= 0; --J) {
        const int k0 = 16 * J, k1 = min(k0 + 16, ns);
        if (tid < 16) {
            for (int k = k1 - 1; k >= k0; --k) {
                double s = Bm[pv_y<NP>(k, tid)];
                for (int m = k1 - 1; m > k; --m) s = fma(-Bm[m * LD + k], Bm[pv_y<NP>(m, tid)], s);
                s /= Bm[k * LD + k];
                Bm[pv_y<NP>(k, tid)] = s;
            }
        }
        __syncthreads();
        const int nb = k1 - k0;                      // (the last tile row, the first one here, may be short)
        for (int idx = tid; idx < k0 * 16; idx += 256) {
            const int m = idx >> 4, j = idx & 15;
            double s = Bm[pv_y<NP>(m, j)];
            for (int kk = nb - 1; kk >= 0; --kk) s = fma(-Bm[(k0 + kk) * LD + m], Bm[pv_y<NP>(k0 + kk, j)], s);
            Bm[pv_y<NP>(m, j)] = s;
        }
        __syncthreads();
    }
}

template <int NT>
__global__ __launch_bounds__(256)
void postsample_kernel(PostSampleParams p)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    constexpr int NP = 16 * NT, LD = NP + 1;
    extern __shared__ double sm[];
    double* Bm = sm;                     // [NP][LD]
    double* wsh = Bm + NP * LD;          // [nwp]
    double* fsh = wsh + p.nwp + 256;     // [16] unused | [16] flag (the places of postvar_kernel)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.nw, nwp = p.nwp, ns = p.ns, n_samples = p.n_samples;
    const size_t prob = blockIdx.x;
    const int e = p.elem[prob];
    const int ds = p.elem_ds[e], kind = p.elem_kind[e];
    const double a = p.alpha[prob];
    const double* V = p.V + (size_t)ds * nwp * NP;
    const double* cc = p.c + (size_t)ds * NP;
    const double* Hp = p.H + (size_t)(p.row ? p.row[prob] : (int)prob) * nw;
    const double* Dp = p.D + (size_t)e * nwp;
    if (tid == 0) fsh[16] = 0.0;
    __syncthreads();
    bool finite = true;
    for (int i = tid; i < nwp; i += 256) {
        double w = 0.0;
        if (i < nw) {
            const double h = Hp[i];
            if (kind == 0) w = h;
            else { const double d2 = 2.0 * Dp[i]; w = sqrt(fma(h, h, d2 * d2)); }
            if (!(fabs(w) <= 1.79769313486231570815e308)) finite = false;
        }
        wsh[i] = w;
    }
    if (!finite) fsh[16] = 1.0;          // (every writer writes the same value)
    for (int i = tid; i < NP * LD; i += 256) Bm[i] = 0.0;
    __syncthreads();
    bool ok = fsh[16] == 0.0;
    const int kq = lane >> 4, cn = lane & 15;
    const int n_groups = (nw + 3) >> 2;          // (the rows of V' behind n_omega are zero)
    const int ntile = (ns + 15) >> 4;
    if (ok) {
        for (int mt = 0; mt < ntile; ++mt) {
            d4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
            for (int g = wave; g < n_groups; g += 4) {
                const double* row = V + (size_t)(4 * g + kq) * NP + cn;
                const double wq = wsh[4 * g + kq];
                const double am = row[16 * mt] * wq;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t >= mt && t < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, row[16 * t], acc[t], 0, 0, 0);
            }
            for (int ph = 0; ph < 4; ++ph) {         // the four waves add their partial tiles one after the other
                if (wave == ph) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t >= mt && t < ntile) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) Bm[(16 * mt + kq + 4 * r) * LD + 16 * t + cn] += acc[t][r];
                        }
                }
                __syncthreads();
            }
        }
        for (int idx = tid; idx < ns * ns; idx += 256) {
            const int i = idx / ns, j = idx % ns;
            if (i <= j) {
                double b = cc[i] * Bm[i * LD + j] * cc[j];
                if (i == j) b += a;
                Bm[j * LD + i] = b;
            }
        }
        __syncthreads();
        for (int j = 0; j < ns; ++j) {               // right-looking Cholesky on the lower triangle
            const double piv = Bm[j * LD + j];
            if (!(piv > 0.0) || !(piv <= 1.79769313486231570815e308)) ok = false;
            const double d = sqrt(piv);
            __syncthreads();
            for (int i = j + 1 + tid; i < ns; i += 256) Bm[i * LD + j] /= d;
            if (tid == 0) Bm[j * LD + j] = d;
            __syncthreads();
            const int m = ns - j - 1;
            for (int idx = tid; idx < m * m; idx += 256) {
                const int i = j + 1 + idx / m, k = j + 1 + idx % m;
                if (k <= i) Bm[i * LD + k] = fma(-Bm[i * LD + j], Bm[k * LD + j], Bm[i * LD + k]);
            }
            __syncthreads();
        }
    }
    double* out = p.out + prob * (size_t)n_samples * nw;
    if (!ok) {                                       // (uniform: every thread saw the same pivots and the same flag)
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
            const double* vrow = V + (size_t)(iv ? i : 0) * NP + kq;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int g = 0; g < kgroups; ++g)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Bm[pv_y<NP>(4 * g + kq, cn)], iv ? vrow[4 * g] : 0.0, acc, 0, 0, 0);
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
            for (int ph = 0; ph < 4; ++ph) {
                if (wave == ph) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < ntile) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) Bm[pv_y<NP>(16 * t + kq + 4 * r, cn)] += acc[t][r];
                        }
                }
                __syncthreads();
            }
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
            const double* vrow = V + (size_t)(iv ? i : 0) * NP + kq;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int g = 0; g < kgroups; ++g)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Bm[pv_y<NP>(4 * g + kq, cn)], iv ? vrow[4 * g] : 0.0, acc, 0, 0, 0);
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
