// mxe_fullmatrix_postvar.hip.h -- posterior (Gaussian) variances of the whole-matrix continuation (nothing of the reference:
// it has neither the solver nor error bars).  DESIGN 4za; the matrix analogue of postvar_kernel (mxe_postvar.hip.h).
//
//   u of one (data set, alpha) pair  ->  value, variance and prior variance of linear functionals x = sum_i Tr(F_i H_i),
//   and of every coordinate h_p,i                                                            fullmatrix_postvar_kernel<M, C>
//
// In the coordinates h_p,i = Tr(E_p H_i) of mxe_fullmatrix.hip.h the matrix entropy has d2S/dh dh = -L^-1 with L_i (P x P) the
// Frechet derivative the solver forms for its Gram products, so the covariance of h around the minimiser of
// Q = chi2 / 2 - alpha S is
//   Gamma   = (alpha L^-1 + (V' c^2 V'^T) (x) 1_P)^-1 = (1 / alpha) [ L - L V' c B^-1 c V'^T L ]
//   B       = alpha I_d + c W c,   W_(p,s),(q,t) = sum_i V'_is L_i,pq V'_it,   d = P n_s,   B = L_B L_B^T
//   var(x)  = (1 / alpha) [ sum_i f_i^T L_i f_i - |L_B^-1 y|^2 ],   y_(p,s) = c_s sum_i V'_is (L_i f_i)_p,   f_p,i = Tr(E_p F_i)
//   var(h_p,i) = (1 / alpha) [ L_i,pp - |L_B^-1 y|^2 ],             y_(q,s) = c_s V'_is L_i,qp
// Both are differences of two sums of non-negative terms, formed as written; B^-1 is never formed.  A difference that rounding
// makes negative is returned as 0 by a comparison: a NaN stays a NaN.  For M = 1 this is postvar_kernel with w = H.
//
// One workgroup of 256 threads per job; the jobs are independent.  The parts (1 to 3 are fmpv_factor, which
// fullmatrix_logdet_kernel of mxe_fullmatrix_logdet.hip.h calls too):
//   1. the evaluation at u of fullmatrix_kernel (a copy of its code: the solver's instantiations are not touched): Gamma
//      coordinates, the Jacobi in registers, W_i, D phi, the H coordinates;
//   2. L, then the P (P + 1) / 2 Gram products on v_mfma_f64_16x16x4_f64 as in the solver; the epilogue writes
//      B = alpha I + c W c to device memory;
//   3. Cholesky of B, right-looking in blocks of 16 columns, the panel in the LDS (the lower triangle alone is read and
//      written); a pivot that is not positive and finite ends the job;
//   4. the functionals in blocks of 16: g = L_i f_i per omega (thread per (q, i, functional)), Y = c o V'^T g as one MFMA
//      chain over the omega rows per (q, tile row of V'), the sums x = sum f h and sum f g (16 threads per functional over
//      interleaved terms, added in order), the blocked forward substitution L_B Z = Y with Y in the LDS -- the rows of a block
//      of 16 first take the part of the rows above it, a thread per (row, functional), then one thread per functional solves
//      the 16 x 16 diagonal block -- and |z|^2;
//   5. (want_diag) the same substitution on blocks of 16 columns y^(i,p), in the order of p n_omega + i.
// No atomics; every sum has one order that depends on the sizes alone, and a column of a block of 16 does not see its
// neighbours: the bits of a job do not depend on the batch, on n_f or on a functional's place in F.
// A job whose u or H is not finite or whose B is not positive definite writes NaN to all its outputs.
// Workgroup b takes the jobs b, b + gridDim.x, ... and works in slice b of the scratch (fmpv_scratch_doubles each): the entry
// point chooses the number of slices so that the scratch stays below a cap; results do not depend on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_fullmatrix.hip.h"

namespace mxe {

constexpr int FMPV_NF = 16;               // functionals (or coordinate columns) of one substitution

struct FullMatrixPostVarParams {
    int n_job, n_omega, n_s, n_f, want_diag;
    const double* V;         // [n_omega][n_s]
    const double* c;         // [n_s]
    const double* D;         // [n_omega]
    const double* alpha;     // [n_job]
    const double* u;         // [n_job][P][n_s]
    const double* F;         // [n_f][P][n_omega] (NULL with n_f == 0)
    double* scratch;         // [gridDim.x][fmpv_scratch_doubles]
    double* out_value;       // [n_job][n_f]
    double* out_var;         // [n_job][n_f]
    double* out_prior;       // [n_job][n_f]
    double* out_diag;        // [n_job][P][n_omega]   (want_diag)
    double* out_dprior;      // [n_job][P][n_omega]   (want_diag)
    double* out_h;           // [n_job][P][n_omega]   (want_diag)
};

__host__ __device__ inline size_t fmpv_scratch_doubles(int m, bool cplx, int nw, int ns)
{
    const size_t P = fm_P(m, cplx), d = P * ns, npair = P * (P + 1) / 2, mm = (size_t)m * m;
    // Gamma coordinates, H coordinates | W_i | D phi | L | L f of a block of functionals | B
    return 2 * P * nw + (cplx ? 2 : 1) * mm * nw + mm * nw + npair * nw + FMPV_NF * P * nw + d * d;
}
// doubles of dynamic LDS: the panel of the Cholesky, then a block of right-hand sides [d][FM_LDP] | partial sums [2][256] |
// sums [32] | flags
__host__ __device__ inline size_t fmpv_lds_doubles(int d)
{
    return (size_t)d * FM_LDP + 2 * FM_T + 32 + 8;
}

// the place of L_pq (any order of p, q) among the P (P + 1) / 2 pairs p <= q
__device__ inline int fmpv_pair(int a, int b, int P)
{
    const int lo = min(a, b), hi = max(a, b);
    return lo * P - lo * (lo - 1) / 2 + (hi - lo);
}

// L_B Z = Y for the 16 columns of Y [d][FM_LDP] in the LDS (overwritten by Z), L_B the lower triangle of Bm [d][d]; returns
// |z_j|^2 to the threads j < 16.  Called by all threads.  r_begin, a multiple of 16: the rows of Y above it are zero (and are
// not read); the substitution and the sums start there.
__device__ inline double fmpv_forward(const double* Bm, int d, double* Ysh, double* part, int tid, int r_begin = 0)
{
    const int rr = tid >> 4, j = tid & 15;
    for (int r0 = r_begin; r0 < d; r0 += 16) {
        const int row = r0 + rr, r1 = min(d, r0 + 16);
        if (row < d && r0 > r_begin) {
            const double* Lr = Bm + (size_t)row * d;
            double s = 0.0;
            for (int k = r_begin; k < r0; ++k) s = fma(Lr[k], Ysh[k * FM_LDP + j], s);
            Ysh[row * FM_LDP + j] -= s;
        }
        __syncthreads();
        if (tid < 16) {
            for (int r = r0; r < r1; ++r) {
                const double* Lr = Bm + (size_t)r * d;
                double s = Ysh[r * FM_LDP + tid];
                for (int k = r0; k < r; ++k) s = fma(-Lr[k], Ysh[k * FM_LDP + tid], s);
                Ysh[r * FM_LDP + tid] = s / Lr[r];
            }
        }
        __syncthreads();
    }
    double s = 0.0;
    for (int r = r_begin + rr; r < d; r += 16) { const double z = Ysh[r * FM_LDP + j]; s = fma(z, z, s); }
    part[rr * 16 + j] = s;
    __syncthreads();
    double q = 0.0;
    if (tid < 16)
        for (int pt = 0; pt < 16; ++pt) q += part[pt * 16 + tid];
    __syncthreads();
    return q;
}

// Parts 1 to 3 of a job, shared by fullmatrix_postvar_kernel and fullmatrix_logdet_kernel (mxe_fullmatrix_logdet.hip.h): the
// evaluation at u, L, B = alpha I + c W c and its Cholesky factor, which is left in the lower triangle of Bm [d][d].  The
// arrays are the caller's slice of the scratch: gam, hc [P][nw] (Gamma and H coordinates), Wv [nw][WPL][M][M], phiD
// [nw][M][M], Lp [NPAIR][nw]; Ysh [d][FM_LDP] is the panel in the LDS; flag: [0] the job is bad, [1] B is positive definite
// so far.  Called by all threads; returns (the same in every thread) whether u and H are finite and every pivot is positive
// and finite.  What is left in hc, Lp and Bm is valid only then.
template <int M, bool C>
__device__ __forceinline__ bool fmpv_factor(const double* V, const double* cc, const double* Dm, const double* u,
                                            const double alpha, const int nw, const int ns, double* gam, double* hc, double* Wv,
                                            double* phiD, double* Lp, double* Bm, double* Ysh, int* flag)
{
    constexpr int P = C ? M * M : M * (M + 1) / 2, NPAIR = P * (P + 1) / 2, MM = M * M, WPL = C ? 2 : 1;
    constexpr double R2 = 1.41421356237309504880;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int d = P * ns, npw = P * nw;
    const int kq = lane >> 4, cn = lane & 15;
    const int ntile = (ns + 15) >> 4, n_groups = (nw + 3) >> 2;
    // ================= 1. evaluation at u (fullmatrix_kernel, part 1) =================
    if (tid == 0) { flag[0] = 0; flag[1] = 1; }
    bool bad = false;
    for (int k = tid; k < d; k += FM_T) bad |= !isfinite(u[k]);
    for (int idx = tid; idx < npw; idx += FM_T) {
        const int pp = idx / nw, i = idx - pp * nw;
        const double* vr = V + (size_t)i * ns;
        const double* xr = u + pp * ns;
        double s = 0.0;
        for (int k = 0; k < ns; ++k) s = fma(vr[k], xr[k], s);
        gam[idx] = s;
    }
    __syncthreads();
    for (int i = tid; i < nw; i += FM_T) {
        double ar[M][M], ai[M][M], wr[M][M], wi[M][M];
        {
            int pp = M;
#pragma unroll
            for (int a = 0; a < M; ++a) { ar[a][a] = gam[a * nw + i]; ai[a][a] = 0.0; }
#pragma unroll
            for (int a = 0; a < M; ++a)
#pragma unroll
                for (int b = a + 1; b < M; ++b) {
                    const double re = gam[pp * nw + i] / R2;
                    const double im = C ? gam[(pp + M * (M - 1) / 2) * nw + i] / R2 : 0.0;
                    ar[a][b] = re; ar[b][a] = re; ai[a][b] = im; ai[b][a] = -im;
                    ++pp;
                }
        }
        fm_jacobi<M, C>(ar, ai, wr, wi);
        const double Di = Dm[i];
        double gk[M], eh[M];
#pragma unroll
        for (int k = 0; k < M; ++k) {
            gk[k] = ar[k][k];
            eh[k] = exp(0.5 * gk[k]);
        }
        // H = D B B^H, B_ak = W_ak e^(gamma_k / 2): the upper triangle
        {
            int pp = M;
#pragma unroll
            for (int a = 0; a < M; ++a)
#pragma unroll
                for (int b = a; b < M; ++b) {
                    double sr = 0.0, si = 0.0;
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        const double xr_ = wr[a][k] * eh[k], yr_ = wr[b][k] * eh[k];
                        if (C) {
                            const double xi_ = wi[a][k] * eh[k], yi_ = wi[b][k] * eh[k];
                            sr += xr_ * yr_ + xi_ * yi_;
                            si += xi_ * yr_ - xr_ * yi_;
                        } else {
                            sr += xr_ * yr_;
                        }
                    }
                    sr *= Di; si *= Di;
                    bad |= !isfinite(sr) || !isfinite(si);
                    if (a == b) {
                        hc[a * nw + i] = sr;
                    } else {
                        hc[pp * nw + i] = R2 * sr;
                        if (C) hc[(pp + M * (M - 1) / 2) * nw + i] = R2 * si;
                        ++pp;
                    }
                }
        }
        double* wo = Wv + (size_t)i * WPL * MM;
        double* po = phiD + (size_t)i * MM;
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
            for (int k = 0; k < M; ++k) {
                wo[a * M + k] = wr[a][k];
                if (C) wo[MM + a * M + k] = wi[a][k];
                const double ph = Di * fm_phi(gk[a], gk[k]);
                bad |= !isfinite(ph);
                po[a * M + k] = ph;
            }
    }
    if (bad) flag[0] = 1;
    __syncthreads();
    bool job_ok = flag[0] == 0;                  // (the same in every thread)

    if (job_ok) {
        // ================= 2. L and B = alpha I + c W c (fullmatrix_kernel, part 2) =================
        for (int idx = tid; idx < NPAIR * nw; idx += FM_T) {
            const int pair = idx / nw, i = idx - pair * nw;
            int pp = 0, rem = pair;
            while (rem >= P - pp) { rem -= P - pp; ++pp; }
            const int qq = pp + rem;
            int k1, a1, b1, k2, a2, b2;
            fm_basis(pp, M, k1, a1, b1);
            fm_basis(qq, M, k2, a2, b2);
            const double* Wr = Wv + (size_t)i * WPL * MM;
            const double* Wi = Wr + (C ? MM : 0);
            const double* ph = phiD + (size_t)i * MM;
            double s = 0.0;
            for (int k = 0; k < M; ++k)
                for (int l = 0; l < M; ++l) {
                    double xr, xi, yr, yi;
                    fm_xkl<M, C>(k1, a1, b1, Wr, Wi, k, l, xr, xi);
                    fm_xkl<M, C>(k2, a2, b2, Wr, Wi, k, l, yr, yi);
                    s = fma(ph[k * M + l], xr * yr + xi * yi, s);
                }
            Lp[idx] = s;
        }
        __syncthreads();
        const int ntp = ntile * (ntile + 1) / 2;
        for (int item = wave; item < NPAIR * ntp; item += 4) {
            const int pair = item / ntp;
            int ti = 0, rem = item - pair * ntp;
            while (rem >= ntile - ti) { rem -= ntile - ti; ++ti; }
            const int tj = ti + rem;
            int pp = 0;
            rem = pair;
            while (rem >= P - pp) { rem -= P - pp; ++pp; }
            const int qq = pp + rem;
            const double* Lr = Lp + (size_t)pair * nw;
            const int sa = 16 * ti + cn, sb = 16 * tj + cn;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int g = 0; g < n_groups; ++g) {
                const int i = 4 * g + kq;
                const bool iv = i < nw;
                const double a = (iv && sa < ns) ? V[(size_t)i * ns + sa] * Lr[i] : 0.0;
                const double b = (iv && sb < ns) ? V[(size_t)i * ns + sb] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            // as in the solver every entry of B has one writer or equal writers; B is symmetric to the bit
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * ti + kq + 4 * r, t = sb;
                if (s >= ns || t >= ns || (ti == tj && s > t)) continue;
                double w = cc[s] * cc[t] * acc[r];
                if (pp == qq && s == t) w += alpha;
                const size_t ps = (size_t)pp * ns + s, pt = (size_t)pp * ns + t, qs = (size_t)qq * ns + s, qt = (size_t)qq * ns + t;
                Bm[ps * d + qt] = w;
                Bm[pt * d + qs] = w;
                if (pp != qq) {
                    Bm[qs * d + pt] = w;
                    Bm[qt * d + ps] = w;
                }
            }
        }
        __syncthreads();

        // ================= 3. B = L_B L_B^T =================
        for (int k0 = 0; k0 < d && job_ok; k0 += FM_NB) {
            const int nb = min(FM_NB, d - k0), mrows = d - k0;
            for (int idx = tid; idx < mrows * nb; idx += FM_T) {
                const int r = idx / nb, c = idx - r * nb;
                Ysh[r * FM_LDP + c] = Bm[(size_t)(k0 + r) * d + k0 + c];
            }
            __syncthreads();
            for (int j = 0; j < nb; ++j) {
                const double pv = Ysh[j * FM_LDP + j];
                if (tid == 0 && !(pv > 0.0 && pv <= 1.79769313486231570815e308)) flag[1] = 0;
                const double dj = sqrt(pv);
                __syncthreads();                              // (everybody has read the pivot)
                for (int r = j + 1 + tid; r < mrows; r += FM_T) Ysh[r * FM_LDP + j] /= dj;
                if (tid == 0) Ysh[j * FM_LDP + j] = dj;
                __syncthreads();
                const int nc = nb - j - 1;
                for (int idx = tid; idx < (mrows - j - 1) * nc; idx += FM_T) {
                    const int r = j + 1 + idx / nc, c = j + 1 + idx % nc;
                    if (c <= r) Ysh[r * FM_LDP + c] = fma(-Ysh[r * FM_LDP + j], Ysh[c * FM_LDP + j], Ysh[r * FM_LDP + c]);
                }
                __syncthreads();
            }
            job_ok = flag[1] != 0;
            if (!job_ok) break;
            for (int idx = tid; idx < mrows * nb; idx += FM_T) {
                const int r = idx / nb, c = idx - r * nb;
                if (c <= r) Bm[(size_t)(k0 + r) * d + k0 + c] = Ysh[r * FM_LDP + c];
            }
            // A22 <- A22 - L21 L21^T, the lower triangle, in tiles of 16 x 16: a thread per entry, the sum in index order
            const int n2 = mrows - nb, nt2 = (n2 + 15) >> 4;
            for (int ti = 0; ti < nt2; ++ti)
                for (int tj = 0; tj <= ti; ++tj) {
                    const int r = nb + 16 * ti + (tid >> 4), c = nb + 16 * tj + (tid & 15);
                    if (r < mrows && c <= r) {
                        double s = Bm[(size_t)(k0 + r) * d + k0 + c];
#pragma unroll
                        for (int l = 0; l < FM_NB; ++l) s = fma(-Ysh[r * FM_LDP + l], Ysh[c * FM_LDP + l], s);
                        Bm[(size_t)(k0 + r) * d + k0 + c] = s;
                    }
                }
            __syncthreads();
        }
    }
    return job_ok;
}

template <int M, bool C>
__global__ __launch_bounds__(FM_T)
void fullmatrix_postvar_kernel(const FullMatrixPostVarParams p)
{
    constexpr int P = C ? M * M : M * (M + 1) / 2, NPAIR = P * (P + 1) / 2, MM = M * M, WPL = C ? 2 : 1;
    extern __shared__ double fmpv_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.n_omega, ns = p.n_s, d = P * ns, n_f = p.n_f, npw = P * nw;
    const int kq = lane >> 4, cn = lane & 15;
    const int ntile = (ns + 15) >> 4, n_groups = (nw + 3) >> 2;
    const double nan = __builtin_nan("");

    // ---- the LDS ----
    double* Ysh = fmpv_smem;                         // [d][FM_LDP]: the panel, then the right-hand sides
    double* part = Ysh + (size_t)d * FM_LDP;         // [2][256] partial sums
    double* fsh = part + 2 * FM_T;                   // [16] values, [16] prior sums
    int* flag = (int*)(fsh + 32);                    // [0] the job is bad, [1] B is positive definite so far

    // ---- the workgroup's slice of the scratch ----
    double* sc = p.scratch + (size_t)blockIdx.x * fmpv_scratch_doubles(M, C, nw, ns);
    double* gam = sc;          sc += (size_t)P * nw;         // [P][nw] Gamma coordinates
    double* hc = sc;           sc += (size_t)P * nw;         // [P][nw] H coordinates
    double* Wv = sc;           sc += (size_t)WPL * MM * nw;  // [nw][WPL][M][M]
    double* phiD = sc;         sc += (size_t)MM * nw;        // [nw][M][M]
    double* Lp = sc;           sc += (size_t)NPAIR * nw;     // [NPAIR][nw]
    double* Gf = sc;           sc += (size_t)FMPV_NF * P * nw;   // [P][nw][16] L_i f_i of a block of functionals
    double* Bm = sc;                                         // [d][d]

    const double* V = p.V;
    const double* cc = p.c;

    for (int job = blockIdx.x; job < p.n_job; job += gridDim.x) {
        const double alpha = p.alpha[job];
        const double* u = p.u + (size_t)job * d;
        double* o_val = p.out_value + (size_t)job * n_f;
        double* o_var = p.out_var + (size_t)job * n_f;
        double* o_pri = p.out_prior + (size_t)job * n_f;
        double* o_dv = p.want_diag ? p.out_diag + (size_t)job * npw : nullptr;
        double* o_dp = p.want_diag ? p.out_dprior + (size_t)job * npw : nullptr;
        double* o_h = p.want_diag ? p.out_h + (size_t)job * npw : nullptr;

        // ================= 1 to 3. evaluation at u, L, B = alpha I + c W c = L_B L_B^T =================
        const bool job_ok = fmpv_factor<M, C>(V, cc, p.D, u, alpha, nw, ns, gam, hc, Wv, phiD, Lp, Bm, Ysh, flag);

        if (!job_ok) {
            for (int j = tid; j < n_f; j += FM_T) { o_val[j] = nan; o_var[j] = nan; o_pri[j] = nan; }
            if (p.want_diag)
                for (int n = tid; n < npw; n += FM_T) { o_dv[n] = nan; o_dp[n] = nan; o_h[n] = nan; }
            __syncthreads();
            continue;
        }

        // ================= 4. the functionals, 16 at a time =================
        for (int f0 = 0; f0 < n_f; f0 += FMPV_NF) {
            for (int idx = tid; idx < npw * 16; idx += FM_T) {
                const int j = idx & 15, n = idx >> 4, q = n / nw, i = n - q * nw, jf = f0 + j;
                double s = 0.0;
                if (jf < n_f) {
                    const double* Fj = p.F + (size_t)jf * npw;
                    for (int pp = 0; pp < P; ++pp) s = fma(Lp[(size_t)fmpv_pair(q, pp, P) * nw + i], Fj[pp * nw + i], s);
                }
                Gf[idx] = s;
            }
            __syncthreads();
            for (int item = wave; item < P * ntile; item += 4) {
                const int q = item / ntile, t = item - q * ntile;
                const int sa = 16 * t + cn;
                const double* Gq = Gf + (size_t)q * nw * 16;
                d4 acc = d4{0.0, 0.0, 0.0, 0.0};
                for (int g = 0; g < n_groups; ++g) {
                    const int i = 4 * g + kq;
                    const bool iv = i < nw;
                    const double a = (iv && sa < ns) ? V[(size_t)i * ns + sa] : 0.0;
                    const double b = iv ? Gq[(size_t)i * 16 + cn] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = 16 * t + kq + 4 * r;
                    if (s < ns) Ysh[(q * ns + s) * FM_LDP + cn] = cc[s] * acc[r];
                }
            }
            {   // x = sum f h and the prior sum f^T L f: 16 threads per functional over interleaved terms, added in order below
                const int j = tid & 15, pt = tid >> 4, jf = f0 + j;
                double sv = 0.0, sp = 0.0;
                if (jf < n_f) {
                    const double* Fj = p.F + (size_t)jf * npw;
                    for (int n = pt; n < npw; n += 16) {
                        const double f = Fj[n];
                        sv = fma(f, hc[n], sv);
                        sp = fma(f, Gf[(size_t)n * 16 + j], sp);
                    }
                }
                part[pt * 16 + j] = sv;
                part[FM_T + pt * 16 + j] = sp;
            }
            __syncthreads();
            if (tid < 16) {
                double sv = 0.0, sp = 0.0;
                for (int pt = 0; pt < 16; ++pt) { sv += part[pt * 16 + tid]; sp += part[FM_T + pt * 16 + tid]; }
                fsh[tid] = sv; fsh[16 + tid] = sp;
            }
            __syncthreads();
            const double q = fmpv_forward(Bm, d, Ysh, part, tid);
            if (tid < 16 && f0 + tid < n_f) {
                const double prior = fsh[16 + tid];
                const double df = prior - q;                 // (a NaN stays one: not fmax)
                o_val[f0 + tid] = fsh[tid];
                o_var[f0 + tid] = (df < 0.0 ? 0.0 : df) / alpha;
                o_pri[f0 + tid] = prior / alpha;
            }
            __syncthreads();
        }

        // ================= 5. the coordinate diagonal: the columns y^(i,p) through the same L_B =================
        if (p.want_diag) {
            for (int n = tid; n < npw; n += FM_T) o_h[n] = hc[n];
            for (int n0 = 0; n0 < npw; n0 += FMPV_NF) {
                for (int idx = tid; idx < d * 16; idx += FM_T) {
                    const int j = idx & 15, row = idx >> 4, q = row / ns, s = row - q * ns, n = n0 + j;
                    double v = 0.0;
                    if (n < npw) {
                        const int pp = n / nw, i = n - pp * nw;
                        v = cc[s] * V[(size_t)i * ns + s] * Lp[(size_t)fmpv_pair(q, pp, P) * nw + i];
                    }
                    Ysh[row * FM_LDP + j] = v;
                }
                __syncthreads();
                const double q = fmpv_forward(Bm, d, Ysh, part, tid);
                if (tid < 16 && n0 + tid < npw) {
                    const int n = n0 + tid, pp = n / nw, i = n - pp * nw;
                    const double prior = Lp[(size_t)fmpv_pair(pp, pp, P) * nw + i];
                    const double df = prior - q;
                    o_dv[n] = (df < 0.0 ? 0.0 : df) / alpha;
                    o_dp[n] = prior / alpha;
                }
                __syncthreads();
            }
        }
        __syncthreads();
    }
}

} // namespace mxe
