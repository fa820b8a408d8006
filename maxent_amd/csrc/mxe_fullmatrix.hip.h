// mxe_fullmatrix.hip.h -- whole-matrix continuation (no counterpart in the reference: its guide announces a
// FullMatrixMaxEnt and its FAQ says it is not implemented).  DESIGN 4z.
//
//   n_prob data sets g^ that share V', c, D and the alpha mesh  ->  u, H, chi2, S, Q, n_iter, converged per alpha
//                                                                                                  fullmatrix_kernel<M, C>
//
// The unknown is the matrix H_i = D_i exp(Gamma_i), Gamma_i = sum_p (V' u)_ip E_p, E_p an orthonormal basis of the
// Hermitian M x M matrices (P = M (M + 1) / 2 real symmetric, C: P = M^2): the diagonal units, (e_ab + e_ba) / sqrt 2 for
// a < b, then (C) i (e_ab - e_ba) / sqrt 2.  u is [P][n_s]; x_p = Tr(E_p X) are the coordinates of a Hermitian X.
//   rho_p = c o V'^T H_p - g^_p     chi2 = sum_p |rho_p|^2 + c_perp     S = sum_i D_i sum_k (e^g - 1 - g e^g)(gamma_ik)
//   F = alpha u + c o rho           J = alpha I + (c^2 (x) 1) W         W_(p,s),(q,t) = sum_i V'_is L_i,pq V'_it
//   L_i,pq = D_i sum_kl phi(gamma_ik, gamma_il) Re( x^p_kl conj(x^q_kl) ),   x^p = W_i^H E_p W_i,   phi(a, b) = (e^a - e^b) / (a - b)
// One workgroup of 256 threads per problem walks the alpha mesh in order, warm-started, with a damped Newton iteration:
// (J + mu I) delta = F, u <- u - delta if Q = chi2 / 2 - alpha S does not rise (a Q that is not finite counts as a rise);
// a step that makes Q rise is halved up to three times (an evaluation each, no factorisation; given up for the rest of an
// alpha once three halvings were not enough), then mu grows; mu shrinks after an accepted step.  An alpha ends converged when a full undamped step was accepted whose first-order change of H,
// || L V' delta ||_F / || H ||_F, lies below tol_h (the rule of mxe_audit), or not converged after maxiter trial points.  The parts, each written once (the alpha loop is a state machine around one evaluation):
//   1. evaluation at a point: Gamma coordinates (thread per (p, i)); per omega one thread diagonalises Gamma_i by a cyclic
//      Jacobi in registers (the round-robin pair order of mxe_hermeig.hip.h, unrolled for M), forms H_i = D_i B B^H,
//      B = W e^(gamma / 2) -- Hermitian positive semi-definite in the computed factors, upper triangle computed, lower
//      mirrored -- and stores W_i and D_i phi; then h = V'^T H_p, rho, chi2, S.
//   2. L (thread per (pair, i)), then the P (P + 1) / 2 Gram products V'^T diag(L_pq) V' on v_mfma_f64_16x16x4_f64: one
//      wavefront per (pair, tile row, tile column >= tile row), the omega sum in index order inside one MFMA chain.
//   3. the Newton matrix of order d = P n_s with the right-hand side as column d, in device memory: LU with partial
//      pivoting, right-looking in blocks of 16 columns, the panel in the LDS (the largest magnitude, lowest row on ties);
//      the forward substitution is the elimination of column d; the back substitution runs in blocks of 16 rows.
// No atomics; every sum has one order that depends on the sizes alone: the bits of a problem do not depend on the batch.
// All arrays of a problem other than the panel live in its slice of a device-memory scratch (fm_scratch_doubles).
//
// fullmatrix_kernel<M, C, true> (mxe_fullmatrix_solve_metric): one error bar per matrix element.  The diagonal metric c, the
// same for all components, becomes a dense n_s x n_s factor per component, diag(1 / sigma_p) U S = Q^_p R_p, A_p = R_p^T R_p,
// shared by the batch; V is not rotated.  c stood in three places, and only they differ:
//   rho_p = R_p V^T H_p - g^_p      F_p = alpha u_p + R_p^T rho_p      J = alpha I + blockdiag_p(A_p) W
// The Gram epilogue writes the unscaled W (into the array LU works on, which is filled only afterwards); a phase of its own
// then forms block row p of J - alpha I as A_p W[(p, .), :] on the same MFMA: one wavefront per 16 x 16 tile (the row tile
// inside one p, the column tiles over all of d), the n_s-long sum in index order inside one chain, zeros beyond n_s and d.
// The other instantiations do not contain any of this: their code is that of the two-parameter template before it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxe {

constexpr int FM_MAX_M = 4;
constexpr int FM_MAX_NS = 64;
constexpr int FM_NB = 16;                 // panel width
constexpr int FM_LDP = FM_NB + 1;         // panel row stride in the LDS
constexpr int FM_MAX_SWEEPS = 30;
constexpr int FM_MAX_HALVINGS = 3;        // of a step that makes Q rise, before the damping grows
constexpr int FM_T = 256;

struct FullMatrixParams {
    int n_prob, n_omega, n_s, n_alpha, maxiter;
    double tol_h, mu_first, mu_grow, mu_max;
    const double* V;         // [n_omega][n_s]
    const double* c;         // [n_s]                      (METRIC: unused)
    const double* R;         // [P][n_s][n_s] row-major     (METRIC only)
    const double* A;         // [P][n_s][n_s] = R_p^T R_p   (METRIC only)
    const double* D;         // [n_omega]
    const double* alpha;     // [n_alpha]
    const double* ghat;      // [n_prob][P][n_s]
    const double* cperp;     // [n_prob]
    const double* u0;        // [n_prob][P][n_s] or NULL (zeros)
    double* scratch;         // [n_prob][fm_scratch_doubles]
    double* out_u;           // [n_prob][n_alpha][P][n_s]
    double* out_H;           // [n_prob][n_alpha][C ? 2 : 1][M][M][n_omega]
    double* out_chi2;        // [n_prob][n_alpha]
    double* out_S;
    double* out_Q;
    int* out_niter;
    int* out_conv;
};

__host__ __device__ inline int fm_P(int m, bool cplx) { return cplx ? m * m : m * (m + 1) / 2; }
__host__ __device__ inline size_t fm_scratch_doubles(int m, bool cplx, int nw, int ns)
{
    const size_t P = fm_P(m, cplx), d = P * ns, npair = P * (P + 1) / 2, mm = (size_t)m * m;
    // u, u_t, rho, rho_t, delta | Gamma coordinates, H coordinates | W_i | D phi | L | J - alpha I | the matrix LU works on
    return 5 * d + 2 * P * nw + (cplx ? 2 : 1) * mm * nw + mm * nw + npair * nw + d * d + d * (d + 1);
}
// the metric variant: the above, then V^T H_p [d]
__host__ __device__ inline size_t fm_scratch_doubles_metric(int m, bool cplx, int nw, int ns)
{
    return fm_scratch_doubles(m, cplx, nw, ns) + (size_t)fm_P(m, cplx) * ns;
}
// doubles of dynamic LDS: the panel (or, in the back substitution, x and 256 partial sums) | reductions | scalars
__host__ __device__ inline size_t fm_lds_doubles(int d)
{
    const size_t panel = (size_t)d * FM_LDP, solve = (size_t)d + FM_T + 16;
    return (panel > solve ? panel : solve) + 8 + 8 + 32;
}

// (e^a - e^b) / (a - b) = e^((a + b) / 2) sinh(x) / x, x = (a - b) / 2
__device__ inline double fm_phi(double a, double b)
{
    const double x = 0.5 * (a - b), x2 = x * x;
    double r;
    if (fabs(x) < 0.1)
        r = 1.0 + x2 / 6.0 * (1.0 + x2 / 20.0 * (1.0 + x2 / 42.0 * (1.0 + x2 / 72.0 * (1.0 + x2 / 110.0))));
    else
        r = sinh(x) / x;
    return exp(0.5 * (a + b)) * r;
}

// basis matrix p of the M x M Hermitian matrices: kind 0 diagonal e_aa, 1 symmetric pair, 2 antisymmetric pair (a < b)
__device__ inline void fm_basis(int p, int m, int& kind, int& a, int& b)
{
    const int no = m * (m - 1) / 2;
    if (p < m) { kind = 0; a = p; b = p; return; }
    int r = p - m;
    kind = 1;
    if (r >= no) { r -= no; kind = 2; }
    a = 0;
    while (r >= m - 1 - a) { r -= m - 1 - a; ++a; }
    b = a + 1 + r;
}

// x_kl of x = W^H E W for the basis matrix (kind, a, b); Wr, Wi: W_ak at [a * M + k]
template <int M, bool C>
__device__ inline void fm_xkl(int kind, int a, int b, const double* Wr, const double* Wi, int k, int l, double& xr, double& xi)
{
    const double ar = Wr[a * M + k], ai = C ? Wi[a * M + k] : 0.0;       // conj(W_ak) = ar - i ai
    if (kind == 0) {
        const double br = Wr[a * M + l], bi = C ? Wi[a * M + l] : 0.0;
        xr = ar * br + ai * bi; xi = ar * bi - ai * br;
        return;
    }
    const double r2 = 0.70710678118654752440;
    const double blr = Wr[b * M + l], bli = C ? Wi[b * M + l] : 0.0;
    const double bkr = Wr[b * M + k], bki = C ? Wi[b * M + k] : 0.0;
    const double alr = Wr[a * M + l], ali = C ? Wi[a * M + l] : 0.0;
    const double t1r = ar * blr + ai * bli, t1i = ar * bli - ai * blr;   // conj(W_ak) W_bl
    const double t2r = bkr * alr + bki * ali, t2i = bkr * ali - bki * alr;   // conj(W_bk) W_al
    if (kind == 1) { xr = r2 * (t1r + t2r); xi = r2 * (t1i + t2i); }
    else { xr = -r2 * (t1i - t2i); xi = r2 * (t1r - t2r); }              // i (t1 - t2) / sqrt 2
}

// cyclic two-sided Jacobi of the Hermitian M x M matrix a (ar, ai; destroyed: its diagonal ends as the eigenvalues) in
// registers; w: the eigenvectors, w[i][k] component i of eigenvector k.  Every index is a compile-time constant.
template <int M, bool C>
__device__ __forceinline__ void fm_jacobi(double (&ar)[M][M], double (&ai)[M][M], double (&wr)[M][M], double (&wi)[M][M])
{
    constexpr int ME = (M + 1) & ~1;
    double nsq = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            nsq += ar[i][j] * ar[i][j] + (C ? ai[i][j] * ai[i][j] : 0.0);
            wr[i][j] = i == j ? 1.0 : 0.0;
            wi[i][j] = 0.0;
        }
    if (M == 1) return;
    const double thresh = sqrt(nsq) * 0x1p-53 / (double)M;
    for (int sweep = 0; sweep < FM_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int step = 0; step < ME - 1; ++step) {
#pragma unroll
            for (int k = 0; k < ME / 2; ++k) {
                int pp, qq;
                hermeig_pair(step, k, ME, pp, qq);
                if (qq >= M) continue;
                const double br = ar[pp][qq], bi = C ? ai[pp][qq] : 0.0;
                const double g = C ? hypot(br, bi) : fabs(br);
                if (!(g > thresh)) continue;
                rotated = true;
                const double er = br / g, ei = bi / g;
                const double tau = (ar[qq][qq] - ar[pp][pp]) / (2.0 * g);
                double tt = 1.0 / (fabs(tau) + sqrt(1.0 + tau * tau));
                if (tau < 0.0) tt = -tt;
                const double c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;
                // columns: A <- A J, W <- W J   (J_pp = J_qq = c, J_pq = s e, J_qp = -s conj(e))
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const double xpr = ar[i][pp], xqr = ar[i][qq], vpr = wr[i][pp], vqr = wr[i][qq];
                    if (C) {
                        const double xpi = ai[i][pp], xqi = ai[i][qq], vpi = wi[i][pp], vqi = wi[i][qq];
                        ar[i][pp] = c * xpr - s * (er * xqr + ei * xqi);
                        ai[i][pp] = c * xpi - s * (er * xqi - ei * xqr);
                        ar[i][qq] = s * (er * xpr - ei * xpi) + c * xqr;
                        ai[i][qq] = s * (er * xpi + ei * xpr) + c * xqi;
                        wr[i][pp] = c * vpr - s * (er * vqr + ei * vqi);
                        wi[i][pp] = c * vpi - s * (er * vqi - ei * vqr);
                        wr[i][qq] = s * (er * vpr - ei * vpi) + c * vqr;
                        wi[i][qq] = s * (er * vpi + ei * vpr) + c * vqi;
                    } else {
                        ar[i][pp] = c * xpr - s * (er * xqr);
                        ar[i][qq] = s * (er * xpr) + c * xqr;
                        wr[i][pp] = c * vpr - s * (er * vqr);
                        wr[i][qq] = s * (er * vpr) + c * vqr;
                    }
                }
                // rows: A <- J^H A; a_pq = a_qp = 0 exactly, a_pp and a_qq real
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const double ypr = ar[pp][j], yqr = ar[qq][j];
                    double npr, nqr, npi = 0.0, nqi = 0.0;
                    if (C) {
                        const double ypi = ai[pp][j], yqi = ai[qq][j];
                        npr = c * ypr - s * (er * yqr - ei * yqi);
                        npi = c * ypi - s * (er * yqi + ei * yqr);
                        nqr = s * (er * ypr + ei * ypi) + c * yqr;
                        nqi = s * (er * ypi - ei * ypr) + c * yqi;
                    } else {
                        npr = c * ypr - s * (er * yqr);
                        nqr = s * (er * ypr) + c * yqr;
                    }
                    if (j == pp) { npi = 0.0; nqr = 0.0; nqi = 0.0; }
                    if (j == qq) { npr = 0.0; npi = 0.0; nqi = 0.0; }
                    ar[pp][j] = npr; ar[qq][j] = nqr;
                    if (C) { ai[pp][j] = npi; ai[qq][j] = nqi; }
                }
            }
        }
        if (!rotated) break;
    }
}

template <int M, bool C, bool METRIC = false>
__global__ __launch_bounds__(FM_T)
void fullmatrix_kernel(const FullMatrixParams p)
{
    constexpr int P = C ? M * M : M * (M + 1) / 2, NPAIR = P * (P + 1) / 2, MM = M * M, WPL = C ? 2 : 1;
    constexpr double R2 = 1.41421356237309504880;
    extern __shared__ double fm_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.n_omega, ns = p.n_s, d = P * ns, lda = d + 1;
    const size_t prob = blockIdx.x;

    // ---- the LDS ----
    const size_t work_doubles = fm_lds_doubles(d) - 48;
    double* panel = fm_smem;                         // [rows][FM_LDP]; back substitution: x [d], partial sums [256], t [16]
    double* red = fm_smem + work_doubles;            // [8] reductions
    double* bc = red + 8;                            // [8] broadcast
    int* piv = (int*)(bc + 8);                       // [16] pivot rows of the panel (relative to the panel), [16] ok flag

    // ---- the problem's slice of the scratch ----
    double* sc = p.scratch + prob * (METRIC ? fm_scratch_doubles_metric(M, C, nw, ns) : fm_scratch_doubles(M, C, nw, ns));
    double* u = sc;            sc += d;
    double* ut = sc;           sc += d;
    double* rho = sc;          sc += d;
    double* rhot = sc;         sc += d;
    double* delta = sc;        sc += d;
    double* gam = sc;          sc += (size_t)P * nw;         // [P][nw] Gamma coordinates (or those of V' delta)
    double* hc = sc;           sc += (size_t)P * nw;         // [P][nw] H coordinates
    double* Wv = sc;           sc += (size_t)WPL * MM * nw;  // [nw][WPL][M][M]
    double* phiD = sc;         sc += (size_t)MM * nw;        // [nw][M][M]
    double* Lp = sc;           sc += (size_t)NPAIR * nw;     // [NPAIR][nw]
    double* Jb = sc;           sc += (size_t)d * d;          // [d][d]  (c^2 (x) 1) W
    double* Aw = sc;           sc += (size_t)d * lda;        // [d][d + 1]  (METRIC: before it is filled, the unscaled W [d][d])
    double* hv = sc;                                         // [d] V^T H_p (METRIC only)

    const double* V = p.V;
    const double* cc = p.c;
    const double* ghat = p.ghat + prob * d;
    const double cperp = p.cperp[prob];

    for (int k = tid; k < d; k += FM_T) u[k] = p.u0 ? p.u0[prob * d + k] : 0.0;
    __syncthreads();

    // state of the alpha loop (the same in every thread)
    int ia = -1, it = 0, conv = 0, nhalf = 0;
    bool trial = false, jac_valid = false, half_ok = true;
    double alpha = 0.0, mu = 0.0, Q0 = 0.0, chi2_0 = 0.0, S_0 = 0.0, hn2_0 = 1.0, corr = 0.0;
    bool lu_ok = true;

    while (true) {
        // ================= 1. evaluation at x: u (a point of the path; ia >= 0: its outputs) or u_t (a trial) =================
        const double* x = trial ? ut : u;
        double* rho_x = trial ? rhot : rho;
        const bool write_out = !trial && ia >= 0;
        for (int idx = tid; idx < P * nw; idx += FM_T) {
            const int pp = idx / nw, i = idx - pp * nw;
            const double* vr = V + (size_t)i * ns;
            const double* xr = x + pp * ns;
            double s = 0.0;
            for (int k = 0; k < ns; ++k) s = fma(vr[k], xr[k], s);
            gam[idx] = s;
        }
        __syncthreads();
        double s_part = 0.0, h_part = 0.0;
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
            const double Di = p.D[i];
            double gk[M], eh[M];
#pragma unroll
            for (int k = 0; k < M; ++k) {
                gk[k] = ar[k][k];
                eh[k] = exp(0.5 * gk[k]);
                const double e = exp(gk[k]);
                s_part += Di * (e - 1.0 - gk[k] * e);
            }
            // H = D B B^H, B_ak = W_ak e^(gamma_k / 2): the upper triangle, the lower its conjugate
            double* oh = write_out ? p.out_H + ((prob * p.n_alpha + ia) * WPL * MM) * (size_t)nw + i : nullptr;
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
                        if (a == b) {
                            hc[a * nw + i] = sr;
                            h_part += sr * sr;
                            if (oh) { oh[(size_t)(a * M + a) * nw] = sr; if (C) oh[(size_t)(MM + a * M + a) * nw] = 0.0; }
                        } else {
                            hc[pp * nw + i] = R2 * sr;
                            if (C) hc[(pp + M * (M - 1) / 2) * nw + i] = R2 * si;
                            h_part += 2.0 * (sr * sr + si * si);
                            if (oh) {
                                oh[(size_t)(a * M + b) * nw] = sr; oh[(size_t)(b * M + a) * nw] = sr;
                                if (C) { oh[(size_t)(MM + a * M + b) * nw] = si; oh[(size_t)(MM + b * M + a) * nw] = -si; }
                            }
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
                    po[a * M + k] = Di * fm_phi(gk[a], gk[k]);
                }
        }
        __syncthreads();
        const double S_x = hermeig_reduce<FM_T, false>(s_part, red);
        const double hn2_x = hermeig_reduce<FM_T, false>(h_part, red);
        double c_part = 0.0;
        for (int idx = tid; idx < d; idx += FM_T) {
            const int pp = idx / ns, k = idx - pp * ns;
            const double* hp = hc + (size_t)pp * nw;
            double s = 0.0;
            for (int i = 0; i < nw; ++i) s = fma(V[(size_t)i * ns + k], hp[i], s);
            if constexpr (METRIC) {
                hv[idx] = s;
            } else {
                const double r = cc[k] * s - ghat[idx];
                rho_x[idx] = r;
                c_part = fma(r, r, c_part);
            }
        }
        __syncthreads();
        if constexpr (METRIC) {
            for (int idx = tid; idx < d; idx += FM_T) {
                const int pp = idx / ns;
                const double* Rr = p.R + (size_t)idx * ns;           // row k of R_p
                const double* hp = hv + (size_t)pp * ns;
                double s = 0.0;
                for (int t = 0; t < ns; ++t) s = fma(Rr[t], hp[t], s);
                const double r = s - ghat[idx];
                rho_x[idx] = r;
                c_part = fma(r, r, c_part);
            }
            __syncthreads();
        }
        const double chi2_x = hermeig_reduce<FM_T, false>(c_part, red) + cperp;

        // ================= the state machine =================
        bool to_point = false;                       // the next evaluation is that of u itself: the end of an alpha
        if (!trial) {
            if (ia >= 0) {
                const size_t o = prob * p.n_alpha + ia;
                for (int k = tid; k < d; k += FM_T) p.out_u[o * d + k] = u[k];
                if (tid == 0) {
                    p.out_chi2[o] = chi2_x; p.out_S[o] = S_x; p.out_Q[o] = 0.5 * chi2_x - alpha * S_x;
                    p.out_niter[o] = it; p.out_conv[o] = conv;
                }
            }
            if (++ia == p.n_alpha) break;
            alpha = p.alpha[ia];
            chi2_0 = chi2_x; S_0 = S_x; hn2_0 = hn2_x;
            Q0 = 0.5 * chi2_x - alpha * S_x;
            mu = 0.0; it = 0; conv = 0; nhalf = 0; half_ok = true;
        } else {
            const double Q1 = 0.5 * chi2_x - alpha * S_x;
            const double slack = 0x1p-44 * (0.5 * chi2_0 + alpha * fabs(S_0));
            const bool good = lu_ok && isfinite(Q1) && isfinite(corr) && Q1 <= Q0 + slack;
            if (good) {
                double* t = u; u = ut; ut = t;
                t = rho; rho = rhot; rhot = t;
                Q0 = Q1; chi2_0 = chi2_x; S_0 = S_x; hn2_0 = hn2_x;
                jac_valid = false;
                if (mu == 0.0 && nhalf == 0 && corr < p.tol_h) { conv = 1; to_point = true; }
                mu = mu > p.mu_first * alpha ? mu / p.mu_grow : 0.0;
                nhalf = 0;
            } else if (half_ok && lu_ok && isfinite(corr) && nhalf < FM_MAX_HALVINGS && it < p.maxiter) {
                // the same direction, half as far: an evaluation, no factorisation
                ++nhalf; ++it;
                corr *= 0.5;
                for (int k = tid; k < d; k += FM_T) {
                    const double dl = 0.5 * delta[k];
                    delta[k] = dl;
                    ut[k] = u[k] - dl;
                }
                __syncthreads();
                continue;
            } else {
                // (a direction on which three halvings were not enough: this alpha is steered by the damping alone from here)
                if (nhalf == FM_MAX_HALVINGS) half_ok = false;
                mu = mu == 0.0 ? p.mu_first * alpha : mu * p.mu_grow;
                nhalf = 0;
                if (!(mu <= p.mu_max * alpha)) to_point = true;
            }
        }
        if (it >= p.maxiter) to_point = true;
        if (to_point) {
            // W_i, phi and rho must be those of u when the next alpha starts from here: evaluate u once more (with its outputs)
            if (trial) { trial = false; continue; }
            // (u was evaluated just now: maxiter < 1)
            continue;
        }

        // ================= 2. L and the Gram products at u (when u moved since they were formed) =================
        if (!jac_valid) {
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
            const int ntile = (ns + 15) >> 4, ntp = ntile * (ntile + 1) / 2, n_groups = (nw + 3) >> 2;
            const int kq = lane >> 4, cn = lane & 15;
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
                // element (s, t) of the block (p, q) is also (t, s) of it and (s, t), (t, s) of the block (q, p); a diagonal
                // tile is written from s <= t alone, so that every entry of J has one writer or equal writers
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = 16 * ti + kq + 4 * r, t = sb;
                    if (s >= ns || t >= ns || (ti == tj && s > t)) continue;
                    const double w = acc[r];
                    const size_t ps = (size_t)pp * ns + s, pt = (size_t)pp * ns + t, qs = (size_t)qq * ns + s, qt = (size_t)qq * ns + t;
                    if constexpr (METRIC) {
                        Aw[ps * d + qt] = w;
                        Aw[pt * d + qs] = w;
                        if (pp != qq) {
                            Aw[qs * d + pt] = w;
                            Aw[qt * d + ps] = w;
                        }
                    } else {
                        const double c2s = cc[s] * cc[s], c2t = cc[t] * cc[t];
                        Jb[ps * d + qt] = c2s * w;
                        Jb[pt * d + qs] = c2t * w;
                        if (pp != qq) {
                            Jb[qs * d + pt] = c2s * w;
                            Jb[qt * d + ps] = c2t * w;
                        }
                    }
                }
            }
            if constexpr (METRIC) {
                // block row p of J - alpha I = A_p W[(p, .), :]: W [d][d] in Aw; the row tile lies inside one p, the column
                // tiles run over all of d; rows and the sum beyond n_s and columns beyond d are fed as zeros, never stored
                __syncthreads();
                const int nct = (d + 15) >> 4, nkg = (ns + 3) >> 2;
                for (int item = wave; item < P * ntile * nct; item += 4) {
                    const int pp = item / (ntile * nct), rem = item - pp * ntile * nct;
                    const int ti = rem / nct, tc = rem - ti * nct;
                    const double* Ap = p.A + (size_t)pp * ns * ns;
                    const double* Wp = Aw + (size_t)pp * ns * d;
                    const int row = 16 * ti + cn, col = 16 * tc + cn;
                    // the operands of eight links of the chain are loaded before the eight run, so that their loads overlap;
                    // the chain itself is the same values in the same order
                    constexpr int NKG = 8;
                    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
                    for (int g0 = 0; g0 < nkg; g0 += NKG) {
                        double av[NKG], bv[NKG];
#pragma unroll
                        for (int g = 0; g < NKG; ++g) {
                            const int s = 4 * (g0 + g) + kq;
                            const bool sv = g0 + g < nkg && s < ns;
                            av[g] = (sv && row < ns) ? Ap[(size_t)row * ns + s] : 0.0;
                            bv[g] = (sv && col < d) ? Wp[(size_t)s * d + col] : 0.0;
                        }
#pragma unroll
                        for (int g = 0; g < NKG; ++g)
                            if (g0 + g < nkg) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g], bv[g], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = 16 * ti + kq + 4 * r;
                        if (k < ns && col < d) Jb[((size_t)pp * ns + k) * d + col] = acc[r];
                    }
                }
            }
            jac_valid = true;
            __syncthreads();
        }

        // ================= 3. (J + mu I) delta = F =================
        for (int idx = tid; idx < d * lda; idx += FM_T) {
            const int r = idx / lda, c = idx - r * lda;
            double v;
            if (c < d) { v = Jb[(size_t)r * d + c]; if (r == c) v += alpha + mu; }
            else if constexpr (METRIC) continue;                     // (column d: below)
            else v = alpha * u[r] + cc[r % ns] * rho[r];
            Aw[idx] = v;
        }
        if constexpr (METRIC) {
            // column d, F_p = alpha u_p + R_p^T rho_p: a thread per (p, k) in a loop of its own (inside the loop above the
            // n_s-long sum would stall its wavefront once per row)
            for (int r = tid; r < d; r += FM_T) {
                const int pp = r / ns, k = r - pp * ns;
                const double* Rc = p.R + (size_t)pp * ns * ns + k;   // column k of R_p
                const double* rp = rho + (size_t)pp * ns;
                double s = 0.0;
                for (int t = 0; t < ns; ++t) s = fma(Rc[(size_t)t * ns], rp[t], s);
                Aw[(size_t)r * lda + d] = alpha * u[r] + s;
            }
        }
        if (tid == 0) piv[16] = 1;
        __syncthreads();
        for (int k0 = 0; k0 < d; k0 += FM_NB) {
            const int nb = min(FM_NB, d - k0), mrows = d - k0;
            for (int idx = tid; idx < mrows * nb; idx += FM_T) {
                const int r = idx / nb, c = idx - r * nb;
                panel[r * FM_LDP + c] = Aw[(size_t)(k0 + r) * lda + k0 + c];
            }
            __syncthreads();
            for (int j = 0; j < nb; ++j) {
                // the pivot: largest magnitude of column j from row j on, the lowest row on ties; a NaN never wins
                double best = -1.0;
                int bi = j;
                for (int r = j + tid; r < mrows; r += FM_T) {
                    const double v = fabs(panel[r * FM_LDP + j]);
                    if (v > best) { best = v; bi = r; }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double ov = __shfl_xor(best, off, 64);
                    const int oi = __shfl_xor(bi, off, 64);
                    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
                }
                if (lane == 0) { red[wave] = best; red[4 + wave] = (double)bi; }
                __syncthreads();
                if (tid == 0) {
                    double bv = red[0];
                    int br = (int)red[4];
                    for (int w = 1; w < 4; ++w) {
                        const double ov = red[w];
                        const int oi = (int)red[4 + w];
                        if (ov > bv || (ov == bv && oi < br)) { bv = ov; br = oi; }
                    }
                    piv[j] = br;
                    if (!(bv > 0.0) || !(bv <= 1.79769313486231570815e308)) piv[16] = 0;
                }
                __syncthreads();
                const int pr = piv[j];
                if (pr != j && tid < nb) {
                    const double t = panel[j * FM_LDP + tid];
                    panel[j * FM_LDP + tid] = panel[pr * FM_LDP + tid];
                    panel[pr * FM_LDP + tid] = t;
                }
                __syncthreads();
                const double pv = panel[j * FM_LDP + j];
                const double inv = 1.0 / pv;
                __syncthreads();                                  // (everybody has read the pivot row's head)
                for (int r = j + 1 + tid; r < mrows; r += FM_T) panel[r * FM_LDP + j] *= inv;
                __syncthreads();
                const int nc = nb - j - 1;
                for (int idx = tid; idx < (mrows - j - 1) * nc; idx += FM_T) {
                    const int r = j + 1 + idx / nc, c = j + 1 + idx % nc;
                    panel[r * FM_LDP + c] = fma(-panel[r * FM_LDP + j], panel[j * FM_LDP + c], panel[r * FM_LDP + c]);
                }
                __syncthreads();
            }
            // the panel back; its row swaps on the columns to its right (L to its left is not read again: the forward
            // substitution is the elimination of column d)
            for (int idx = tid; idx < mrows * nb; idx += FM_T) {
                const int r = idx / nb, c = idx - r * nb;
                Aw[(size_t)(k0 + r) * lda + k0 + c] = panel[r * FM_LDP + c];
            }
            for (int c = k0 + nb + tid; c < lda; c += FM_T) {
                for (int j = 0; j < nb; ++j) {
                    const int pr = piv[j];
                    if (pr != j) {
                        const double t = Aw[(size_t)(k0 + j) * lda + c];
                        Aw[(size_t)(k0 + j) * lda + c] = Aw[(size_t)(k0 + pr) * lda + c];
                        Aw[(size_t)(k0 + pr) * lda + c] = t;
                    }
                }
            }
            __syncthreads();
            // U12 = L11^-1 A12 and A22 <- A22 - L21 U12, column by column to the right of the panel (the right-hand side is
            // one of them): the 16 values of a column of U12 in registers, the column's rows dealt to as many threads as
            // there are to spare (each solves the column for itself: the same bits; the first of them stores it)
            const int c1 = k0 + nb, ncr = lda - c1, nrr = d - c1;
            const int nchunk = ncr >= FM_T ? 1 : FM_T / ncr;
            for (int base = 0; base < ncr; base += FM_T) {
                const int cidx = base + (nchunk == 1 ? tid : tid % ncr), chunk = nchunk == 1 ? 0 : tid / ncr;
                const bool act = cidx < ncr && chunk < nchunk;
                const int c = c1 + (act ? cidx : 0);
                double x[FM_NB];
#pragma unroll
                for (int l = 0; l < FM_NB; ++l) x[l] = (act && l < nb) ? Aw[(size_t)(k0 + l) * lda + c] : 0.0;
                __syncthreads();                                  // (every thread of a column has read it before one stores it)
                if (act) {
#pragma unroll
                    for (int j = 1; j < FM_NB; ++j)
                        if (j < nb) {
                            double s = x[j];
#pragma unroll
                            for (int l = 0; l < j; ++l) s = fma(-panel[j * FM_LDP + l], x[l], s);
                            x[j] = s;
                        }
                    if (chunk == 0) {
#pragma unroll
                        for (int j = 1; j < FM_NB; ++j)
                            if (j < nb) Aw[(size_t)(k0 + j) * lda + c] = x[j];
                    }
                    for (int rr = chunk; rr < nrr; rr += nchunk) {
                        const double* lrow = panel + (size_t)(nb + rr) * FM_LDP;
                        double s = Aw[(size_t)(c1 + rr) * lda + c];
#pragma unroll
                        for (int l = 0; l < FM_NB; ++l)
                            if (l < nb) s = fma(-lrow[l], x[l], s);
                        Aw[(size_t)(c1 + rr) * lda + c] = s;
                    }
                }
            }
            __syncthreads();
        }
        lu_ok = piv[16] != 0;
        // back substitution U x = y (y: column d), blocks of 16 rows from the bottom
        {
            double* xs = panel;                  // [d]
            double* part = panel + d;            // [256]
            double* tsum = part + FM_T;          // [16]
            const int nblk = (d + 15) >> 4;
            for (int blk = nblk - 1; blk >= 0; --blk) {
                const int r0 = 16 * blk, r1 = min(d, r0 + 16);
                {
                    const int row = r0 + (tid >> 4), pt = tid & 15;
                    double s = 0.0;
                    if (row < r1)
                        for (int j = r1 + pt; j < d; j += 16) s = fma(Aw[(size_t)row * lda + j], xs[j], s);
                    part[tid] = s;
                }
                __syncthreads();
                if (tid < 16) {
                    double s = 0.0;
                    for (int q = 0; q < 16; ++q) s += part[tid * 16 + q];
                    tsum[tid] = s;
                }
                __syncthreads();
                if (tid == 0) {
                    for (int r = r1 - 1; r >= r0; --r) {
                        double s = Aw[(size_t)r * lda + d] - tsum[r - r0];
                        for (int j = r + 1; j < r1; ++j) s = fma(-Aw[(size_t)r * lda + j], xs[j], s);
                        xs[r] = s / Aw[(size_t)r * lda + r];
                    }
                }
                __syncthreads();
            }
            for (int k = tid; k < d; k += FM_T) {
                const double dl = xs[k];
                delta[k] = dl;
                ut[k] = u[k] - dl;
            }
            __syncthreads();
        }
        ++it;
        nhalf = 0;
        // the first-order change of H the step makes, || L V' delta ||_F / || H ||_F
        for (int idx = tid; idx < P * nw; idx += FM_T) {
            const int pp = idx / nw, i = idx - pp * nw;
            const double* vr = V + (size_t)i * ns;
            const double* xr = delta + pp * ns;
            double s = 0.0;
            for (int k = 0; k < ns; ++k) s = fma(vr[k], xr[k], s);
            gam[idx] = s;
        }
        __syncthreads();
        double n_part = 0.0;
        for (int idx = tid; idx < P * nw; idx += FM_T) {
            const int pp = idx / nw, i = idx - pp * nw;
            double s = 0.0;
            for (int qq = 0; qq < P; ++qq) {
                const int lo = min(pp, qq), hi = max(pp, qq);
                const int pair = lo * P - lo * (lo - 1) / 2 + (hi - lo);
                s = fma(Lp[(size_t)pair * nw + i], gam[qq * nw + i], s);
            }
            n_part = fma(s, s, n_part);
        }
        __syncthreads();
        corr = sqrt(hermeig_reduce<FM_T, false>(n_part, red) / hn2_0);
        trial = true;
    }
}

} // namespace mxe
