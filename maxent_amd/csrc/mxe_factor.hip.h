// mxe_factor.hip.h -- the Cholesky factor of B = c W c + a I in LDS, and what its five consumers share
//
//   factor_B            -> logdet_kernel      (mxe_logdet, below)
//                          postvar_kernel     (mxe_posterior_var, mxe_postvar.hip.h)
//                          postsample_kernel  (mxe_posterior_sample, mxe_postsample.hip.h)
//                          fitdiag_kernel     (mxe_fit_diagnostics, mxe_fitdiag.hip.h)
//                          response_kernel    (mxe_response, mxe_response.hip.h)
//
// In the whitened singular basis (K^T Sigma^-1 K = V' c^2 V'^T) the curvature of Q = eta chi2 / 2 - alpha~ S collapses
// onto the n_s x n_s matrix
//
//   B = c W c + a I,   W = V'^T diag(w) V',   a = alpha~ / eta,   B = L L^T
//
// with w rebuilt from the hidden image (normal entropy: w = H; plus-minus: w = sqrt(H^2 + 4 D^2), free of cancellation).
// One workgroup (4 waves, 256 threads) per problem calls factor_B, which
//   1. builds w in LDS (wsh) and marks a value that is not finite through an LDS flag;
//   2. forms W by v_mfma_f64_16x16x4_f64: the omega rows go to the four waves round-robin in groups of 4, the
//      upper-triangular 16 x 16 tiles (mt <= t) of one tile row per sweep of V', the waves' partial tiles are added
//      in wave order (add_tiles_in_wave_order);
//   3. forms B on the lower triangle of Bm ([NP][NP + 1] doubles) and runs a right-looking Cholesky there with all
//      threads; L_jj is stored on the diagonal.
// It returns false, to every thread alike, when a w is not finite or a pivot is not in (0, DBL_MAX]; Bm then holds nothing
// of use.  Bits do not depend on the batch: every sum other than the wave-ordered one runs in index order in one thread
// or inside one MFMA chain.  factor_B is __forceinline__: it is the whole first half of its three kernels and must not
// cost them a call, nor its accumulators a trip through scratch.
//
// Once B is mirrored to its lower triangle, the rows 0 .. NP/2-1 of the columns NP/2 .. NP-1 (all strictly above the
// diagonal) are dead, NP^2/4 >= 16 NP doubles: a block of 16 right-hand sides lives there (pv_y), row k of it the 16
// doubles at row k/2, column NP/2 + 16 (k mod 2).  pv_forward_solve and ps_backward_solve run L Z = Y and L^T X = Z on
// that block in place; block_times_Vt multiplies it with the rows of V'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxe {

typedef double d4 __attribute__((ext_vector_type(4)));

// what the kernels that factorise B per problem are handed (the posterior kernels add their own fields)
struct FactorParams {
    const double* V;            // [n_ds][nwp][NP]
    const double* c;            // [n_ds][NP]
    const int* elem_ds;         // [n_elem]
    const int* elem_kind;       // [n_elem]
    const double* D;            // [n_elem][nwp]
    const int* elem;            // [P] element of a problem
    const double* alpha;        // [P] alpha~ / eta
    const double* H;            // rows of n_omega values
    const int* row;             // [P] row of H that belongs to a problem, or NULL: row p
    int nw, nwp, ns;
};

// one problem's operands
struct FactorProblem {
    const double* V;            // [nwp][NP] of its data set
    const double* cc;           // [NP]
    const double* Hp;           // [nw] its H row
    const double* Dp;           // [nwp] its default model
    int kind;                   // 0: normal entropy, else plus-minus
    double a;
};

template <int NP>
__device__ __forceinline__ FactorProblem resolve_problem(const FactorParams& p, size_t prob)
{
    const int e = p.elem[prob];
    const int ds = p.elem_ds[e];
    FactorProblem q;
    q.V = p.V + (size_t)ds * p.nwp * NP;
    q.cc = p.c + (size_t)ds * NP;
    q.Hp = p.H + (size_t)(p.row ? p.row[prob] : (int)prob) * p.nw;
    q.Dp = p.D + (size_t)e * p.nwp;
    q.kind = p.elem_kind[e];
    q.a = p.alpha[prob];
    return q;
}

// element (k, j) of a block of 16 right-hand sides inside B's dead upper-right block (see above)
template <int NP> __device__ __forceinline__ int pv_y(int k, int j) { return (k >> 1) * (NP + 1) + NP / 2 + ((k & 1) << 4) + j; }

// The four waves add their partial tiles t0 <= t < t1 one after the other: element r of tile t goes to Bm[at(t, r)].
// Called by all threads; ends with a barrier.  (at gives an index, not an address: handed pointers, the compiler chose
// other registers and another layout for the whole kernel, and postvar_kernel ran 2 % slower -- DESIGN 4c.)
template <int NT, typename At>
__device__ __forceinline__ void add_tiles_in_wave_order(double* Bm, const d4 (&acc)[NT], int t0, int t1, int wave, At at)
{
    for (int ph = 0; ph < 4; ++ph) {
        if (wave == ph) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t >= t0 && t < t1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Bm[at(t, r)] += acc[t][r];
                }
        }
        __syncthreads();
    }
}

// Bm <- L (lower triangle, L_jj on the diagonal), wsh <- w; flag: one double of LDS.  See the head of the file.
template <int NT>
__device__ __forceinline__ bool factor_B(const FactorProblem& q, int nw, int nwp, int ns, double* Bm, double* wsh, double* flag)
{
    constexpr int NP = 16 * NT, LD = NP + 1;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double* V = q.V;
    const double* cc = q.cc;
    const double a = q.a;
    if (tid == 0) *flag = 0.0;
    __syncthreads();
    bool finite = true;
    for (int i = tid; i < nwp; i += 256) {
        double w = 0.0;
        if (i < nw) {
            const double h = q.Hp[i];
            if (q.kind == 0) w = h;
            else { const double d2 = 2.0 * q.Dp[i]; w = sqrt(fma(h, h, d2 * d2)); }
            if (!(fabs(w) <= 1.79769313486231570815e308)) finite = false;
        }
        wsh[i] = w;
    }
    if (!finite) *flag = 1.0;            // (every writer writes the same value)
    for (int i = tid; i < NP * LD; i += 256) Bm[i] = 0.0;
    __syncthreads();
    bool ok = *flag == 0.0;
    if (!ok) return false;               // (uniform)
    const int kq = lane >> 4, cn = lane & 15;
    const int n_groups = (nw + 3) >> 2;          // (the rows of V' behind n_omega are zero)
    const int ntile = (ns + 15) >> 4;            // tile rows / columns that hold data
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
        add_tiles_in_wave_order<NT>(Bm, acc, mt, ntile, wave,
                                    [=](int t, int r) { return (16 * mt + kq + 4 * r) * LD + 16 * t + cn; });
    }
    // B = c W c + a I from the upper triangle (row <= col), written to the lower one
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
        __syncthreads();                         // everybody has read the pivot
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
    return ok;                                   // (uniform: every thread saw the same pivots)
}

// L Z = Y for the block of 16 right-hand sides (pv_y), in place; returns (to threads 0..15) |z_j|^2 of column j = tid
template <int NP>
__device__ inline double pv_forward_solve(double* Bm, int ns, int tid)
{
    constexpr int LD = NP + 1;
    double q = 0.0;
    const int ntile = (ns + 15) >> 4;
    for (int J = 0; J < ntile; ++J) {
        const int k0 = 16 * J, k1 = min(k0 + 16, ns);
        if (tid < 16) {
            for (int k = k0; k < k1; ++k) {
                double s = Bm[pv_y<NP>(k, tid)];
                for (int m = k0; m < k; ++m) s = fma(-Bm[k * LD + m], Bm[pv_y<NP>(m, tid)], s);
                s /= Bm[k * LD + k];
                Bm[pv_y<NP>(k, tid)] = s;
                q = fma(s, s, q);
            }
        }
        __syncthreads();
        const int below = ns - k1;
        for (int idx = tid; idx < below * 16; idx += 256) {
            const int m = k1 + (idx >> 4), j = idx & 15;
            double s = Bm[pv_y<NP>(m, j)];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) s = fma(-Bm[m * LD + k0 + kk], Bm[pv_y<NP>(k0 + kk, j)], s);   // (rows below exist: the block is full)
            Bm[pv_y<NP>(m, j)] = s;
        }
        __syncthreads();
    }
    return q;
}

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

// One 16 x 16 tile of (block of 16 right-hand sides)^T V'^T: element r of the result belongs to the right-hand side
// kq + 4 r and to the omega point i of this lane (iv: it exists); the k-sum over the kgroups groups of 4 singular
// directions runs inside one MFMA chain.
template <int NP>
__device__ __forceinline__ d4 block_times_Vt(const double* Bm, const double* V, int i, bool iv, int kgroups, int kq, int cn)
{
    const double* vrow = V + (size_t)(iv ? i : 0) * NP + kq;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < kgroups; ++g)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Bm[pv_y<NP>(4 * g + kq, cn)], iv ? vrow[4 * g] : 0.0, acc, 0, 0, 0);
    return acc;
}

// ---- log det(I + M W / alpha) of every problem of the last launch (mxe_logdet) ---------------------------------------
// In the whitened basis M = diag(c^2), so det(I + M W / a) = det(B) / a^n_s over ALL n_s kept directions (no
// active-subspace cut here): log det = 2 sum_j log L_jj - n_s log a, NaN when factor_B fails.  Problem prob is row prob
// of H and belongs to the chain prob / n_alpha.  LDS: Bm | wsh | 4 doubles, the first of them factor_B's flag.
inline size_t logdet_lds_bytes(int NP, int nwp) { return ((size_t)NP * (NP + 1) + (size_t)nwp + 4) * sizeof(double); }

template <int NT>
__global__ __launch_bounds__(256)
void logdet_kernel(const double* __restrict__ Vall, const double* __restrict__ call,
                   const int* __restrict__ elem_ds, const int* __restrict__ elem_kind,
                   const double* __restrict__ Dall, const int* __restrict__ elem_of_chain,
                   const double* __restrict__ alpha, const double* __restrict__ H,
                   double* __restrict__ out, int n_alpha, int nw, int nwp, int ns)
{
    constexpr int NP = 16 * NT, LD = NP + 1;
    extern __shared__ double sm[];
    double* Bm = sm;                 // [NP][LD]
    double* wsh = Bm + NP * LD;      // [nwp]
    const size_t prob = blockIdx.x;
    const int e = elem_of_chain[prob / n_alpha];
    const int ds = elem_ds[e];
    FactorProblem q;
    q.V = Vall + (size_t)ds * nwp * NP;
    q.cc = call + (size_t)ds * NP;
    q.Hp = H + prob * nw;
    q.Dp = Dall + (size_t)e * nwp;
    q.kind = elem_kind[e];
    q.a = alpha[prob];
    const bool ok = factor_B<NT>(q, nw, nwp, ns, Bm, wsh, wsh + nwp);
    // log L_jj by thread j, into the dead slot right of the diagonal (column NP of the last row is padding); one
    // thread adds them in index order
    const int tid = threadIdx.x;
    if (ok && tid < ns) Bm[tid * LD + tid + 1] = log(Bm[tid * LD + tid]);
    __syncthreads();
    if (tid == 0) {
        double logsum = 0.0;
        if (ok) {
#pragma unroll 8
            for (int j = 0; j < ns; ++j) logsum += Bm[j * LD + j + 1];
        }
        out[prob] = ok ? 2.0 * logsum - ns * log(q.a) : __builtin_nan("");
    }
}

} // namespace mxe
