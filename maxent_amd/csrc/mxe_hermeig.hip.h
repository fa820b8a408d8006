// mxe_hermeig.hip.h -- is a matrix-valued spectral function positive?  (no counterpart in the reference)
//
//   n_mat matrices A (m x m, real or complex)  ->  eigenvalues and eigenvectors of Herm(A) = (A + A^H) / 2, its projection
//                                                  onto the cone lambda >= floor, the weight below the floor     hermeig_kernel
//
// Element-wise continuation gives a matrix A(omega) that is Hermitian but, as a rule, not positive semi-definite.  Whether,
// where and by how much is one small Hermitian eigenproblem per frequency (and per alpha): tens of thousands of them.  The
// one-sided Jacobi codes of mxe_svd.hip.h and mxe_bins.hip.h cannot do it: an indefinite matrix has eigenvalues +-lambda
// that share a singular value, and [[0, a], [a, 0]] has orthogonal columns already.  This is a two-sided cyclic Jacobi.
//
// A (m x ld, ld = m | 1) and W = V^T (row p of W is column p of V) stay in the LDS for the whole solve, real and imaginary
// parts in planes of their own (the real path has no imaginary planes: half the LDS).  Workgroups of 256 threads; a matrix
// is worked on by T threads: T = 64 (one wavefront per matrix, four matrices per workgroup) for m <= HERMEIG_WAVE_M,
// T = 256 (one workgroup per matrix) above.
//   1. load A, form Herm(A), || A - A^H ||_F, the pair condition max_{i<j} |a_ij| - sqrt(max(a_ii, 0) max(a_jj, 0)), is it
//      finite, || Herm(A) ||_F (scaled by the largest magnitude).  W = I.
//   2. sweeps of me - 1 steps (me = m rounded up to even) of the round-robin ordering: step s pairs (me - 1, s) and
//      ((s + k) mod (me - 1), (s - k) mod (me - 1)), k = 1 .. me / 2 - 1 -- disjoint pairs, every pair once per sweep; a pair
//      with an index >= m (odd m) has a bye.  Per step:
//        a. thread k forms the rotation of pair k from a_pp, a_qq, a_pq: e = a_pq / |a_pq|, tau = (a_qq - a_pp) / (2 |a_pq|),
//           t = sign(tau) / (|tau| + sqrt(1 + tau^2)) (the smaller root), c = 1 / sqrt(1 + t^2), s = t c;
//           J_pp = J_qq = c, J_pq = s e, J_qp = -s conj(e).  A pair with |a_pq| <= 2^-53 || A ||_F / m is skipped.   barrier
//        b. columns: A <- A J, items (pair, row).                                                                 barrier
//        c. rows: A <- J^H A and W <- J^T W (that is V <- V J), items (pair, column); the item that writes a_pq, a_qp
//           writes exact zeros, the one that writes a_pp, a_qq a real number.                                     barrier
//      A sweep in which no pair of the matrix rotated ends its solve (info = the sweeps that rotated); after
//      HERMEIG_MAX_SWEEPS sweeps info = -2.  A matrix that is done does no more work, but its threads run every barrier:
//      the workgroup leaves the sweep loop on one value all its threads read from the LDS after a barrier (all its matrices
//      done), so every wavefront runs the same number of barriers.
//   3. lambda ascending (rank sort, by index on ties), the permutation applied to V; one Newton-Schulz step
//      V <- V (3 I - V^H V) / 2 takes the accumulated rounding of the rotations out of the orthogonality of V; every
//      eigenvector scaled to unit norm with its component of largest magnitude (lowest index on ties) real and positive,
//      as bins_eig_kernel does it.
//   4. P = V max(Lambda, floor) V^H formed in the LDS where A was: the upper triangle computed (sum over the eigenvalues in
//      ascending order), the lower its conjugate, the diagonal real -- exactly Hermitian --, stored with coalesced 16-byte
//      stores (a real matrix of odd m: 8-byte stores, its rows do not start on 16 bytes).
// A matrix with a NaN or an Inf: info -1, NaN in every output of that matrix.  No atomics; every sum has one order that
// depends on (m, real or complex) alone: a matrix's bits depend on nothing but the matrix, alone or in a batch, and repeat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mxe {

constexpr int HERMEIG_MAX_M = 64;         // two padded 64 x 64 complex matrices: 133 KB of the 160 KB of LDS
constexpr int HERMEIG_MAX_SWEEPS = 30;
constexpr int HERMEIG_T = 256;
// m <= HERMEIG_WAVE_M: one wavefront per matrix.  A step of m = 16 has 8 x 16 = 128 items, two per lane of one wavefront;
// four wavefronts on one matrix would leave three of them idle at every m below that, and the LDS of four 16 x 16 complex
// matrices (36 KB) still admits four workgroups -- sixteen wavefronts -- per CU.  From m = 17 on a step has more items than
// two per lane and the LDS, not the wavefront count, bounds the matrices resident on a CU.
constexpr int HERMEIG_WAVE_M = 16;

struct HermEigParams {
    int n_mat, m;
    double floor;
    const double* A;         // [n_mat][m][m] (complex: [2])
    double* lambda;          // [n_mat][m]             (every output may be NULL)
    double* vec;             // [n_mat][m][m] ([2])
    double* proj;            // [n_mat][m][m] ([2])
    double* neg;             // [n_mat]
    double* dist;            // [n_mat]
    double* pair;            // [n_mat]
    double* asym;            // [n_mat]
    int* info;               // [n_mat]
};

__host__ __device__ inline int hermeig_ld(int m) { return m | 1; }
// doubles of LDS per matrix: the planes of A and W | c, s, Re e, Im e of 32 pairs | lambda as found, sorted, clipped |
// partial sums of four wavefronts | the permutation (64 ints) | done, rotated (2 ints)
__host__ __device__ inline size_t hermeig_slot_doubles(int m, bool cplx)
{
    return (size_t)(cplx ? 4 : 2) * m * hermeig_ld(m) + 4 * 32 + 3 * 64 + 4 + 32 + 1;
}

template <int T, bool MAX>
__device__ inline double hermeig_reduce(double x, double* red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double y = __shfl_xor(x, off, 64);
        x = MAX ? fmax(x, y) : x + y;
    }
    if (T > 64) {
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
        __syncthreads();
        x = MAX ? fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) : ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
    return x;
}

__device__ inline void hermeig_pair(int step, int k, int me, int& p, int& q)
{
    const int r = me - 1;
    int a, b;
    if (k == 0) { a = r; b = step; }
    else { a = (step + k) % r; b = (step - k + r) % r; }
    p = min(a, b); q = max(a, b);
}

template <bool C, int T>
__global__ __launch_bounds__(HERMEIG_T)
void hermeig_kernel(const HermEigParams p)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int SLOTS = HERMEIG_T / T;
    extern __shared__ double hermeig_smem[];
    const int m = p.m, ld = hermeig_ld(m), me = (m + 1) & ~1, np = me >> 1, mm = m * m;
    const int tid = threadIdx.x, slot = tid / T, t = tid % T;
    const size_t sd = hermeig_slot_doubles(m, C), plane = (size_t)m * ld;
    double* base = hermeig_smem + slot * sd;
    double* Are = base;
    double* Aim = C ? Are + plane : Are;
    double* Wre = Aim + plane;
    double* Wim = C ? Wre + plane : Wre;
    double* rc = Wim + plane;            // [32]
    double* rs = rc + 32;
    double* rer = rs + 32;
    double* rei = rer + 32;
    double* lam = rei + 32;              // [64] as found on the diagonal
    double* lams = lam + 64;             // [64] ascending
    double* lamc = lams + 64;            // [64] ascending, raised to the floor
    double* red = lamc + 64;             // [4]
    int* perm = (int*)(red + 4);         // [64] perm[r]: the row of W that holds eigenvector r
    int* flag = perm + 64;               // [0] done, [1] a pair rotated in this sweep
    const size_t flag_off = (size_t)(4 * 32 + 3 * 64 + 4 + 32) + (size_t)(C ? 4 : 2) * plane;   // doubles from the slot's base

    const long long mat = (long long)blockIdx.x * SLOTS + slot;
    const bool valid = mat < p.n_mat;                        // (the grid's tail: such a slot is done from the start)
    const size_t g0 = valid ? (size_t)mat * mm : 0;
    const double nan = __builtin_nan("");

    // ---- 1. load, Herm(A), norms ----
    for (int idx = t; idx < mm; idx += T) {
        const int i = idx / m, j = idx - i * m;
        double re = 0.0, im = 0.0;
        if (valid) {
            if (C) { const d2 v = ((const d2*)p.A)[g0 + idx]; re = v.x; im = v.y; }
            else re = p.A[g0 + idx];
        }
        Wre[i * ld + j] = re;
        if (C) Wim[i * ld + j] = im;
    }
    __syncthreads();
    double nbad = 0.0, amax = 0.0, asq = 0.0, pmax = -__builtin_inf();
    for (int idx = t; idx < mm; idx += T) {
        const int i = idx / m, j = idx - i * m;
        const double xr = Wre[i * ld + j], yr = Wre[j * ld + i];
        const double xi = C ? Wim[i * ld + j] : 0.0, yi = C ? Wim[j * ld + i] : 0.0;
        const double hr = 0.5 * (xr + yr), hi = 0.5 * (xi - yi);
        const double dr = xr - yr, di = xi + yi;
        asq += dr * dr + di * di;
        if (!(isfinite(xr) && isfinite(xi))) nbad += 1.0;
        amax = fmax(amax, fmax(fabs(hr), fabs(hi)));
        Are[i * ld + j] = hr;
        if (C) Aim[i * ld + j] = hi;
        if (i < j) {
            const double aii = fmax(Wre[i * ld + i], 0.0), ajj = fmax(Wre[j * ld + j], 0.0);
            const double g = C ? sqrt(hr * hr + hi * hi) : fabs(hr);
            pmax = fmax(pmax, g - sqrt(aii * ajj));
        }
    }
    __syncthreads();
    nbad = hermeig_reduce<T, false>(nbad, red);
    const bool bad = nbad != 0.0;
    amax = hermeig_reduce<T, true>(amax, red);
    asq = hermeig_reduce<T, false>(asq, red);
    pmax = hermeig_reduce<T, true>(pmax, red);
    if (m == 1) pmax = 0.0;                                   // (no pair: nothing to violate)
    double nsq = 0.0;
    {
        const double sc = amax > 0.0 ? 1.0 / amax : 0.0;
        for (int idx = t; idx < mm; idx += T) {
            const int i = idx / m, j = idx - i * m;
            const double hr = Are[i * ld + j] * sc, hi = C ? Aim[i * ld + j] * sc : 0.0;
            nsq += hr * hr + hi * hi;
            Wre[i * ld + j] = i == j ? 1.0 : 0.0;             // (every read of the raw A lies before the barrier above)
            if (C) Wim[i * ld + j] = 0.0;
        }
    }
    nsq = hermeig_reduce<T, false>(nsq, red);
    const double fro = amax * sqrt(nsq);
    const double thresh = fro * 0x1p-53 / (double)m;
    int info = bad ? -1 : -2;                                 // (used by thread 0 of the matrix)
    if (t == 0) { flag[0] = (!valid || bad) ? 1 : 0; flag[1] = 0; }
    __syncthreads();

    // ---- 2. sweeps ----
    for (int sweep = 0; sweep < HERMEIG_MAX_SWEEPS; ++sweep) {
        const bool act = flag[0] == 0;
        for (int step = 0; step < me - 1; ++step) {
            if (t < np) {
                int pp, qq;
                hermeig_pair(step, t, me, pp, qq);
                double c = 1.0, s = 0.0, er = 1.0, ei = 0.0;
                if (act && qq < m) {
                    const double br = Are[pp * ld + qq], bi = C ? Aim[pp * ld + qq] : 0.0;
                    const double g = C ? hypot(br, bi) : fabs(br);
                    if (g > thresh) {
                        const double app = Are[pp * ld + pp], aqq = Are[qq * ld + qq];
                        er = br / g; ei = bi / g;
                        const double tau = (aqq - app) / (2.0 * g);
                        double tt = 1.0 / (fabs(tau) + sqrt(1.0 + tau * tau));
                        if (tau < 0.0) tt = -tt;
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = tt * c;
                        flag[1] = 1;                          // (every writer writes the same value)
                    }
                }
                rc[t] = c; rs[t] = s; rer[t] = er; rei[t] = ei;
            }
            __syncthreads();
            if (act) {
                for (int item = t; item < np * m; item += T) {
                    const int k = item / m, i = item - k * m;
                    const double s = rs[k];
                    if (s == 0.0) continue;
                    int pp, qq;
                    hermeig_pair(step, k, me, pp, qq);
                    const double c = rc[k], er = rer[k], ei = C ? rei[k] : 0.0;
                    const double xpr = Are[i * ld + pp], xqr = Are[i * ld + qq];
                    if (C) {
                        const double xpi = Aim[i * ld + pp], xqi = Aim[i * ld + qq];
                        Are[i * ld + pp] = c * xpr - s * (er * xqr + ei * xqi);
                        Aim[i * ld + pp] = c * xpi - s * (er * xqi - ei * xqr);
                        Are[i * ld + qq] = s * (er * xpr - ei * xpi) + c * xqr;
                        Aim[i * ld + qq] = s * (er * xpi + ei * xpr) + c * xqi;
                    } else {
                        Are[i * ld + pp] = c * xpr - s * (er * xqr);
                        Are[i * ld + qq] = s * (er * xpr) + c * xqr;
                    }
                }
            }
            __syncthreads();
            if (act) {
                for (int item = t; item < np * m; item += T) {
                    const int k = item / m, j = item - k * m;
                    const double s = rs[k];
                    if (s == 0.0) continue;
                    int pp, qq;
                    hermeig_pair(step, k, me, pp, qq);
                    const double c = rc[k], er = rer[k], ei = C ? rei[k] : 0.0;
                    const double ypr = Are[pp * ld + j], yqr = Are[qq * ld + j];
                    const double wpr = Wre[pp * ld + j], wqr = Wre[qq * ld + j];
                    double npr, nqr, npi = 0.0, nqi = 0.0;
                    if (C) {
                        const double ypi = Aim[pp * ld + j], yqi = Aim[qq * ld + j];
                        const double wpi = Wim[pp * ld + j], wqi = Wim[qq * ld + j];
                        npr = c * ypr - s * (er * yqr - ei * yqi);
                        npi = c * ypi - s * (er * yqi + ei * yqr);
                        nqr = s * (er * ypr + ei * ypi) + c * yqr;
                        nqi = s * (er * ypi - ei * ypr) + c * yqi;
                        Wre[pp * ld + j] = c * wpr - s * (er * wqr + ei * wqi);
                        Wim[pp * ld + j] = c * wpi - s * (er * wqi - ei * wqr);
                        Wre[qq * ld + j] = s * (er * wpr - ei * wpi) + c * wqr;
                        Wim[qq * ld + j] = s * (er * wpi + ei * wpr) + c * wqi;
                    } else {
                        npr = c * ypr - s * (er * yqr);
                        nqr = s * (er * ypr) + c * yqr;
                        Wre[pp * ld + j] = c * wpr - s * (er * wqr);
                        Wre[qq * ld + j] = s * (er * wpr) + c * wqr;
                    }
                    if (j == pp) { npi = 0.0; nqr = 0.0; nqi = 0.0; }         // a_pp real, a_qp = 0
                    if (j == qq) { npr = 0.0; npi = 0.0; nqi = 0.0; }         // a_pq = 0, a_qq real
                    Are[pp * ld + j] = npr; Are[qq * ld + j] = nqr;
                    if (C) { Aim[pp * ld + j] = npi; Aim[qq * ld + j] = nqi; }
                }
            }
            __syncthreads();
        }
        if (t == 0) {
            if (act && flag[1] == 0) { flag[0] = 1; info = sweep; }
            flag[1] = 0;
        }
        __syncthreads();
        bool all = true;
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) all = all && ((const int*)(hermeig_smem + sl * sd + flag_off))[0] != 0;
        if (all) break;                                       // (one value for the whole workgroup, read after the barrier)
    }

    // ---- 3. order, normalise ----
    if (t < m) { lam[t] = Are[t * ld + t]; perm[t] = t; }
    __syncthreads();
    if (t < m) {
        const double x = lam[t];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double y = lam[j];
            rank += (y < x || (y == x && j < t)) ? 1 : 0;
        }
        perm[rank] = t;
        lams[rank] = x;
        lamc[rank] = fmax(x, p.floor);
    }
    // E = V^H V - I into the planes of A (its diagonal is in lam): E_pq = sum_i conj(W_pi) W_qi, the upper triangle
    // computed, the lower its conjugate
    for (int idx = t; idx < mm; idx += T) {
        const int pp = idx / m, qq = idx - pp * m;
        if (pp > qq) continue;
        double sr = 0.0, si = 0.0;
        for (int i = 0; i < m; ++i) {
            const double ar = Wre[pp * ld + i], br = Wre[qq * ld + i];
            if (C) {
                const double ai = Wim[pp * ld + i], bi = Wim[qq * ld + i];
                sr += ar * br + ai * bi;
                si += ar * bi - ai * br;
            } else {
                sr += ar * br;
            }
        }
        if (pp == qq) { sr -= 1.0; si = 0.0; }
        Are[pp * ld + qq] = sr; Are[qq * ld + pp] = sr;
        if (C) { Aim[pp * ld + qq] = si; Aim[qq * ld + pp] = -si; }
    }
    __syncthreads();
    // one Newton-Schulz step V <- V (I - E / 2): the rounding of the rotations (every entry of V is touched m - 1 times per
    // sweep) leaves || V^H V - I ||_F at 4 to 10 m 2^-52 for m >= 33; the step brings it below m 2^-52 and leaves the
    // residual as it is (to first order it removes the Hermitian part of V_exact^H dV, which is orthogonal to the rest)
    {
        constexpr int NI = T == 64 ? (HERMEIG_WAVE_M * HERMEIG_WAVE_M + 63) / 64 : (HERMEIG_MAX_M * HERMEIG_MAX_M + 255) / 256;
        double nr[NI], ni[NI];
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const int idx = t + n * T;
            nr[n] = 0.0; ni[n] = 0.0;
            if (idx < mm) {
                const int qq = idx / m, i = idx - qq * m;
                double sr = 0.0, si = 0.0;
                for (int pp = 0; pp < m; ++pp) {
                    const double er = Are[pp * ld + qq], wr = Wre[pp * ld + i];
                    if (C) {
                        const double ei = Aim[pp * ld + qq], wi = Wim[pp * ld + i];
                        sr += er * wr - ei * wi;
                        si += er * wi + ei * wr;
                    } else {
                        sr += er * wr;
                    }
                }
                nr[n] = Wre[qq * ld + i] - 0.5 * sr;
                if (C) ni[n] = Wim[qq * ld + i] - 0.5 * si;
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const int idx = t + n * T;
            if (idx < mm) {
                const int qq = idx / m, i = idx - qq * m;
                Wre[qq * ld + i] = nr[n];
                if (C) Wim[qq * ld + i] = ni[n];
            }
        }
    }
    __syncthreads();
    if (t < m && !bad) {
        const int row = perm[t];
        double best = -1.0, n2 = 0.0;
        int ib = 0;
        for (int i = 0; i < m; ++i) {
            const double wr = Wre[row * ld + i], wi = C ? Wim[row * ld + i] : 0.0;
            const double a2 = wr * wr + wi * wi;
            n2 += a2;
            if (a2 > best) { best = a2; ib = i; }
        }
        if (n2 > 0.0) {
            const double br = Wre[row * ld + ib], bi = C ? Wim[row * ld + ib] : 0.0;
            const double ab = C ? sqrt(br * br + bi * bi) : fabs(br);
            const double sc = 1.0 / sqrt(n2);
            const double fr = br / ab * sc, fi = -bi / ab * sc;          // conj(w_b) / |w_b| / || w ||
            for (int i = 0; i < m; ++i) {
                const double wr = Wre[row * ld + i];
                if (C) {
                    const double wi = Wim[row * ld + i];
                    Wre[row * ld + i] = wr * fr - wi * fi;
                    Wim[row * ld + i] = wr * fi + wi * fr;
                } else {
                    Wre[row * ld + i] = wr * fr;
                }
            }
            Wre[row * ld + ib] = ab * sc;
            if (C) Wim[row * ld + ib] = 0.0;
        }
    }
    __syncthreads();

    // ---- 4. projection (into the planes of A), outputs ----
    for (int idx = t; idx < mm; idx += T) {
        const int i = idx / m, j = idx - i * m;
        if (i > j) continue;
        double sr = 0.0, si = 0.0;
        for (int r = 0; r < m; ++r) {
            const int row = perm[r];
            const double l = lamc[r];
            const double ar = Wre[row * ld + i], br = Wre[row * ld + j];
            if (C) {
                const double ai = Wim[row * ld + i], bi = Wim[row * ld + j];
                sr += l * (ar * br + ai * bi);
                si += l * (ai * br - ar * bi);
            } else {
                sr += l * (ar * br);
            }
        }
        if (i == j) si = 0.0;
        Are[i * ld + j] = sr; Are[j * ld + i] = sr;
        if (C) { Aim[i * ld + j] = si; Aim[j * ld + i] = -si; }
    }
    __syncthreads();
    if (!valid) return;                                       // (no barrier follows)
    if (t == 0) {
        double sn = 0.0, sq = 0.0;
        for (int r = 0; r < m; ++r) {
            const double d = p.floor - lams[r];
            if (d > 0.0) { sn += d; sq += d * d; }
        }
        if (p.neg) p.neg[mat] = bad ? nan : sn;
        if (p.dist) p.dist[mat] = bad ? nan : sqrt(sq);
        if (p.pair) p.pair[mat] = bad ? nan : pmax;
        if (p.asym) p.asym[mat] = bad ? nan : sqrt(asq);
        if (p.info) p.info[mat] = info;
    }
    if (p.lambda && t < m) p.lambda[(size_t)mat * m + t] = bad ? nan : lams[t];
    if (p.vec) {
        for (int idx = t; idx < mm; idx += T) {
            const int i = idx / m, r = idx - i * m;
            const int row = perm[r];
            if (C) {
                d2 v; v.x = bad ? nan : Wre[row * ld + i]; v.y = bad ? nan : Wim[row * ld + i];
                ((d2*)p.vec)[g0 + idx] = v;
            } else {
                p.vec[g0 + idx] = bad ? nan : Wre[row * ld + i];
            }
        }
    }
    if (p.proj) {
        if (C) {
            for (int idx = t; idx < mm; idx += T) {
                const int i = idx / m, j = idx - i * m;
                d2 v; v.x = bad ? nan : Are[i * ld + j]; v.y = bad ? nan : Aim[i * ld + j];
                ((d2*)p.proj)[g0 + idx] = v;
            }
        } else if ((mm & 1) == 0) {
            for (int u = t; 2 * u < mm; u += T) {
                const int i0 = (2 * u) / m, j0 = 2 * u - i0 * m, i1 = (2 * u + 1) / m, j1 = 2 * u + 1 - i1 * m;
                d2 v; v.x = bad ? nan : Are[i0 * ld + j0]; v.y = bad ? nan : Are[i1 * ld + j1];
                ((d2*)(p.proj + g0))[u] = v;
            }
        } else {
            for (int idx = t; idx < mm; idx += T) {
                const int i = idx / m, j = idx - i * m;
                p.proj[g0 + idx] = bad ? nan : Are[i * ld + j];
            }
        }
    }
}

} // namespace mxe
