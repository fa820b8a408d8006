// mxe_evidence.hip.h -- default-model scans: evidence of a scan, model averages of a group of scans (no counterpart in
// the reference, whose users loop run() over their default models)
//
//   log p(alpha, D | G) of every alpha of a scan, its H rows  ->  log Z, weights over alpha, ONE row   evidence_scan_kernel
//   the rows and log Z of the scans of a group                ->  weights of the models, mean, spread   evidence_group_kernel
//
// evidence_scan_kernel: one workgroup (4 wavefronts) per scan -- the streaming part, n_alpha x n_omega doubles per scan.
//   1. which alphas are good (a finite logp), the largest exponents (a maximum: exact in any order) and kmax, the first
//      index of the largest logp; the terms exp(x_k - m) go through LDS in tiles of 256 and ONE thread adds them in k
//      order; the weights over alpha are the same terms over that sum.
//   2. row_mode 0: lanes over omega (two neighbouring points per lane, one 16-byte load where the rows are aligned, 8-byte
//      loads else: the arithmetic per point is the same), the rows in k order, row = sum_k walpha_k H_k by one fma per row
//      and point.  The sweep also tells which rows are not finite.  If one of them had a finite logp it is struck from
//      the good alphas and steps 1 and 2 run once more: the maximum may have been its exponent.  The second sweep is the
//      final one -- every row with a finite logp was looked at in the first.
//      row_mode 1, 2: the row at kmax, at pick[s]; only that row is read.
//   3. a scan with no good alpha, a chosen row that is not finite or a negative pick is unusable: log Z = -inf, NaN row.
//      Functional values F row: one wavefront per functional, lanes over omega, butterfly sum (fixed order).
// evidence_group_kernel: one workgroup per group over the rows the first kernel wrote, launched behind it on the stream.
//   u_s = softmax of log Z_s + log prior_s over the usable scans (maximum subtracted, terms added in s order by one
//   thread), then per omega point one thread: mean = sum_s u_s row_s in s order, between = sum_s u_s (row_s - mean)^2 in a
//   second pass on the explicit difference; the same for the functional values and their covariance.
// No atomics, no sum whose order depends on the launch: a scan's bits depend on its own rows, a group's on its own scans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mxe_bins.hip.h"

namespace mxe {

constexpr int EV_T = 256;                // threads of a workgroup of both kernels
constexpr double EV_DBL_MAX = 1.79769313486231570815e308;

struct EvidenceParams {
    const double* H;         // rows of nw values; scan s owns the n_alpha rows from row0[s]
    const long long* row0;   // [n_scan]
    const double* logp;      // [n_scan][n_alpha]
    const double* log_quad;  // [n_alpha]
    const double* log_mix;   // [n_alpha]
    const double* log_prior; // [n_scan]
    const int* pick;         // [n_scan] (row_mode 2)
    const int* off;          // [n_groups + 1]
    const double* F;         // [n_f][nw], unused with n_f == 0
    int n_alpha, nw, n_f, row_mode;
    int* good;               // [n_scan][n_alpha]  scratch: 1 where the alpha is good
    int* usable;             // [n_scan]
    double* logZ;            // [n_scan]
    int* kmax;               // [n_scan]
    int* ngood;              // [n_scan]
    double* walpha;          // [n_scan][n_alpha]
    double* row;             // [n_scan][nw]
    double* fval;            // [n_scan][n_f]
    double* wmodel;          // [n_scan]
    double* mean;            // [n_groups][nw]
    double* between;         // [n_groups][nw]
    double* fmean;           // [n_groups][n_f]
    double* fcov;            // [n_groups][n_f][n_f]
    int* used;               // [n_groups]
};

__device__ __forceinline__ bool ev_finite(double x) { return fabs(x) <= EV_DBL_MAX; }

// the maximum of x over the workgroup (exact: the order does not matter); red: EV_T doubles of LDS
__device__ __forceinline__ double ev_block_max(double x, double* red, int tid)
{
    red[tid] = x;
    __syncthreads();
    for (int o = EV_T / 2; o > 0; o >>= 1) {
        if (tid < o) { const double y = red[tid + o]; if (y > red[tid]) red[tid] = y; }
        __syncthreads();
    }
    const double m = red[0];
    __syncthreads();
    return m;
}

// sum over the n entries of exp(x_k - m), x_k = a[k] + b[k] where flag[k] (b == nullptr: x_k = a[k]), added in k order by thread 0
__device__ __forceinline__ double ev_ordered_expsum(const double* a, const double* b, const int* flag, int n, double m,
                                                    double* red, int tid)
{
    double s = 0.0;
    for (int k0 = 0; k0 < n; k0 += EV_T) {
        const int k = k0 + tid;
        red[tid] = (k < n && flag[k]) ? exp(a[k] + (b ? b[k] : 0.0) - m) : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int kn = min(EV_T, n - k0);
            for (int q = 0; q < kn; ++q) s += red[q];        // (an entry without the flag holds 0: s stays as it is)
        }
        __syncthreads();
    }
    if (tid == 0) red[0] = s;
    __syncthreads();
    s = red[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(EV_T)
void evidence_scan_kernel(const EvidenceParams p)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = p.n_alpha, nw = p.nw, n_f = p.n_f, mode = p.row_mode;
    const double* logp = p.logp + (size_t)s * na;
    const double* H = p.H + (size_t)p.row0[s] * nw;
    int* good = p.good + (size_t)s * na;
    double* walpha = p.walpha + (size_t)s * na;
    double* row = p.row + (size_t)s * nw;
    const double nan = __builtin_nan("");
    const double ninf = -__builtin_inf();
    // (one 16-byte load per lane where every row starts on 16 bytes)
    const bool vec = ((nw & 1) == 0) && ((((uintptr_t)H) & 15) == 0);

    __shared__ double red[EV_T];
    __shared__ int ired[EV_T];
    __shared__ double wt[EV_T];          // the weights and flags of a tile of alphas
    __shared__ int gd[EV_T];
    __shared__ int flag[2];              // [0]: a good alpha's row is not finite; [1]: the chosen row is not finite

    for (int k = tid; k < na; k += EV_T) good[k] = ev_finite(logp[k]) ? 1 : 0;
    if (tid < 2) flag[tid] = 0;
    __syncthreads();

    int n_good = 0, kbest = -1;
    double logZ = ninf;
    for (int sweep = 0; sweep < 2; ++sweep) {
        // ---- 1. maxima, kmax, log Z, weights over alpha ----
        double mq = ninf, mm = ninf, ml = ninf;
        int kl = 0x7fffffff, cnt = 0;
        for (int k = tid; k < na; k += EV_T)
            if (good[k]) {
                const double l = logp[k];
                mq = fmax(mq, l + p.log_quad[k]);
                mm = fmax(mm, l + p.log_mix[k]);
                if (l > ml) { ml = l; kl = k; }          // (k ascends: the first index of a thread's largest)
                ++cnt;
            }
        mq = ev_block_max(mq, red, tid);
        mm = ev_block_max(mm, red, tid);
        const double mlb = ev_block_max(ml, red, tid);
        ired[tid] = (cnt > 0 && ml == mlb) ? kl : 0x7fffffff;
        __syncthreads();
        for (int o = EV_T / 2; o > 0; o >>= 1) {
            if (tid < o) ired[tid] = min(ired[tid], ired[tid + o]);
            __syncthreads();
        }
        kbest = (ired[0] == 0x7fffffff) ? -1 : ired[0];
        __syncthreads();
        ired[tid] = cnt;
        __syncthreads();
        for (int o = EV_T / 2; o > 0; o >>= 1) {
            if (tid < o) ired[tid] += ired[tid + o];
            __syncthreads();
        }
        n_good = ired[0];
        __syncthreads();
        if (n_good > 0) {
            const double sq = ev_ordered_expsum(logp, p.log_quad, good, na, mq, red, tid);
            const double sm = ev_ordered_expsum(logp, p.log_mix, good, na, mm, red, tid);
            logZ = mq + log(sq);
            for (int k = tid; k < na; k += EV_T) walpha[k] = good[k] ? exp(logp[k] + p.log_mix[k] - mm) / sm : 0.0;
        } else {
            logZ = ninf;
            for (int k = tid; k < na; k += EV_T) walpha[k] = 0.0;
        }
        __syncthreads();                                 // (walpha is read below by other threads)
        if (mode != 0 || n_good == 0) break;

        // ---- 2. row = sum_k walpha_k H_k, the rows in k order; which rows are not finite ----
        // An alpha that is not good reads the row at kmax instead, with the weight 0: the loop has no branch on k.
        for (int c0 = 0; c0 < nw; c0 += 2 * EV_T) {
            const int i0 = c0 + 2 * tid;
            const bool act = i0 < nw, two = i0 + 1 < nw;
            double a0 = 0.0, a1 = 0.0;
            for (int k0 = 0; k0 < na; k0 += EV_T) {
                __syncthreads();                         // (the tile before this one has been used)
                if (k0 + tid < na) { wt[tid] = walpha[k0 + tid]; gd[tid] = good[k0 + tid] != 0; }
                __syncthreads();
                const int kn = min(EV_T, na - k0);
                if (act) {
#pragma unroll 4
                    for (int q = 0; q < kn; ++q) {
                        const int k = gd[q] ? k0 + q : kbest;
                        const double* h = H + (size_t)k * nw + i0;
                        double h0, h1;
                        if (vec) { const d2 v = *reinterpret_cast<const d2*>(h); h0 = v.x; h1 = v.y; }
                        else { h0 = h[0]; h1 = two ? h[1] : 0.0; }
                        if (!(ev_finite(h0) && ev_finite(h1))) good[k] = 2;        // (2: struck after this sweep)
                        const double w = wt[q];
                        a0 = fma(w, h0, a0);
                        a1 = fma(w, h1, a1);
                    }
                }
            }
            if (act) {
                row[i0] = a0;
                if (two) row[i0 + 1] = a1;
            }
        }
        __syncthreads();
        int struck = 0;
        for (int k = tid; k < na; k += EV_T) if (good[k] == 2) { good[k] = 0; struck = 1; }
        if (struck) flag[0] = 1;
        __syncthreads();
        if (!flag[0]) break;                             // (the same for every thread: LDS, read behind the barrier)
        __syncthreads();
        if (tid == 0) flag[0] = 0;
        __syncthreads();
    }

    // ---- 3. the chosen row of modes 1 and 2, is the scan usable, functional values ----
    int ksel = -1;
    if (mode == 1) ksel = kbest;
    if (mode == 2) ksel = p.pick[s];
    if (mode != 0 && ksel >= 0 && n_good > 0)
        for (int i = tid; i < nw; i += EV_T) row[i] = H[(size_t)ksel * nw + i];
    __syncthreads();
    bool ok = n_good > 0 && (mode == 0 || ksel >= 0);
    if (ok) {
        int bad = 0;
        for (int i = tid; i < nw; i += EV_T) if (!ev_finite(row[i])) bad = 1;
        if (bad) flag[1] = 1;
    }
    __syncthreads();
    ok = ok && !flag[1];
    if (!ok) {
        for (int i = tid; i < nw; i += EV_T) row[i] = nan;
        for (int f = tid; f < n_f; f += EV_T) p.fval[(size_t)s * n_f + f] = nan;
        logZ = ninf;
    } else {
        for (int f = wave; f < n_f; f += EV_T / 64) {
            const double* Ff = p.F + (size_t)f * nw;
            double t = 0.0;
            for (int i = lane; i < nw; i += 64) t = fma(Ff[i], row[i], t);
            t = bins_wave_sum(t);
            if (lane == 0) p.fval[(size_t)s * n_f + f] = t;
        }
    }
    if (tid == 0) {
        p.logZ[s] = logZ;
        p.kmax[s] = kbest;
        p.ngood[s] = n_good;
        p.usable[s] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(EV_T)
void evidence_group_kernel(const EvidenceParams p)
{
    const int g = blockIdx.x;
    const int tid = threadIdx.x;
    const int nw = p.nw, n_f = p.n_f;
    const int s0 = p.off[g], s1 = p.off[g + 1], ns = s1 - s0;
    const int* usable = p.usable + s0;
    const double ninf = -__builtin_inf();
    const double nan = __builtin_nan("");

    __shared__ double red[EV_T];
    __shared__ int ired[EV_T];

    // ---- weights of the models: softmax of log Z + log prior over the usable scans ----
    double m = ninf;
    int cnt = 0;
    for (int q = tid; q < ns; q += EV_T)
        if (usable[q]) { m = fmax(m, p.logZ[s0 + q] + p.log_prior[s0 + q]); ++cnt; }
    m = ev_block_max(m, red, tid);
    ired[tid] = cnt;
    __syncthreads();
    for (int o = EV_T / 2; o > 0; o >>= 1) {
        if (tid < o) ired[tid] += ired[tid + o];
        __syncthreads();
    }
    const int nu = ired[0];
    __syncthreads();
    double* wmodel = p.wmodel + s0;
    if (nu > 0) {
        const double sum = ev_ordered_expsum(p.logZ + s0, p.log_prior + s0, usable, ns, m, red, tid);
        for (int q = tid; q < ns; q += EV_T)
            wmodel[q] = usable[q] ? exp(p.logZ[s0 + q] + p.log_prior[s0 + q] - m) / sum : 0.0;
    } else {
        for (int q = tid; q < ns; q += EV_T) wmodel[q] = 0.0;
    }
    __syncthreads();

    // ---- mean and spread between the models, in s order ----
    for (int i = tid; i < nw; i += EV_T) {
        double mean = nan, b = nan;
        if (nu > 0) {
            mean = 0.0;
            for (int q = 0; q < ns; ++q)
                if (usable[q]) mean = fma(wmodel[q], p.row[(size_t)(s0 + q) * nw + i], mean);
            b = 0.0;
            for (int q = 0; q < ns; ++q)
                if (usable[q]) { const double d = p.row[(size_t)(s0 + q) * nw + i] - mean; b = fma(wmodel[q], d * d, b); }
        }
        p.mean[(size_t)g * nw + i] = mean;
        p.between[(size_t)g * nw + i] = b;
    }
    double* fmean = p.fmean + (size_t)g * n_f;
    for (int f = tid; f < n_f; f += EV_T) {
        double t = nan;
        if (nu > 0) {
            t = 0.0;
            for (int q = 0; q < ns; ++q)
                if (usable[q]) t = fma(wmodel[q], p.fval[(size_t)(s0 + q) * n_f + f], t);
        }
        fmean[f] = t;
    }
    __syncthreads();
    for (int idx = tid; idx < n_f * n_f; idx += EV_T) {
        const int f1 = idx / n_f, f2 = idx - f1 * n_f;
        double c = nan;
        if (nu > 0) {
            const double m1 = fmean[f1], m2 = fmean[f2];
            c = 0.0;
            for (int q = 0; q < ns; ++q)
                if (usable[q])
                    c = fma(wmodel[q], (p.fval[(size_t)(s0 + q) * n_f + f1] - m1) * (p.fval[(size_t)(s0 + q) * n_f + f2] - m2), c);
        }
        p.fcov[((size_t)g * n_f + f1) * n_f + f2] = c;
    }
    if (tid == 0) p.used[g] = nu;
}

} // namespace mxe
