// micro-test of two instruction savings tried on the lock-step round, one shipped and one measured and dropped
// (profiles/r06_experiments.txt):
//  1. gj2_solve64_f32 (mxe_kernel.hip.h) with the packed trailing update against the scalar one, N = 16 .. 32: the same bits.
//  2. (dropped: 0.834 -> 0.883 ms per step -- v_fma_mix{lo,hi}_f16 cost more issue time than the 2.5 instructions per value they
//     replace; kept here as the record of its accuracy) the operand split of the Gram tiles, x = v s as two binary16 numbers, by
//     two v_fma_mix{lo,hi}_f16 per value (split_f16 below) against the sequence of the kernels (product rounded to binary32,
//     v_cvt_pkrtz_f16_f32, v_fma_mix_f32, v_cvt_pkrtz_f16_f32: split_before below): hi + lo against the binary64 product on a fixed
//     list, and the Gram entries hi hi + hi lo + lo hi of 32 x 32 blocks through v_mfma_f32_16x16x32_f16 as the kernels form them.
// Prints "key value" lines (tests/test_gpu_gj_packed.py reads the solve_* ones); exit status 0 unless a HIP call failed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/split_check.hip -o tools/split_check && tools/split_check
#include "../maxent_amd/csrc/mxe_kernel.hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <random>

using namespace mxe;

#define CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); exit(2); } } while (0)

// the split that was tried: hi = binary16(v s) in one v_fma_mix{lo,hi}_f16 (binary32 x binary32 + 0), lo = binary16(v s - hi) in one
// more with the half just written as its third source; rounds to nearest, so |x| >= 65520 becomes an infinity where the conversion
// towards zero saturates -- the kernels would have to bound sw at its source (gram_sw)
template <bool ODD>
__device__ __forceinline__ void split_f16(float v, float s, unsigned& xh, unsigned& xl)
{
    if constexpr (!ODD) {
        asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(xh) : "v"(v), "v"(s));
        asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(xl) : "v"(v), "v"(s), "v"(xh));
    } else {
        asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(xh) : "v"(v), "v"(s));
        asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(xl) : "v"(v), "v"(s), "v"(xh));
    }
}
__device__ __forceinline__ float gram_sw(float w_scaled) { return __builtin_sqrtf(fminf(w_scaled, 4.0e9f)); }     // sqrt: 63245.6 < 65504

// the split of the kernels: the pair (x0, x1) of binary32 products -> packed hi, packed lo, both rounded towards zero
__device__ __forceinline__ void split_before(float x0, float x1, unsigned& xh, unsigned& xl)
{
    const auto hh = __builtin_amdgcn_cvt_pkrtz(x0, x1);
    const unsigned hu = __builtin_bit_cast(unsigned, hh);
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hu), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hu), "v"(x1));
    xh = hu;
    xl = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(l0, l1));
}

// values 2 p and 2 p + 1 of the list share a register pair, as an even and an odd row group do; out: hi | lo packed, new and before
__global__ void k_split(const float* __restrict__ v, const float* __restrict__ s, int n_pairs, unsigned* __restrict__ out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const float v0 = v[2 * p], v1 = v[2 * p + 1], s0 = s[2 * p], s1 = s[2 * p + 1];
    unsigned h, l;
    split_f16<false>(v0, s0, h, l);
    split_f16<true>(v1, s1, h, l);
    unsigned bh, bl;
    split_before(v0 * s0, v1 * s1, bh, bl);
    out[4 * p + 0] = h; out[4 * p + 1] = l; out[4 * p + 2] = bh; out[4 * p + 3] = bl;
}

// the bound of the row pass: sw = gram_sw(w sc2)
__global__ void k_sw(const float* __restrict__ w, int n, float* __restrict__ sw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sw[i] = gram_sw(w[i]);
}

// W = X^T X of a K x 32 block X = diag(s) V (K a multiple of 32) on one wave, as the fused pass does it: lane (g, m) holds of
// column 16 t + m the rows 32 ks + 8 g + e, e = 0 .. 7; three products per tile.  W: 32 x 32, row-major.
template <bool NEW>
__global__ void k_gram(const float* __restrict__ V, const float* __restrict__ s, int K, float* __restrict__ W)
{
    typedef float g4 __attribute__((ext_vector_type(4)));
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    g4 acc[3] = {g4{0, 0, 0, 0}, g4{0, 0, 0, 0}, g4{0, 0, 0, 0}};
    for (int ks = 0; ks < K / 32; ++ks) {
        u4v xh[2], xl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
                const int k0 = 32 * ks + 8 * g + 2 * e2;
                const float v0 = V[k0 * 32 + 16 * t + m], v1 = V[(k0 + 1) * 32 + 16 * t + m];
                unsigned h, l;
                if (NEW) { split_f16<false>(v0, s[k0], h, l); split_f16<true>(v1, s[k0 + 1], h, l); }
                else split_before(v0 * s[k0], v1 * s[k0 + 1], h, l);
                xh[t][e2] = h; xl[t][e2] = l;
            }
#pragma unroll
        for (int prod = 0; prod < 3; ++prod) {
            int pr = 0;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = mt; nt < 2; ++nt) {
                    const h8 a = __builtin_bit_cast(h8, prod == 2 ? xl[mt] : xh[mt]);
                    const h8 b = __builtin_bit_cast(h8, prod == 1 ? xl[nt] : xh[nt]);
                    acc[pr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[pr], 0, 0, 0);
                    ++pr;
                }
        }
    }
    // accumulator register r of lane (g, m): row 4 g + r, column m of the tile
    const int mt_of[3] = {0, 0, 1}, nt_of[3] = {0, 1, 1};
    for (int pr = 0; pr < 3; ++pr)
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * mt_of[pr] + 4 * g + r, j = 16 * nt_of[pr] + m;
            W[i * 32 + j] = acc[pr][r];
            W[j * 32 + i] = acc[pr][r];          // (the tile (1, 0) is the transpose; on the diagonal tiles the same value twice over)
        }
}

template <int N, bool PK>
__global__ void k_solve(const float* __restrict__ M, const float* __restrict__ rhs, float* __restrict__ z)
{
    const int lane = threadIdx.x & 63, sys = blockIdx.x;
    const int i = lane & 31, h = lane >> 5;
    const float* Ms = M + (size_t)sys * 32 * 32;
    float A[N / 2];
    for (int kk = 0; kk < N / 2; ++kk) A[kk] = (i < N) ? Ms[i * 32 + 2 * kk + h] : ((2 * kk + h) == i ? 1.0f : 0.0f);
    const float b = (i < N) ? rhs[sys * 32 + i] : 0.0f;
    float zz = 0.0f;
    bool small;
    gj2_solve64_f32<N, PK>(A, b, i, zz, small);
    if (h == 0) z[sys * 32 + i] = (i < N) ? zz : 0.0f;
}

static double half_bits_to_double(unsigned short b)
{
    const int sign = b >> 15, ex = (b >> 10) & 31, man = b & 1023;
    double x;
    if (ex == 31) x = man ? NAN : INFINITY;
    else if (ex == 0) x = std::ldexp((double)man, -24);
    else x = std::ldexp((double)(1024 + man), ex - 25);
    return sign ? -x : x;
}

template <int N>
static int solve_mismatches(const float* dM, const float* dr, float* dz, int n_sys, double* worst_res, const std::vector<float>& M, const std::vector<float>& rhs)
{
    std::vector<float> za(n_sys * 32), zb(n_sys * 32);
    CHK(hipMemset(dz, 0, n_sys * 32 * 4));
    k_solve<N, true><<<n_sys, 64>>>(dM, dr, dz);
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(za.data(), dz, za.size() * 4, hipMemcpyDeviceToHost));
    CHK(hipMemset(dz, 0, n_sys * 32 * 4));
    k_solve<N, false><<<n_sys, 64>>>(dM, dr, dz);
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(zb.data(), dz, zb.size() * 4, hipMemcpyDeviceToHost));
    int bad = 0;
    for (size_t q = 0; q < za.size(); ++q) if (std::memcmp(&za[q], &zb[q], 4) != 0) ++bad;
    // (that the solve solves at all: residual of the leading N x N block against the right-hand side)
    double w = 0.0;
    for (int s = 0; s < n_sys; ++s) {
        double num = 0, den = 0;
        for (int i = 0; i < N; ++i) {
            double a = 0;
            for (int j = 0; j < N; ++j) a += (double)M[(size_t)s * 1024 + i * 32 + j] * za[s * 32 + j];
            num += (a - rhs[s * 32 + i]) * (a - rhs[s * 32 + i]); den += (double)rhs[s * 32 + i] * rhs[s * 32 + i];
        }
        w = std::max(w, std::sqrt(num / den));
    }
    *worst_res = w;
    return bad;
}

int main()
{
    // ---- 1. the fixed list of (v, s): index ranges [first, last) of its groups ----
    std::vector<float> v, s;
    auto add = [&](double vv, double ss) { v.push_back((float)vv); s.push_back((float)ss); };
    std::mt19937 rng(20);
    std::uniform_real_distribution<double> un(0.0, 1.0);
    // normal values across the scaled range: |v| <= 1 of either sign, sw in (2^-8, 16], products down to 2^-10
    const int n_normal = 8192;
    for (int q = 0; q < n_normal; ++q) {
        const double ss = 16.0 * std::exp2(-12.0 * un(rng));
        double vv = (2.0 * un(rng) - 1.0);
        if (std::fabs(vv * ss) < std::exp2(-10.0)) vv = std::copysign(std::exp2(-10.0) / ss * (1.0 + un(rng)), vv);
        add(vv, ss);
    }
    const int first_special = (int)v.size();
    add(0.0, 3.0); add(-0.0, 5.0); add(0.25, 0.0); add(-1.0, 16.0);              // zero and negative V, zero sw
    add(1.0, 16.0); add(-0.999999940395, 15.9999990463);
    add(1.0, 65504.0);                                                          // the largest finite operand
    add(-1.0, 65504.0);
    const int first_sub = (int)v.size();
    for (int q = 0; q < 1024; ++q) {                                            // products in the binary16 subnormal range (< 2^-14)
        const double x = std::exp2(-14.0 - 10.0 * un(rng)) * (q & 1 ? -1.0 : 1.0);
        const double ss = 16.0 * std::exp2(-12.0 * un(rng));
        add(x / ss, ss);
    }
    const int first_over = (int)v.size();
    add(1.0, 65536.0); add(1.0, 65519.0);                                       // beyond the largest: the raw split (reported, not bounded)
    add(-1.0, 1.0e6); add(1.0, 65520.0);
    const int n_val = (int)v.size();                                            // (even)
    float *dv, *ds; unsigned* dout;
    CHK(hipMalloc(&dv, n_val * 4)); CHK(hipMalloc(&ds, n_val * 4)); CHK(hipMalloc(&dout, (size_t)n_val * 2 * 4));
    CHK(hipMemcpy(dv, v.data(), n_val * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(ds, s.data(), n_val * 4, hipMemcpyHostToDevice));
    k_split<<<(n_val / 2 + 63) / 64, 64>>>(dv, ds, n_val / 2, dout);
    CHK(hipDeviceSynchronize());
    std::vector<unsigned> out((size_t)n_val * 2);
    CHK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    auto part = [&](int q, int which) {          // which: 0 hi, 1 lo, 2 hi before, 3 lo before
        const unsigned w = out[4 * (q >> 1) + which];
        return half_bits_to_double((unsigned short)((q & 1) ? (w >> 16) : (w & 0xffff)));
    };
    // rel_big: over the values with |x| >= 2^-3, whose remainder (>= 2^-11 of x: 2^-14) is a normal binary16 number -- below, the
    // remainder is rounded to a multiple of 2^-24 and the error is absolute
    struct Err { double rel = 0, rel_big = 0, abs = 0; int nonfinite = 0; };
    auto group = [&](int a, int b, int which) {
        Err e;
        for (int q = a; q < b; ++q) {
            const double x = (double)v[q] * (double)s[q], got = part(q, which) + part(q, which + 1);
            if (!std::isfinite(got)) { ++e.nonfinite; continue; }
            e.abs = std::max(e.abs, std::fabs(got - x));
            if (x != 0.0) e.rel = std::max(e.rel, std::fabs(got - x) / std::fabs(x));
            if (std::fabs(x) >= 0.125) e.rel_big = std::max(e.rel_big, std::fabs(got - x) / std::fabs(x));
            else if (got != 0.0) e.rel = INFINITY;
        }
        return e;
    };
    const char* names[3] = {"normal", "special", "subnormal"};
    const int lim[4] = {0, first_special, first_sub, first_over};
    for (int gq = 0; gq < 3; ++gq) {
        const Err en = group(lim[gq], lim[gq + 1], 0), eb = group(lim[gq], lim[gq + 1], 2);
        printf("split_%s_n %d\n", names[gq], lim[gq + 1] - lim[gq]);
        printf("split_%s_rel_new %.6e\nsplit_%s_rel_before %.6e\n", names[gq], en.rel, names[gq], eb.rel);
        printf("split_%s_relbig_new %.6e\nsplit_%s_relbig_before %.6e\n", names[gq], en.rel_big, names[gq], eb.rel_big);
        printf("split_%s_abs_new %.6e\nsplit_%s_abs_before %.6e\n", names[gq], en.abs, names[gq], eb.abs);
        printf("split_%s_nonfinite_new %d\nsplit_%s_nonfinite_before %d\n", names[gq], en.nonfinite, names[gq], eb.nonfinite);
    }
    {
        const Err en = group(first_over, n_val, 0), eb = group(first_over, n_val, 2);
        printf("split_over_n %d\nsplit_over_nonfinite_new %d\nsplit_over_nonfinite_before %d\n", n_val - first_over, en.nonfinite, eb.nonfinite);
    }
    // the same overflow through the bound of the row pass: sw = gram_sw(w sc2), |v| <= 1
    {
        const float wl[8] = {4.2949673e9f /* 65536^2 */, 1.0e10f, 3.0e38f, INFINITY, 4.2907740e9f /* 65504^2 */, 1.0e12f, NAN, 256.0f};
        float* dw; float* dsw;
        CHK(hipMalloc(&dw, 32)); CHK(hipMalloc(&dsw, 32));
        CHK(hipMemcpy(dw, wl, 32, hipMemcpyHostToDevice));
        k_sw<<<1, 64>>>(dw, 8, dsw);
        CHK(hipDeviceSynchronize());
        float swl[8];
        CHK(hipMemcpy(swl, dsw, 32, hipMemcpyDeviceToHost));
        std::vector<float> v2(16), s2(16);
        for (int q = 0; q < 8; ++q) { v2[2 * q] = 1.0f; v2[2 * q + 1] = -1.0f; s2[2 * q] = s2[2 * q + 1] = swl[q]; }
        CHK(hipMemcpy(dv, v2.data(), 64, hipMemcpyHostToDevice)); CHK(hipMemcpy(ds, s2.data(), 64, hipMemcpyHostToDevice));
        k_split<<<1, 64>>>(dv, ds, 8, dout);
        CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(out.data(), dout, 8 * 4 * 4, hipMemcpyDeviceToHost));
        int nonfinite = 0; double rel = 0, sw_max = 0;
        for (int q = 0; q < 16; ++q) {
            const double x = (double)v2[q] * (double)s2[q], got = part(q, 0) + part(q, 1);
            if (!std::isfinite(got) || !std::isfinite(x)) { ++nonfinite; continue; }
            rel = std::max(rel, std::fabs(got - x) / std::fabs(x));
            sw_max = std::max(sw_max, std::fabs(x));
        }
        printf("bounded_n 16\nbounded_nonfinite_new %d\nbounded_rel_new %.6e\nbounded_sw_max %.6f\nbounded_sw_of_256 %.6f\n", nonfinite, rel, sw_max, swl[7]);
        CHK(hipFree(dw)); CHK(hipFree(dsw));
    }
    // ---- the Gram entries of a 32 x 32 block, K = 256 rows ----
    // "kernel": operands as the lock-step kernels form them: V with ORTHONORMAL columns (entries ~ K^-1/2) and sw = sqrt(w sc2) of a spectrum -- two peaks
    //   on a background eight decades below -- with sc2 = 2^(8 - exponent of the largest w), the scale the home section sets.
    // "wide": a block outside that class -- columns of independent entries up to 1, decaying twelvefold across the block,
    //   sw over four decades: most products lie where the remainder is a binary16 subnormal (absolute error 2^-25 per operand, 2^-24
    //   before) and the small columns carry it against a small sqrt(W_ii W_jj).
    for (int block = 0; block < 2; ++block) {
        const int K = 256;
        std::vector<float> V(K * 32), sw(K);
        if (block == 0) {
            std::vector<double> Q(K * 32);
            std::normal_distribution<double> nd;
            for (auto& q : Q) q = nd(rng);
            for (int c = 0; c < 32; ++c)                          // modified Gram-Schmidt, twice
                for (int pass = 0; pass < 2; ++pass) {
                    for (int b2 = 0; b2 < c; ++b2) {
                        double d = 0;
                        for (int k = 0; k < K; ++k) d += Q[k * 32 + c] * Q[k * 32 + b2];
                        for (int k = 0; k < K; ++k) Q[k * 32 + c] -= d * Q[k * 32 + b2];
                    }
                    double n2 = 0;
                    for (int k = 0; k < K; ++k) n2 += Q[k * 32 + c] * Q[k * 32 + c];
                    for (int k = 0; k < K; ++k) Q[k * 32 + c] /= std::sqrt(n2);
                }
            for (int q = 0; q < K * 32; ++q) V[q] = (float)Q[q];
            std::vector<double> w(K);
            double wmax = 0;
            for (int k = 0; k < K; ++k) {
                const double om = -5.0 + 10.0 * k / (K - 1);
                w[k] = 0.5 * std::exp(-0.5 * (om + 1.5) * (om + 1.5) / 0.25) / std::sqrt(2 * M_PI * 0.25)
                     + 0.5 * std::exp(-0.5 * (om - 1.0) * (om - 1.0) / 0.64) / std::sqrt(2 * M_PI * 0.64) + 1e-8;
                w[k] *= 10.0 / (K - 1);
                wmax = std::max(wmax, w[k]);
            }
            const double sc2 = std::ldexp(1.0, 8 - std::ilogb(wmax));
            for (int k = 0; k < K; ++k) sw[k] = std::sqrt((float)(w[k] * sc2));
        } else {
            for (int k = 0; k < K; ++k) {
                sw[k] = (float)(16.0 * std::exp2(-13.0 * un(rng)));
                for (int c = 0; c < 32; ++c) V[k * 32 + c] = (float)((2.0 * un(rng) - 1.0) * std::exp(-0.08 * c));
            }
            sw[3] = 16.0f; sw[77] = 0.0f;
            for (int c = 0; c < 32; ++c) V[5 * 32 + c] = 0.0f;
        }
        std::vector<double> Wd(32 * 32, 0.0);
        for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j) {
            double a = 0;
            for (int k = 0; k < K; ++k) a += ((double)V[k * 32 + i] * (double)sw[k]) * ((double)V[k * 32 + j] * (double)sw[k]);
            Wd[i * 32 + j] = a;
        }
        float *dV, *dsw, *dW;
        CHK(hipMalloc(&dV, V.size() * 4)); CHK(hipMalloc(&dsw, K * 4)); CHK(hipMalloc(&dW, 32 * 32 * 4));
        CHK(hipMemcpy(dV, V.data(), V.size() * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(dsw, sw.data(), K * 4, hipMemcpyHostToDevice));
        std::vector<float> W(32 * 32);
        for (int pass = 0; pass < 2; ++pass) {
            CHK(hipMemset(dW, 0, 32 * 32 * 4));
            if (pass == 0) k_gram<true><<<1, 64>>>(dV, dsw, K, dW); else k_gram<false><<<1, 64>>>(dV, dsw, K, dW);
            CHK(hipDeviceSynchronize());
            CHK(hipMemcpy(W.data(), dW, W.size() * 4, hipMemcpyDeviceToHost));
            double worst = 0;
            for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j)
                worst = std::max(worst, std::fabs((double)W[i * 32 + j] - Wd[i * 32 + j]) / std::sqrt(Wd[i * 32 + i] * Wd[j * 32 + j]));
            printf("gram_%s_err_%s %.6e\n", block == 0 ? "kernel" : "wide", pass == 0 ? "new" : "before", worst);
        }
        CHK(hipFree(dV)); CHK(hipFree(dsw)); CHK(hipFree(dW));
    }
    CHK(hipFree(dv)); CHK(hipFree(ds)); CHK(hipFree(dout));

    // ---- 2. the elimination: random positive definite systems scaled to a unit diagonal ----
    {
        const int n_sys = 64;
        std::normal_distribution<double> nd;
        std::vector<float> M((size_t)n_sys * 1024), rhs(n_sys * 32);
        for (int q = 0; q < n_sys; ++q) {
            static double X[32][48], A[32][32];
            for (int i = 0; i < 32; ++i) for (int k = 0; k < 48; ++k) X[i][k] = nd(rng) * std::exp(-0.2 * i);
            for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j) { double a = 0; for (int k = 0; k < 48; ++k) a += X[i][k] * X[j][k]; A[i][j] = a + (i == j ? 1e-3 * (1 + q % 7) : 0.0); }
            for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j) M[(size_t)q * 1024 + i * 32 + j] = (float)(A[i][j] / std::sqrt(A[i][i] * A[j][j]));
            for (int i = 0; i < 32; ++i) rhs[q * 32 + i] = (float)nd(rng);
        }
        float *dM, *dr, *dz;
        CHK(hipMalloc(&dM, M.size() * 4)); CHK(hipMalloc(&dr, rhs.size() * 4)); CHK(hipMalloc(&dz, rhs.size() * 4));
        CHK(hipMemcpy(dM, M.data(), M.size() * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(dr, rhs.data(), rhs.size() * 4, hipMemcpyHostToDevice));
        double res;
        int bad;
        bad = solve_mismatches<16>(dM, dr, dz, n_sys, &res, M, rhs); printf("solve_16_mismatches %d\nsolve_16_residual %.3e\n", bad, res);
        bad = solve_mismatches<20>(dM, dr, dz, n_sys, &res, M, rhs); printf("solve_20_mismatches %d\nsolve_20_residual %.3e\n", bad, res);
        bad = solve_mismatches<24>(dM, dr, dz, n_sys, &res, M, rhs); printf("solve_24_mismatches %d\nsolve_24_residual %.3e\n", bad, res);
        bad = solve_mismatches<28>(dM, dr, dz, n_sys, &res, M, rhs); printf("solve_28_mismatches %d\nsolve_28_residual %.3e\n", bad, res);
        bad = solve_mismatches<32>(dM, dr, dz, n_sys, &res, M, rhs); printf("solve_32_mismatches %d\nsolve_32_residual %.3e\n", bad, res);
        printf("solve_values_per_size %d\n", n_sys * 32);
        CHK(hipFree(dM)); CHK(hipFree(dr)); CHK(hipFree(dz));
    }
    return 0;
}
