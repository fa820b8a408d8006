// maxent_hip.hip -- C-ABI of libmaxent_hip.so (see include/maxent_hip.h)
//
// Host side of the drop-in boundary: owns the device, whitens each data set
// (one-sided Jacobi SVD of diag(1/err) U S, done once per (U, err) pair on
// the host), stages the singular basis in HBM in the two layouts the kernel
// streams (V row-major for h = V^T H and the Gram matrix, V^T for u = V v),
// launches the chain kernel on its own stream and times it with HIP events.
#include "../../include/maxent_hip.h"
#include "mxe_kernel.hip.h"
#include "mxe_kernel_mc.hip.h"
#include "mxe_kernel_lv.hip.h"
#include "mxe_eval.hip.h"
#include "mxe_plan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <map>
#include <vector>
#include <mutex>
#include <thread>

using mxe::KParams;

namespace {

struct DataSet {
    int n_rows = 0;
    bool identity_q = true;
    std::vector<double> Q;      // n_s x n_s (row-major), caller basis <- whitened basis
    std::vector<double> c;      // n_s
    std::vector<double> Uhat;   // n_rows x n_s
    std::vector<double> err;    // n_rows
};

// Wait for the ctx stream by polling: a blocking hipStreamSynchronize was seen to return tens of
// milliseconds after the work had finished in a quarter of the processes on the MI355X boxes (the
// device time of 20 launches 33 ms, the host-side wait 67 ms); the launches last 1-20 ms, so the host
// thread spins on hipStreamQuery for up to two seconds and only then blocks.
static hipError_t stream_wait(hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return hipStreamSynchronize(s);
    }
}

// Device allocations are kept when a context lets go of them and handed to the next one that asks (per device, best
// fit): a fresh TauMaxEnt / ElementwiseMaxEnt object -- a new kernel, so a new context with its 100+ MB of result
// buffers -- otherwise pays hipMalloc + hipFree of that size, 50-150 ms per object on the MI355X boxes against 25 ms for
// everything else it does.  At most 4 GiB and 512 blocks are kept; what comes out of the pool is NOT zeroed (nothing
// here relies on zeroed memory: hipMalloc does not promise it either).
struct DevPool {
    struct Block { void* p; size_t bytes; int device; };
    std::mutex mu;
    std::vector<Block> blocks;
    size_t held = 0;
    static constexpr size_t MAX_HELD = (size_t)4 << 30, MAX_BLOCKS = 512;
    void* take(size_t bytes, size_t* got) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        int best = -1;
        for (size_t i = 0; i < blocks.size(); ++i)
            if (blocks[i].device == dev && blocks[i].bytes >= bytes && blocks[i].bytes <= 2 * bytes + 65536 &&
                (best < 0 || blocks[i].bytes < blocks[best].bytes)) best = (int)i;
        if (best < 0) return nullptr;
        void* p = blocks[best].p; *got = blocks[best].bytes;
        held -= blocks[best].bytes;
        blocks.erase(blocks.begin() + best);
        return p;
    }
    bool give(void* p, size_t bytes) {
        int dev = 0;
        if (getenv("MXE_NO_POOL") || hipGetDevice(&dev) != hipSuccess) return false;
        std::lock_guard<std::mutex> lk(mu);
        if (held + bytes > MAX_HELD || blocks.size() >= MAX_BLOCKS) return false;
        blocks.push_back(Block{p, bytes, dev});
        held += bytes;
        return true;
    }
};
DevPool g_pool;

// Large device-to-host copies into pageable memory (all H of a launch: 102 MB for the BASELINE batch) run at 2.5-5 GB/s
// through hipMemcpy on these boxes.  d2h_pipelined copies in chunks through two pinned staging buffers (allocated once
// per process): the DMA of chunk k + 1 runs while the host copies chunk k out of the other buffer.
struct PinnedPair {
    std::mutex mu;
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    static constexpr size_t CHUNK = (size_t)8 << 20;
    bool ready() {
        if (buf[0]) return true;
        for (int k = 0; k < 2; ++k) {
            if (hipHostMalloc(&buf[k], CHUNK, hipHostMallocDefault) != hipSuccess) { buf[0] = nullptr; return false; }
            if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) { buf[0] = nullptr; return false; }
        }
        return true;
    }
};
// one pair per device: an event belongs to the device it was created on, and d2h_pipelined records it on the stream of
// whichever context is fetching (with one process-wide pair, created on the device of the first context, a fetch
// on another device failed with hipErrorInvalidHandle -- BatchSolver(device_ids = (0, 1, ...)) from ~22 scans of 500
// frequencies on)
constexpr int MXE_MAX_DEVICES = 64;
PinnedPair g_pinned_dev[MXE_MAX_DEVICES];

// Pinned host memory for the callers' result arrays (mxe_host_alloc / mxe_host_free): a copy into it runs at the rate of the
// link (102 MB: 2-3 ms) where one into pageable memory takes 11-22 ms even through the staging pair above -- page faults of
// the fresh destination and the second pass of the host copy.  Blocks are kept (a few, best fit) because pinning costs
// about as much as the copy it saves.
struct HostPool {
    std::mutex mu;
    std::map<void*, size_t> live;                // handed out: base -> bytes
    std::vector<std::pair<void*, size_t>> idle;
    static constexpr size_t KEEP = 24;     // (the scalars and rows of jobs in flight are ~1 MB blocks, several per job)
    static constexpr size_t KEEP_BIG = 3, BIG = (size_t)16 << 20;
    void* take(size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        int best = -1;
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i].second >= bytes && idle[i].second <= 2 * bytes + (1u << 20) && (best < 0 || idle[i].second < idle[best].second)) best = (int)i;
        void* p = nullptr; size_t got = bytes;
        if (best >= 0) { p = idle[best].first; got = idle[best].second; idle.erase(idle.begin() + best); }
        else if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        live[p] = got;
        return p;
    }
    void give(void* p) {
        std::unique_lock<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return;
        const size_t bytes = it->second;
        live.erase(it);
        idle.emplace_back(p, bytes);
        void* drop = nullptr;
        // (of the large blocks -- all H of a launch -- three are kept, as before; the oldest goes first)
        size_t big = 0;
        for (auto& b : idle) big += b.second >= BIG;
        if (big > KEEP_BIG) {
            for (size_t i = 0; i < idle.size(); ++i) if (idle[i].second >= BIG) { drop = idle[i].first; idle.erase(idle.begin() + i); break; }
        } else if (idle.size() - big > KEEP) {
            for (size_t i = 0; i < idle.size(); ++i) if (idle[i].second < BIG) { drop = idle[i].first; idle.erase(idle.begin() + i); break; }
        }
        lk.unlock();
        if (drop) (void)hipHostFree(drop);
    }
    bool holds(const void* q, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.upper_bound(const_cast<void*>(q));
        if (it == live.begin()) return false;
        --it;
        const char* b = (const char*)it->first;
        return (const char*)q >= b && (const char*)q + bytes <= b + it->second;
    }
};
HostPool g_host;

hipError_t d2h_pipelined(void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (g_host.holds(dst, bytes)) {              // a destination of mxe_host_alloc: one DMA, no staging
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    }
    // (also the analyzers' rows of a launch, 3 MB: hipMemcpy into pageable memory took 0.7-1.1 ms for them, this way 0.3)
    if (bytes < ((size_t)256 << 10)) { hipError_t e0 = hipStreamSynchronize(s); return e0 != hipSuccess ? e0 : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MXE_MAX_DEVICES) dev = -1;
    PinnedPair* pp = dev >= 0 ? &g_pinned_dev[dev] : nullptr;
    std::unique_lock<std::mutex> lk;
    if (pp) lk = std::unique_lock<std::mutex>(pp->mu, std::try_to_lock);
    if (!pp || !lk.owns_lock() || !pp->ready()) {
        // (another thread's copy through this device's pair is in flight, or no pinned memory: a plain copy -- which runs on the
        //  null stream and does NOT wait for work queued on the non-blocking stream s: wait for it first)
        hipError_t e0 = hipStreamSynchronize(s);
        return e0 != hipSuccess ? e0 : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    }
    PinnedPair& g_pinned = *pp;
    const size_t C = PinnedPair::CHUNK, n = (bytes + C - 1) / C;
    hipError_t e = hipSuccess;
    for (size_t k = 0; k <= n && e == hipSuccess; ++k) {
        if (k < n) {
            const size_t len = std::min(C, bytes - k * C);
            e = hipMemcpyAsync(g_pinned.buf[k & 1], (const char*)src + k * C, len, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipEventRecord(g_pinned.ev[k & 1], s);
        }
        if (k > 0 && e == hipSuccess) {
            const size_t j = k - 1, len = std::min(C, bytes - j * C);
            while ((e = hipEventQuery(g_pinned.ev[j & 1])) == hipErrorNotReady) {}
            if (e == hipSuccess) std::memcpy((char*)dst + j * C, g_pinned.buf[j & 1], len);
        }
    }
    return e;
}

template <typename T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    size_t bytes = 0;                            // of the allocation (>= n * sizeof(T) when it came from the pool)
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        const size_t need = std::max<size_t>(count, 1) * sizeof(T);
        if (p && need <= bytes) { n = count; return hipSuccess; }
        if (p) { hipDeviceSynchronize(); release(); }      // (growing: whoever still reads the old block finishes first, as hipFree made sure)
        size_t got = 0;
        void* q = g_pool.take(need, &got);
        static const bool poison = getenv("MXE_POISON_ALLOC") != nullptr;      // (debugging aid: nothing may rely on what a fresh block holds)
        // (the fill runs on the null stream and the contexts' streams do not wait for that one: it has to be through before
        //  anybody writes the block -- without the wait a staged array now and then came out with the pattern in it)
        if (q) { p = (T*)q; bytes = got; n = count; if (poison) { hipMemset(p, 0xA5, bytes); hipDeviceSynchronize(); } return hipSuccess; }
        hipError_t e = hipMalloc((void**)&p, need);
        if (e == hipSuccess) { n = count; bytes = need; if (poison) { hipMemset(p, 0xA5, bytes); hipDeviceSynchronize(); } }
        return e;
    }
    // (callers make sure nothing in flight uses the block: mxe_ctx_destroy waits for its stream first)
    void release() { if (p && !g_pool.give(p, bytes)) hipFree(p); p = nullptr; n = 0; bytes = 0; }
};

} // namespace

struct mxe_ctx {
    int device = 0, n_cu = 256;         // n_cu: compute units of the device (256 where it does not say)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mark = nullptr;
    int n_tau = 0, n_omega = 0, n_s = 0, NP = 64, nwp = 0;
    std::vector<double> U, S, V;
    std::vector<DataSet> ds;
    bool ds_dirty = true;
    // elements (host)
    int n_elem = 0;
    std::vector<int> elem_ds, elem_kind;
    std::vector<double> h_sumD, h_D;           // h_D: [n_elem][nwp], for the classes of the start-state table
    // chains
    int n_chain = 0, n_alpha = 0;
    std::vector<int> chain_elem;      // per parent chain
    std::vector<int> sub_elem, sub_prob0, sub_len, sub_v0, wg_chains;   // per launched (sub-)chain
    int n_sub = 0, n_wg = 0, mc_na = 0, mc_wgpc = 1, wgpc_auto = 2, n_queue = 0, n_solo = 0;
    std::vector<int> excluded;          // problems no piece of the lock-step launch covers (more than 32 coupled directions): mxe_chains_finish
    DevBuf<int> dexcluded;
    bool mc_gst = false;              // lock-step layout with u, H, sw in device memory (frequency meshes beyond the LDS)
    // chain_kernel_lv (V^T resident in LDS as binary32, mxe_kernel_lv.hip.h): 0 = not used, 1 = it IS the launch
    // (mxe_opts.precision = F32), 2 = first pass of a binary64 launch that does not fill the GPU -- chain_kernel_mc then
    // takes every alpha as a piece of its own from the v it left (the arrays of that second pass: d2_*)
    int lv_mode = 0;
    int mc_wgpc_hint = 1;               // workgroups per CU the auto rule of the launch plan chose last (mxe_plan.h: pieces_per_scan)
    int n_wg2 = 0, wgpc2 = 1;
    DevBuf<int> d2_elem, d2_prob0, d2_len, d2_v0, d2_queue, dcnt1_niter, dcnt1_nevals;
    DevBuf<int> drounds;                // rounds per workgroup of the last lock-step launch: [n_wg] | [n_wg2] (mxe_launch_depth)
    int rounds_n[2] = {0, 0};
    int placement_checked = 0;          // the last upload that wanted solo workgroups: 0 none did, 1 the placement rule holds, 2 it does not
    DevBuf<double> dgstate_mc;
    std::vector<int> queue;
    std::vector<int> sub_pre;                                           // leading alpha of a piece: entries before its first alpha (0: none)
    std::vector<int> sub_walk0;                                         // led piece: its ladder starts at walk_alpha[sub_walk0] (-1: it walks the scan's mesh)
    std::vector<double> walk_alpha;                                     // the ladders of the led pieces of a coarse mesh (mxe_chains_upload)
    bool has_walk = false;
    bool has_pre = false;
    mxe_opts opts;
    bool chains_ready = false, launched = false;
    int last_nw = 0, last_lds = 0;
    std::string last_kernel;
    // device
    DevBuf<float> dVf, dVtf;          // binary32 copies of dV / dVt (mxe_opts.precision = F32)
    DevBuf<double> dsel3;                        // mxe_select3_launch: [3][n_chain] indices | [3][n_chain][n_omega] rows
    std::vector<double> h_sel3;
    // copies queued behind the launch (mxe_chains_prefetch / mxe_select3_prefetch_rows): where to, until a launch, an upload or a
    // finishing pass that ran makes them stale.  The fetch calls given the same destinations then only wait.
    double* pre_d = nullptr; int32_t* pre_i = nullptr; bool pre_scaled = false;
    double* pre_rows = nullptr; int pre_first = 0, pre_count = 0; bool pre_index = false;
    double* h_sel3_pinned = nullptr; size_t h_sel3_pinned_n = 0;
    // mxe_elements_update_data projects on the device: Uhat | err of every data set, built at its first call
    DevBuf<double> dproj_U, dproj_err, dproj_G;
    DevBuf<long long> dproj_off;                 // [n_ds][3]: offset of Uhat, offset of err, rows
    bool proj_ready = false;
    // mxe_fit_diagnostics: rperp = G~ - Uhat ghat of every element, [rows of its data set] at elem_roff[e].  The host copy is
    // written wherever ghat is projected on the host, the device copy by project_kernel; rperp_dirty: the host copy is the
    // newer one and goes up at the next diagnostics call.  roff_ready: drperp is sized and delem_roff holds elem_roff.
    std::vector<double> h_rperp;
    std::vector<long long> elem_roff;
    DevBuf<double> drperp;
    DevBuf<long long> delem_roff;
    bool rperp_dirty = false, roff_ready = false;
    DevBuf<double> dV, dVx, dVt, dc, dcinv, dghat, dcperp, dD, dsumD, dalpha, dv0;
    DevBuf<int> delem_ds, delem_kind, dchain_elem, dsub_prob0, dsub_len, dsub_v0, dwg_chains;
    // H, chi2, S, Q live back to back in ONE allocation (dout_pack) so that a
    // multi-GPU driver can move all per-alpha results with a single collective
    DevBuf<double> dout_v, dout_pack, dout_pack2, dB, dA, dlogdet;
    DevBuf<int> dparent_elem;
    int result_buffer = 0;        // which of the two result allocations launches write to
    struct View { double* p = nullptr; } dout_H, dout_chi2, dout_S, dout_Q;
    DevBuf<int> dout_niter, dout_nact;       // dout_niter: niter [P] | converged [P] | nevals [P] in ONE block (mxe_chains_fetch: one copy)
    struct IView { int* p = nullptr; } dout_conv, dout_nevals;
    DevBuf<long long> dprof, dprof_lf;      // (diagnostic build: stamps of the chain kernels / of linefit_kernel)
    DevBuf<int> dqueue, dcounter;           // dcounter: the pair of words of MCExtra::counter | two words of chain_kernel_lv's two passes
    int counter_par = 0;                // word of the pair the next lock-step launch draws from
    int counter_armed = -1;             // start value both words were set to / the launches re-arm to (-1: not armed)
    DevBuf<double> dalpha_log;          // [2][P]: log | log10 of dalpha, by alpha_log_kernel behind every write of dalpha (linefit_kernel)
    DevBuf<int> dsub_pre, dsub_init, dsub_walk0;
    DevBuf<double> dwalk_alpha;
    DevBuf<double> dinit_tab;           // start states per class of pieces (KParams::init_tab)
    DevBuf<double> dgstate;             // omega-space state of the chains when it does not fit LDS (KParams::gstate)
    DevBuf<int> dfin_budget, dfin_out;  // mxe_chains_finish: iterations every entry may still spend; where it writes its record (-1: a rung)
    DevBuf<double> dfin_alpha;          //   the alphas of the entries (mesh alphas and rungs)
    DevBuf<int> dfin_elem, dfin_prob0, dfin_len, dfin_v0;       // mxe_chains_finish: one piece per alpha that is solved again
    DevBuf<double> dfin_start;          //   and its start vector (the state the lock-step kernel left)
    int sel3_nc = 0;                    // scans of the launch the last mxe_select3_launch chose for (0: none since the chains were uploaded)
    bool has_init = false;
    // mxe_eval_batch / mxe_audit scratch
    DevBuf<double> ev_x, ev_alpha, ev_scal, ev_vecw, ev_vecs, ev_mat;
    DevBuf<int> ev_elem;
    // scratch blocks of the single-launch entries (each lays its block out where it fills it)
    DevBuf<double> pv_d;            // mxe_posterior_var, mxe_fit_diagnostics, mxe_response
    DevBuf<int> pv_i;               //   and mxe_posterior_sample: element | row of every problem
    DevBuf<double> ps_d;            // mxe_posterior_sample
    DevBuf<double> rr_d;            // mxe_resample_reduce, mxe_resample_quantiles
    DevBuf<int> rr_i;               //   their integers
    DevBuf<double> er_d;            // mxe_evidence_reduce
    DevBuf<int> er_i;               //   its integers
    DevBuf<long long> er_l;         //   the first row of every scan
    DevBuf<double> rows_out;        // mxe_fetch_rows: the selected rows, gathered on the device
    DevBuf<int> rows_idx;
    double chi2_factor = 1.0;     // of the staged chains (mxe_opts.chi2_factor)
    struct mxe_comm_state* comm = nullptr;      // gather between GPUs (mxe_comm_*)
    std::string hip_err;
};

// nothing may propagate through the C boundary: function-try-blocks of the entry points
#define MXE_CATCH_ALL \
    catch (const std::bad_alloc&) { return MXE_ERR_NOMEM; } \
    catch (...) { return MXE_ERR_ARG; }

#define HIPCHK(ctx, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { \
    (ctx)->hip_err = std::string(#call) + ": " + hipGetErrorString(e__); return MXE_ERR_HIP; } } while (0)

// Stage, Block and the shared checks of the single-launch entry points
#include "mxe_stage.h"

namespace {

// One-sided Jacobi (Hestenes) SVD of C (m x n, row-major, m >= 1):
// C = Uhat diag(c) Q^T.  On exit C's columns hold Uhat*c, Q the rotations.
// High relative accuracy for columns of wildly different scale, which is
// exactly the situation of diag(1/err) U S (S spans 1e1 .. 1e-14).
void jacobi_svd(std::vector<double>& C, int m, int n, std::vector<double>& Q)
{
    Q.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) Q[(size_t)i * n + i] = 1.0;
    const double eps = 2.220446049250313e-16;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                double a = 0.0, b = 0.0, g = 0.0;
                for (int i = 0; i < m; ++i) {
                    const double x = C[(size_t)i * n + p], y = C[(size_t)i * n + q];
                    a += x * x; b += y * y; g += x * y;
                }
                if (a == 0.0 || b == 0.0) continue;
                if (std::fabs(g) <= eps * std::sqrt(a * b)) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta >= 0 ? 1.0 : -1.0) /
                                 (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < m; ++i) {
                    const double x = C[(size_t)i * n + p], y = C[(size_t)i * n + q];
                    C[(size_t)i * n + p] = cs * x - sn * y;
                    C[(size_t)i * n + q] = sn * x + cs * y;
                }
                for (int i = 0; i < n; ++i) {
                    const double x = Q[(size_t)i * n + p], y = Q[(size_t)i * n + q];
                    Q[(size_t)i * n + p] = cs * x - sn * y;
                    Q[(size_t)i * n + q] = sn * x + cs * y;
                }
            }
        }
        if (!rotated) break;
    }
}

int build_dataset(mxe_ctx* ctx, int n_rows, const double* U_rot, const double* err, DataSet& d)
{
    const int ns = ctx->n_s;
    for (int i = 0; i < n_rows; ++i)
        if (!(err[i] > 0.0) || !std::isfinite(err[i])) return MXE_ERR_NUMERIC;
    d.n_rows = n_rows;
    d.err.assign(err, err + n_rows);
    const double* U = U_rot ? U_rot : ctx->U.data();
    bool scalar_err = (U_rot == nullptr);
    for (int i = 1; i < n_rows && scalar_err; ++i) scalar_err = (err[i] == err[0]);
    d.c.resize(ns);
    d.Uhat.assign((size_t)n_rows * ns, 0.0);
    if (scalar_err) {
        // the ctx's U has orthonormal columns: C = U diag(S/err) already
        d.identity_q = true;
        d.Q.clear();
        for (int k = 0; k < ns; ++k) d.c[k] = ctx->S[k] / err[0];
        std::copy(U, U + (size_t)n_rows * ns, d.Uhat.begin());
    } else {
        d.identity_q = false;
        std::vector<double> C((size_t)n_rows * ns);
        for (int i = 0; i < n_rows; ++i)
            for (int k = 0; k < ns; ++k)
                C[(size_t)i * ns + k] = U[(size_t)i * ns + k] * ctx->S[k] / err[i];
        std::vector<double> Q;
        jacobi_svd(C, n_rows, ns, Q);
        std::vector<double> nrm(ns);
        for (int k = 0; k < ns; ++k) {
            double s = 0.0;
            for (int i = 0; i < n_rows; ++i) s += C[(size_t)i * ns + k] * C[(size_t)i * ns + k];
            nrm[k] = std::sqrt(s);
        }
        std::vector<int> order(ns);
        for (int k = 0; k < ns; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nrm[a] > nrm[b]; });
        d.Q.assign((size_t)ns * ns, 0.0);
        for (int kk = 0; kk < ns; ++kk) {
            const int k = order[kk];
            d.c[kk] = nrm[k];
            for (int i = 0; i < ns; ++i) d.Q[(size_t)i * ns + kk] = Q[(size_t)i * ns + k];
            // (C has rank <= n_rows: with fewer rows than singular directions the columns behind the n_rows largest are
            //  null, their norms rounding residue of the sweeps -- normalised they would be unit vectors of noise that are
            //  not orthogonal to the others, and ghat, c_perp and the chi2 reported with them wrong by a constant)
            if (nrm[k] > 0.0 && kk < n_rows)
                for (int i = 0; i < n_rows; ++i)
                    d.Uhat[(size_t)i * ns + kk] = C[(size_t)i * ns + k] / nrm[k];
        }
    }
    double cmax = 0.0;
    for (int k = 0; k < ns; ++k) cmax = std::max(cmax, d.c[k]);
    if (!(cmax > 0.0)) return MXE_ERR_NUMERIC;
    for (int k = 0; k < ns; ++k) d.c[k] = std::max(d.c[k], 1e-150 * cmax);
    return MXE_OK;
}

int upload_bases(mxe_ctx* ctx)
{
    const int nds = (int)ctx->ds.size(), ns = ctx->n_s, NP = ctx->NP, nw = ctx->n_omega, nwp = ctx->nwp;
    // V carries zero rows behind the last data set for the look-ahead of the fused pass
    std::vector<double> hV(((size_t)nds * nwp + mxe::MC_LOOKAHEAD_ROWS) * NP, 0.0), hVt((size_t)nds * NP * nwp + 2 * mxe::MC_LOOKAHEAD_ROWS, 0.0);
    std::vector<double> hc((size_t)nds * NP, 1.0), hci((size_t)nds * NP, 1.0);
    for (int d = 0; d < nds; ++d) {
        const DataSet& D = ctx->ds[d];
        for (int i = 0; i < nw; ++i) {
            for (int k = 0; k < ns; ++k) {
                double val;
                if (D.identity_q) val = ctx->V[(size_t)i * ns + k];
                else {
                    val = 0.0;
                    for (int j = 0; j < ns; ++j) val += ctx->V[(size_t)i * ns + j] * D.Q[(size_t)j * ns + k];
                }
                hV[((size_t)d * nwp + i) * NP + k] = val;
                hVt[((size_t)d * NP + k) * nwp + i] = val;
            }
        }
        for (int k = 0; k < ns; ++k) { hc[(size_t)d * NP + k] = D.c[k]; hci[(size_t)d * NP + k] = 1.0 / D.c[k]; }
    }
    HIPCHK(ctx, ctx->dV.ensure(hV.size()));
    if (NP == 64) {
        // the lock-step fused pass reads V with 16-byte loads (the address unit takes a wave-instruction in 16 cycles
        // whatever its width: 8 B per lane stream at 32 B per cycle and CU, 16 B at 64 -- tools/l2_stream_rate.hip):
        // a lane's two doubles are the same lane position of two neighbouring 16-column tiles
        std::vector<double> hVx(hV.size(), 0.0);
        for (size_t r = 0; r < hV.size() / NP; ++r)
            for (int tp = 0; tp < 2; ++tp)
                for (int m = 0; m < 16; ++m)
                    for (int sdx = 0; sdx < 2; ++sdx)
                        hVx[r * NP + 32 * tp + 2 * m + sdx] = hV[r * NP + 16 * (2 * tp + sdx) + m];
        HIPCHK(ctx, ctx->dVx.ensure(hVx.size()));
        HIPCHK(ctx, hipMemcpyAsync(ctx->dVx.p, hVx.data(), hVx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, stream_wait(ctx->stream));
    }
    HIPCHK(ctx, ctx->dVt.ensure(hVt.size()));
    HIPCHK(ctx, ctx->dc.ensure(hc.size()));
    HIPCHK(ctx, ctx->dcinv.ensure(hci.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dV.p, hV.data(), hV.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dVt.p, hVt.data(), hVt.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dc.p, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dcinv.p, hci.data(), hci.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    std::vector<float> hVf(hV.begin(), hV.end()), hVtf(hVt.begin(), hVt.end());
    HIPCHK(ctx, ctx->dVf.ensure(hVf.size()));
    HIPCHK(ctx, ctx->dVtf.ensure(hVtf.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dVf.p, hVf.data(), hVf.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dVtf.p, hVtf.data(), hVtf.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    ctx->ds_dirty = false;
    return MXE_OK;
}

// ---- From a build (mxe::KernelBuild, chosen in mxe_plan.h) to its kernel.  Entry i of a table is the instantiation of entry i
// of mxe::LOCKSTEP_BUILDS / mxe::ONE_CHAIN_BUILDS: those lists are what is instantiated, and a build that is not in them has
// no kernel (nullptr) -- never a neighbouring one.
using LockstepFn = void (*)(KParams, mxe::MCExtra);
using OneChainFn = void (*)(KParams);
template <int I> constexpr LockstepFn lockstep_entry()
{
    constexpr mxe::LockstepKey k = mxe::LOCKSTEP_BUILDS[I];
    return mxe::chain_kernel_mc<k.NA, k.WGPC, k.lead, k.NWV, k.gst>;
}
template <int I> constexpr OneChainFn one_chain_entry()
{
    constexpr mxe::OneChainKey k = mxe::ONE_CHAIN_BUILDS[I];
    return mxe::chain_kernel<k.NW, k.NAB, std::conditional_t<k.f32, float, double>, k.gst>;
}
template <int... I> LockstepFn lockstep_at(int i, std::integer_sequence<int, I...>) { static const LockstepFn tab[] = {lockstep_entry<I>()...}; return tab[i]; }
template <int... I> OneChainFn one_chain_at(int i, std::integer_sequence<int, I...>) { static const OneChainFn tab[] = {one_chain_entry<I>()...}; return tab[i]; }
// the twelve chain_kernel builds
OneChainFn one_chain_kernel(const mxe::KernelBuild& b)
{
    const int i = mxe::build_index(b);
    if (i < 0 || b.kind != mxe::KernelBuild::ONE_CHAIN) return nullptr;
    return one_chain_at(i, std::make_integer_sequence<int, mxe::N_ONE_CHAIN_BUILDS>());
}
// the ten chain_kernel_mc builds and chain_kernel_lv
LockstepFn lockstep_kernel(const mxe::KernelBuild& b)
{
    const int i = mxe::build_index(b);
    if (i < 0 || b.kind == mxe::KernelBuild::ONE_CHAIN) return nullptr;
    return b.kind == mxe::KernelBuild::LV ? mxe::chain_kernel_lv : lockstep_at(i, std::make_integer_sequence<int, mxe::N_LOCKSTEP_BUILDS>());
}
// The one launch of a chain kernel: build b on `grid` workgroups of b.waves() wavefronts.  A lock-step or lv build takes
// (kp, *ex), a one-chain build kp alone.  MXE_ERR_STATE: the build has no kernel (nothing is enqueued then)
int launch_build(mxe_ctx* ctx, const mxe::LaunchEnv& env, const mxe::KernelBuild& b, int grid, const KParams& kp, const mxe::MCExtra* ex)
{
    const dim3 g((unsigned)grid), block(64 * b.waves());
    if (b.kind == mxe::KernelBuild::ONE_CHAIN) {
        const OneChainFn k = one_chain_kernel(b);
        if (!k) return MXE_ERR_STATE;
        HIPCHK(ctx, launch_lds(k, g, block, b.lds, ctx->stream, kp));
        return MXE_OK;
    }
    const LockstepFn k = lockstep_kernel(b);
    if (!k || !ex) return MXE_ERR_STATE;
    if (env.debug_occ && b.kind == mxe::KernelBuild::LOCKSTEP) {
        int resident = 0;
        HIPCHK(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b.lds));
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, (const void*)k, 64 * b.NWV, b.lds);
        fprintf(stderr, "[mxe] lock-step kernel NA=%d NWV=%d lds=%zu: %d workgroup(s) per CU resident\n", b.NA, b.NWV, b.lds, resident);
    }
    HIPCHK(ctx, launch_lds(k, g, block, b.lds, ctx->stream, kp, *ex));
    return MXE_OK;
}
// a host vector into a buffer of the context, on its stream (the vector has to outlive the copy: stream_wait)
template <class Buf, class Vec> hipError_t put(mxe_ctx* ctx, Buf& buf, const Vec& vec)
{
    if (const hipError_t e = buf.ensure(vec.size()); e != hipSuccess || vec.empty()) return e;
    return hipMemcpyAsync(buf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, ctx->stream);
}

} // namespace

extern "C" {

const char* mxe_version(void) { return "maxent_hip 0.1 (gfx950)"; }

#ifndef MXE_SRC_HASH
#define MXE_SRC_HASH "unknown"
#endif
const char* mxe_source_hash(void) { return MXE_SRC_HASH; }
void* mxe_host_alloc(size_t bytes) { return bytes ? g_host.take(bytes) : nullptr; }
void mxe_host_free(void* p) { if (p) g_host.give(p); }

const char* mxe_strerror(int code)
{
    switch (code) {
        case MXE_OK: return "ok";
        case MXE_ERR_ARG: return "invalid argument";
        case MXE_ERR_HIP: return "HIP runtime error (see mxe_last_hip_error)";
        case MXE_ERR_NODEVICE: return "no usable HIP device";
        case MXE_ERR_STATE: return "call order violated";
        case MXE_ERR_LIMIT: return "problem exceeds kernel limits (n_s <= 128, 160 KB LDS per chain; device SVD: more singular values above the threshold than ns_max, or a matrix with more than 128 significant directions, which svd_backend=\"host\" takes)";
        case MXE_ERR_NUMERIC: return "numerical failure (whitening: error bars must be finite and > 0; device SVD: Jacobi sweeps exhausted, or a matrix that is not finite or whose squares overflow)";
        case MXE_ERR_NOMEM: return "out of host memory";
        default: return "unknown error";
    }
}

int mxe_device_count(int* n)
{
    if (!n) return MXE_ERR_ARG;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return MXE_ERR_NODEVICE; }
    *n = c;
    return MXE_OK;
}

void mxe_opts_default(mxe_opts* o)
{
    if (!o) return;
    o->maxiter = 1000; o->miniter = 0;
    o->tol_h = 1e-9; o->tol_d = 0.0; o->tol_relq = 0.0;
    o->step_max = 0.2; o->mu_first = 1e-3; o->mu_grow = 4.0; o->mu_max = 1e20;
    o->decouple_tol = 1e-5;
    o->waves_per_chain = 0; o->chains_per_wg = 0; o->alpha_split = 0; o->stop_estimate = 1;
    o->precision = MXE_PRECISION_F64; o->wg_per_cu = 0;
    o->chi2_factor = 1.0;
    o->lds_basis = 0; o->in_flight = 0;
}

int mxe_ctx_create(int device, int n_tau, int n_omega, int n_s,
                   const double* U, const double* S, const double* V, mxe_ctx** out)
try {
    if (!out || !S || !V || n_tau < 1 || n_omega < 1 || n_s < 1) return MXE_ERR_ARG;
    if (n_s > 128) return MXE_ERR_LIMIT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return MXE_ERR_NODEVICE;
    if (device < 0 || device >= ndev) return MXE_ERR_ARG;
    mxe_ctx* ctx = new (std::nothrow) mxe_ctx();
    if (!ctx) return MXE_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return MXE_ERR_NODEVICE; }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipEventCreate(&ctx->ev_mark) != hipSuccess) {
        delete ctx; return MXE_ERR_HIP;
    }
    if (hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ctx->n_cu <= 0) { (void)hipGetLastError(); ctx->n_cu = 256; }
    ctx->n_tau = n_tau; ctx->n_omega = n_omega; ctx->n_s = n_s;
    ctx->NP = (n_s <= 64) ? 64 : 128;
    ctx->nwp = ((n_omega + 127) / 128) * 128;   // the lock-step kernel's fused pass runs whole trips of 128 rows
    if (ctx->nwp > 1536) ctx->nwp = ((n_omega + 255) / 256) * 256;     // (long meshes run its eight-wave build: trips of 256)
    if (U) ctx->U.assign(U, U + (size_t)n_tau * n_s);
    ctx->S.assign(S, S + n_s);
    ctx->V.assign(V, V + (size_t)n_omega * n_s);
    mxe_opts_default(&ctx->opts);
    if (device >= 0 && device < MXE_MAX_DEVICES) {      // (the staging buffers of d2h_pipelined: once per device -- the current one is this context's)
        std::lock_guard<std::mutex> lk(g_pinned_dev[device].mu); g_pinned_dev[device].ready();
    }
    *out = ctx;
    return MXE_OK;
}
MXE_CATCH_ALL

static void comm_release(mxe_ctx* ctx);

void mxe_ctx_destroy(mxe_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);      // (the blocks go back to the pool: nothing in flight may use them)
    comm_release(ctx);
    if (ctx->h_sel3_pinned) { (void)hipHostFree(ctx->h_sel3_pinned); ctx->h_sel3_pinned = nullptr; ctx->h_sel3_pinned_n = 0; }
    ctx->dproj_U.release(); ctx->dproj_err.release(); ctx->dproj_G.release(); ctx->dproj_off.release();
    ctx->drperp.release(); ctx->delem_roff.release();
    ctx->dVx.release(); ctx->dsel3.release(); ctx->dgstate.release(); ctx->dgstate_mc.release(); ctx->dfin_elem.release(); ctx->dfin_prob0.release();
    ctx->dfin_len.release(); ctx->dfin_v0.release(); ctx->dfin_start.release();
    ctx->dfin_budget.release(); ctx->dfin_out.release(); ctx->dfin_alpha.release();
    ctx->dlogdet.release(); ctx->dparent_elem.release(); ctx->dV.release(); ctx->dVt.release(); ctx->dVf.release(); ctx->dVtf.release(); ctx->dc.release(); ctx->dcinv.release();
    ctx->dghat.release(); ctx->dcperp.release(); ctx->dD.release(); ctx->dsumD.release();
    ctx->dalpha.release(); ctx->dv0.release(); ctx->delem_ds.release(); ctx->delem_kind.release();
    ctx->dchain_elem.release(); ctx->dsub_prob0.release(); ctx->dsub_len.release(); ctx->dsub_v0.release(); ctx->dwg_chains.release(); ctx->dqueue.release(); ctx->dcounter.release(); ctx->dalpha_log.release(); ctx->dprof_lf.release(); ctx->dsub_pre.release(); ctx->dsub_init.release(); ctx->dsub_walk0.release(); ctx->dwalk_alpha.release(); ctx->dinit_tab.release(); ctx->dout_v.release(); ctx->dout_pack.release(); ctx->dout_pack2.release();
    ctx->dout_niter.release(); ctx->dout_conv.p = ctx->dout_nevals.p = nullptr; ctx->dout_nact.release(); ctx->dexcluded.release();
    ctx->dB.release(); ctx->dA.release(); ctx->dprof.release();
    ctx->rows_out.release(); ctx->rows_idx.release();
    ctx->ev_x.release(); ctx->ev_alpha.release(); ctx->ev_scal.release(); ctx->ev_vecw.release(); ctx->ev_vecs.release();
    ctx->ev_mat.release(); ctx->ev_elem.release();
    ctx->pv_d.release(); ctx->pv_i.release();
    ctx->rr_d.release(); ctx->rr_i.release();
    ctx->er_d.release(); ctx->er_i.release(); ctx->er_l.release();
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->ev_mark) hipEventDestroy(ctx->ev_mark);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* mxe_last_hip_error(mxe_ctx* ctx) { return ctx ? ctx->hip_err.c_str() : ""; }

int mxe_dataset_add(mxe_ctx* ctx, int n_rows, const double* U_rot, const double* err, int* id)
try {
    if (!ctx || !err || n_rows < 1) return MXE_ERR_ARG;
    if (!U_rot && (ctx->U.empty() || n_rows != ctx->n_tau)) return MXE_ERR_ARG;
    DataSet d;
    int rc = build_dataset(ctx, n_rows, U_rot, err, d);
    if (rc != MXE_OK) return rc;
    ctx->ds.push_back(std::move(d));
    ctx->ds_dirty = true; ctx->proj_ready = false;
    ctx->chains_ready = false;
    if (id) *id = (int)ctx->ds.size() - 1;
    return MXE_OK;
}
MXE_CATCH_ALL

int mxe_dataset_clear(mxe_ctx* ctx)
{
    if (!ctx) return MXE_ERR_ARG;
    ctx->ds.clear(); ctx->ds_dirty = true; ctx->proj_ready = false; ctx->n_elem = 0; ctx->chains_ready = false;
    return MXE_OK;
}

namespace {
// ghat = Uhat^T (G / err) and c_perp = |G / err - Uhat ghat|^2 of elements [e0, e1): the data side of the whitened problem
// (DESIGN.md section 2).  Both along the rows of Uhat (unit stride); the residual is formed term by term (a sum of squares: no
// cancellation).  A batch of 256 elements is 5.7 M multiply-adds: on one host core 0.5-0.9 ms -- more than the kernel that solves
// them takes --, so batches are cut over a handful of threads (the arithmetic of an element does not depend on the cut).
// The residual itself, rperp, is kept for mxe_fit_diagnostics: hrperp + roff[e].
void project_elements(const mxe_ctx* ctx, int e0, int e1, const int32_t* dataset_of_elem, const double* G, const int64_t* G_offset,
                      double* hghat, double* hcperp, double* hrperp, const long long* roff)
{
    const int ns = ctx->n_s, NP = ctx->NP;
    std::vector<double> Gt;
    for (int e = e0; e < e1; ++e) {
        const DataSet& DS = ctx->ds[dataset_of_elem[e]];
        const double* Ge = G + G_offset[e];
        Gt.assign(DS.n_rows, 0.0);
        for (int i = 0; i < DS.n_rows; ++i) Gt[i] = Ge[i] / DS.err[i];
        double* gh = hghat + (size_t)e * NP;
        for (int i = 0; i < DS.n_rows; ++i) {
            const double* ui = DS.Uhat.data() + (size_t)i * ns;
            const double gi = Gt[i];
            for (int k = 0; k < ns; ++k) gh[k] += ui[k] * gi;
        }
        double cp = 0.0;
        for (int i = 0; i < DS.n_rows; ++i) {
            const double* ui = DS.Uhat.data() + (size_t)i * ns;
            double r = Gt[i];
            for (int k = 0; k < ns; ++k) r -= ui[k] * gh[k];
            hrperp[roff[e] + i] = r;
            cp += r * r;
        }
        hcperp[e] = cp;
    }
}

void project_all(const mxe_ctx* ctx, int n_elem, const int32_t* dataset_of_elem, const double* G, const int64_t* G_offset,
                 double* hghat, double* hcperp, double* hrperp, const long long* roff)
{
    int nt = (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency()));
    nt = std::min(nt, n_elem / 32);
    if (nt <= 1) { project_elements(ctx, 0, n_elem, dataset_of_elem, G, G_offset, hghat, hcperp, hrperp, roff); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        const int e0 = (int)((long long)n_elem * t / nt), e1 = (int)((long long)n_elem * (t + 1) / nt);
        pool.emplace_back(project_elements, ctx, e0, e1, dataset_of_elem, G, G_offset, hghat, hcperp, hrperp, roff);
    }
    for (auto& th : pool) th.join();
}
}

int mxe_elements_set(mxe_ctx* ctx, int n_elem, const int32_t* dataset_of_elem,
                     const double* G, const int64_t* G_offset,
                     const double* D, const int32_t* entropy)
try {
    if (!ctx || n_elem < 1 || !dataset_of_elem || !G || !G_offset || !D || !entropy) return MXE_ERR_ARG;
    if (ctx->ds.empty()) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int ns = ctx->n_s, NP = ctx->NP, nw = ctx->n_omega, nwp = ctx->nwp;
    std::vector<double> hghat((size_t)n_elem * NP, 0.0), hcperp(n_elem), hD((size_t)n_elem * nwp, 0.0), hsumD(n_elem);
    ctx->elem_ds.assign(n_elem, 0); ctx->elem_kind.assign(n_elem, 0);
    for (int e = 0; e < n_elem; ++e) {
        const int d = dataset_of_elem[e];
        if (d < 0 || d >= (int)ctx->ds.size()) return MXE_ERR_ARG;
        if (entropy[e] != MXE_ENTROPY_NORMAL && entropy[e] != MXE_ENTROPY_PLUSMINUS) return MXE_ERR_ARG;
        double sd = 0.0;
        for (int i = 0; i < nw; ++i) { hD[(size_t)e * nwp + i] = D[(size_t)e * nw + i]; sd += D[(size_t)e * nw + i]; }
        hsumD[e] = (entropy[e] == MXE_ENTROPY_PLUSMINUS) ? 2.0 * sd : sd;
        ctx->elem_ds[e] = d; ctx->elem_kind[e] = entropy[e];
    }
    ctx->elem_roff.assign(n_elem, 0);
    long long total_rows = 0;
    for (int e = 0; e < n_elem; ++e) { ctx->elem_roff[e] = total_rows; total_rows += ctx->ds[dataset_of_elem[e]].n_rows; }
    ctx->h_rperp.assign((size_t)total_rows, 0.0);
    ctx->rperp_dirty = true; ctx->roff_ready = false;
    project_all(ctx, n_elem, dataset_of_elem, G, G_offset, hghat.data(), hcperp.data(), ctx->h_rperp.data(), ctx->elem_roff.data());
    ctx->n_elem = n_elem;
    ctx->h_sumD = hsumD;
    ctx->h_D = hD;
    HIPCHK(ctx, ctx->dghat.ensure(hghat.size()));
    HIPCHK(ctx, ctx->dcperp.ensure(n_elem));
    HIPCHK(ctx, ctx->dD.ensure(hD.size()));
    HIPCHK(ctx, ctx->dsumD.ensure(n_elem));
    HIPCHK(ctx, ctx->delem_ds.ensure(n_elem));
    HIPCHK(ctx, ctx->delem_kind.ensure(n_elem));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dghat.p, hghat.data(), hghat.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dcperp.p, hcperp.data(), (size_t)n_elem * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dD.p, hD.data(), hD.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dsumD.p, hsumD.data(), (size_t)n_elem * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->delem_ds.p, ctx->elem_ds.data(), (size_t)n_elem * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->delem_kind.p, ctx->elem_kind.data(), (size_t)n_elem * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    if (ctx->ds_dirty) { int rc = upload_bases(ctx); if (rc != MXE_OK) return rc; }
    ctx->chains_ready = false;
    return MXE_OK;
}
MXE_CATCH_ALL

namespace {
// project_elements for one element per workgroup, the same operations in the same order with every product and sum rounded on
// its own (no contraction into fused multiply-adds: the host code has none either), so that new data staged this way give
// the bits mxe_elements_set gives: ghat_k = sum_i Uhat_ik G_i / err_i summed over i in turn, the residual row by row, its
// squares summed in turn.
#pragma clang fp contract(off)
__global__ __launch_bounds__(256)
void project_kernel(const double* __restrict__ G, const int* __restrict__ elem_ds, const long long* __restrict__ ds_off,
                    const double* __restrict__ U, const double* __restrict__ err, int ns, int NP,
                    double* __restrict__ ghat, double* __restrict__ cperp, int rows_max, const long long* __restrict__ G_off,
                    double* __restrict__ rperp, const long long* __restrict__ roff)
{
    extern __shared__ double psh[];
    double* Gt = psh; double* gh = psh + rows_max; double* r2 = gh + NP;
    const int e = blockIdx.x, tid = threadIdx.x;
    const long long* o = ds_off + 3 * (size_t)elem_ds[e];
    const double* Ud = U + o[0]; const double* ed = err + o[1]; const int rows = (int)o[2];
    const double* Ge = G + G_off[e];
    for (int i = tid; i < rows; i += 256) Gt[i] = Ge[i] / ed[i];
    __syncthreads();
    for (int k = tid; k < NP; k += 256) {
        double acc = 0.0;
        if (k < ns) for (int i = 0; i < rows; ++i) { const double pr = Ud[(size_t)i * ns + k] * Gt[i]; acc = acc + pr; }
        gh[k] = acc;
        ghat[(size_t)e * NP + k] = acc;
    }
    __syncthreads();
    for (int i = tid; i < rows; i += 256) {
        double r = Gt[i];
        for (int k = 0; k < ns; ++k) { const double pr = Ud[(size_t)i * ns + k] * gh[k]; r = r - pr; }
        rperp[roff[e] + i] = r;
        r2[i] = r * r;
    }
    __syncthreads();
    if (tid == 0) {
        double cp = 0.0;
        for (int i = 0; i < rows; ++i) cp = cp + r2[i];
        cperp[e] = cp;
    }
}
#pragma clang fp contract(fast)

// Uhat | err of every data set on the device (project_kernel, fitdiag_kernel), built again after a change of data sets
int upload_projection(mxe_ctx* ctx)
{
    if (ctx->proj_ready) return MXE_OK;
    std::vector<double> hU, herr; std::vector<long long> off;
    for (const DataSet& D : ctx->ds) {
        off.push_back((long long)hU.size()); off.push_back((long long)herr.size()); off.push_back(D.n_rows);
        hU.insert(hU.end(), D.Uhat.begin(), D.Uhat.end());
        herr.insert(herr.end(), D.err.begin(), D.err.end());
    }
    HIPCHK(ctx, ctx->dproj_U.ensure(hU.size()));
    HIPCHK(ctx, ctx->dproj_err.ensure(herr.size()));
    HIPCHK(ctx, ctx->dproj_off.ensure(off.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dproj_U.p, hU.data(), hU.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dproj_err.p, herr.data(), herr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dproj_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    ctx->proj_ready = true;
    return MXE_OK;
}

// room for rperp of the elements that are set, and where each element's rows begin (after mxe_elements_set)
int upload_row_offsets(mxe_ctx* ctx)
{
    if (ctx->roff_ready) return MXE_OK;
    HIPCHK(ctx, ctx->drperp.ensure(ctx->h_rperp.size()));
    HIPCHK(ctx, ctx->delem_roff.ensure(ctx->elem_roff.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->delem_roff.p, ctx->elem_roff.data(), ctx->elem_roff.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    ctx->roff_ready = true;
    return MXE_OK;
}
}

int mxe_elements_update_data(mxe_ctx* ctx, int n_elem, const double* G, const int64_t* G_offset)
try {
    if (!ctx || !G || !G_offset) return MXE_ERR_ARG;
    if (ctx->n_elem < 1 || ctx->ds.empty() || ctx->ds_dirty) return MXE_ERR_STATE;
    if (n_elem != ctx->n_elem) return MXE_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int ns = ctx->n_s, NP = ctx->NP;
    // the data of the elements as ONE span of the caller's array (what set_elements of maxent_amd.device builds; anything else
    // goes through the host projection)
    long long lo = 0, hi = 0; int rows_max = 0; bool span = true;
    for (int e = 0; e < n_elem && span; ++e) {
        const int rows = ctx->ds[ctx->elem_ds[e]].n_rows;
        rows_max = std::max(rows_max, rows);
        if (G_offset[e] < 0) span = false;
        if (e == 0) { lo = G_offset[e]; hi = lo + rows; }
        else { lo = std::min<long long>(lo, G_offset[e]); hi = std::max<long long>(hi, G_offset[e] + rows); }
    }
    size_t total_rows = 0;
    for (int e = 0; e < n_elem; ++e) total_rows += ctx->ds[ctx->elem_ds[e]].n_rows;
    const size_t lds = ((size_t)2 * rows_max + NP) * 8;
    if (span && (size_t)(hi - lo) <= 2 * total_rows && lds <= 64 * 1024 && !getenv("MXE_HOST_PROJECTION")) {
        int rc = upload_projection(ctx);
        if (rc != MXE_OK) return rc;
        rc = upload_row_offsets(ctx);
        if (rc != MXE_OK) return rc;
        std::vector<long long> goff(n_elem);
        for (int e = 0; e < n_elem; ++e) goff[e] = G_offset[e] - lo;
        HIPCHK(ctx, ctx->dproj_G.ensure((size_t)(hi - lo) + (size_t)n_elem));
        // (offsets behind the data in the same allocation: two copies, one wait)
        long long* dgoff = (long long*)(ctx->dproj_G.p + (hi - lo));
        HIPCHK(ctx, hipMemcpyAsync(ctx->dproj_G.p, G + lo, (size_t)(hi - lo) * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(dgoff, goff.data(), (size_t)n_elem * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(project_kernel, dim3(n_elem), dim3(256), lds, ctx->stream, ctx->dproj_G.p, ctx->delem_ds.p, ctx->dproj_off.p,
                           ctx->dproj_U.p, ctx->dproj_err.p, ns, NP, ctx->dghat.p, ctx->dcperp.p, rows_max, dgoff,
                           ctx->drperp.p, ctx->delem_roff.p);
        HIPCHK(ctx, hipGetLastError());
        ctx->rperp_dirty = false;                    // (the device copy of rperp is the one that holds)
        HIPCHK(ctx, stream_wait(ctx->stream));       // (goff is the caller-side vector of this call; G the caller's array)
        return MXE_OK;
    }
    std::vector<double> hghat((size_t)n_elem * NP, 0.0), hcperp(n_elem);
    project_all(ctx, n_elem, ctx->elem_ds.data(), G, G_offset, hghat.data(), hcperp.data(), ctx->h_rperp.data(),
                ctx->elem_roff.data());                                                     // (as mxe_elements_set: the same bits)
    ctx->rperp_dirty = true;
    // (behind whatever the stream still runs with the old data)
    HIPCHK(ctx, hipMemcpyAsync(ctx->dghat.p, hghat.data(), hghat.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dcperp.p, hcperp.data(), (size_t)n_elem * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}
MXE_CATCH_ALL

namespace {
int launch_eval(mxe_ctx* ctx, const mxe::EvalParams& ep, size_t P);
void eval_params_base(mxe_ctx* ctx, mxe::EvalParams& ep);

// Start states of the lock-step kernel (KParams::init_tab): every piece of a scan starts from the scan's v0, and
// scans of one class -- same data set, entropy, default model, v0 -- share what the evaluation of that vector
// gives: H, S, h = V^T H, the Gram matrix.  They are evaluated ONCE per class with the device's own evaluation
// kernel (eval_kernel, the one behind mxe_eval_batch) when the chains are uploaded, and a piece begins with a
// Newton step instead of the evaluation of its start vector (one round of the kernel per piece).  At most
// eight classes; scans beyond that start the old way.
int build_init_table(mxe_ctx* ctx, int n_chain, const int32_t* elem_of_chain, const std::vector<double>& hv0)
{
    ctx->has_init = false;
    const int NP = ctx->NP, nw = ctx->n_omega, nwp = ctx->nwp;
    if (NP != 64 || ctx->mc_na != 32) return MXE_OK;
    std::vector<int> rep, class_of(n_chain, -1);
    for (int c = 0; c < n_chain; ++c) {
        const int e = elem_of_chain[c];
        int k = -1;
        for (size_t q = 0; q < rep.size() && k < 0; ++q) {
            const int c0 = rep[q], e0 = elem_of_chain[c0];
            if (ctx->elem_kind[e0] == ctx->elem_kind[e] && ctx->elem_ds[e0] == ctx->elem_ds[e] &&
                std::memcmp(&hv0[(size_t)c0 * NP], &hv0[(size_t)c * NP], (size_t)NP * 8) == 0 &&
                (e0 == e || std::memcmp(&ctx->h_D[(size_t)e0 * nwp], &ctx->h_D[(size_t)e * nwp], (size_t)nwp * 8) == 0)) k = (int)q;
        }
        if (k < 0 && rep.size() < 8) { k = (int)rep.size(); rep.push_back(c); }
        class_of[c] = k;
    }
    const int P = (int)rep.size();
    if (P == 0) return MXE_OK;
    std::vector<double> hx((size_t)P * NP), halpha(P, 1.0);
    std::vector<int> helem(P);
    for (int q = 0; q < P; ++q) {
        std::copy(hv0.begin() + (size_t)rep[q] * NP, hv0.begin() + (size_t)(rep[q] + 1) * NP, hx.begin() + (size_t)q * NP);
        helem[q] = elem_of_chain[rep[q]];
    }
    HIPCHK(ctx, ctx->ev_x.ensure(hx.size()));
    HIPCHK(ctx, ctx->ev_alpha.ensure(P));
    HIPCHK(ctx, ctx->ev_elem.ensure(P));
    HIPCHK(ctx, ctx->ev_scal.ensure((size_t)5 * P));
    HIPCHK(ctx, ctx->ev_vecw.ensure((size_t)4 * P * nw));
    HIPCHK(ctx, ctx->ev_vecs.ensure((size_t)2 * P * NP));
    HIPCHK(ctx, ctx->ev_mat.ensure((size_t)P * NP * NP));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ev_x.p, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ev_alpha.p, halpha.data(), (size_t)P * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ev_elem.p, helem.data(), (size_t)P * 4, hipMemcpyHostToDevice, ctx->stream));
    mxe::EvalParams ep;
    eval_params_base(ctx, ep);
    ep.elem = ctx->ev_elem.p; ep.alpha = ctx->ev_alpha.p; ep.x = ctx->ev_x.p; ep.x_stride = NP;
    ep.input_is_H = 0; ep.eta = 1.0; ep.want_gram = 1;
    ep.Q = ctx->ev_scal.p; ep.chi2 = ep.Q + P; ep.S = ep.chi2 + P;
    ep.H = ctx->ev_vecw.p; ep.u = ep.H + (size_t)P * nw; ep.w = ep.u + (size_t)P * nw;
    ep.h = ctx->ev_vecs.p; ep.g = ep.h + (size_t)P * NP;
    ep.W = ctx->ev_mat.p;
    int rc = launch_eval(ctx, ep, (size_t)P);
    if (rc != MXE_OK) return rc;
    std::vector<double> hS(P), hH((size_t)P * nw), hw((size_t)P * nw), hh((size_t)P * NP), hW((size_t)P * NP * NP);
    HIPCHK(ctx, hipMemcpyAsync(hS.data(), ep.S, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hH.data(), ep.H, hH.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hw.data(), ep.w, hw.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hh.data(), ep.h, hh.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hW.data(), ep.W, hW.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    const int STR = mxe::MC_INIT_STRIDE;
    std::vector<double> tab((size_t)P * STR, 0.0);
    for (int q = 0; q < P; ++q) {
        double Hn2 = 0.0, wmax = 0.0;
        for (int i = 0; i < nw; ++i) { Hn2 += hH[(size_t)q * nw + i] * hH[(size_t)q * nw + i]; wmax = std::max(wmax, hw[(size_t)q * nw + i]); }
        if (!(wmax > 1e-290 && wmax < 1e290) || !std::isfinite(Hn2) || !std::isfinite(hS[q])) {       // nothing to tabulate: these scans start the old way
            for (int c = 0; c < n_chain; ++c) if (class_of[c] == q) class_of[c] = -1;
            continue;
        }
        const double sc2 = std::ldexp(1.0, 8 - std::ilogb(wmax));       // as the kernel scales the operands of its Gram tiles
        double* T = &tab[(size_t)q * STR];
        const double* W = &hW[(size_t)q * NP * NP];
        int pr = 0;
        for (int mt = 0; mt < 2; ++mt)
            for (int nt = mt; nt < 2; ++nt, ++pr)
                for (int r = 0; r < 4; ++r)
                    for (int l = 0; l < 64; ++l) {
                        const int a = 16 * mt + 4 * (l >> 4) + r, b = 16 * nt + (l & 15);      // accumulator layout of the 16 x 16 tile
                        T[(pr * 4 + r) * 64 + l] = sc2 * W[(size_t)a * NP + b];
                    }
        for (int k = 0; k < NP; ++k) T[3 * 256 + k] = hh[(size_t)q * NP + k];
        T[3 * 256 + NP + 0] = hS[q]; T[3 * 256 + NP + 1] = Hn2; T[3 * 256 + NP + 2] = wmax; T[3 * 256 + NP + 3] = sc2;
    }
    std::vector<int> sub_init(std::max(ctx->n_sub, 1), -1);
    bool any = false;
    for (int sc = 0; sc < ctx->n_sub; ++sc) { sub_init[sc] = class_of[ctx->sub_v0[sc]]; any = any || sub_init[sc] >= 0; }
    if (!any) return MXE_OK;
    HIPCHK(ctx, ctx->dinit_tab.ensure(tab.size()));
    HIPCHK(ctx, ctx->dsub_init.ensure(sub_init.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dinit_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dsub_init.p, sub_init.data(), sub_init.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    ctx->has_init = true;
    return MXE_OK;
}
// Which workgroups of a launch of two per CU share a CU?  The solo schedule of the lock-step kernel (the longest pieces get a
// CU to themselves: workgroup b's partner b + gridDim / 2 leaves at once) rests on an OBSERVED placement -- the dispatcher fills
// every CU with one workgroup before any gets its second, in order -- that HIP does not promise.  Probed once per device with
// the launch shape of that kernel (256 threads, LDS for exactly two workgroups per CU, every workgroup resident at once):
// every workgroup records XCC_ID / HW_ID; the rule holds when b and b + n_cu report the same CU for every b.  Where it does
// not, n_solo stays 0: the schedule is a speed-up only, results never depend on it.
__global__ __launch_bounds__(256)
void placement_probe_kernel(unsigned* out)
{
    extern __shared__ char probe_lds[];
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = hw; out[2 * blockIdx.x + 1] = xcc; probe_lds[0] = 1; }
    const long long t0 = clock64();
    while (clock64() - t0 < 60000) { }           // ~25 us: every workgroup of the grid is resident before the first one leaves
}
int g_placement[MXE_MAX_DEVICES];                // 0: not probed, 1: the rule holds, 2: it does not
std::mutex g_placement_mu;

int placement_rule_holds(mxe_ctx* ctx, int n_cu, bool* holds)
{
    *holds = false;
    if (getenv("MXE_FORCE_NO_SOLO_RULE")) return MXE_OK;              // (tests: the branch a different dispatcher would take)
    const int dev = ctx->device;
    if (dev < 0 || dev >= MXE_MAX_DEVICES) return MXE_OK;
    std::lock_guard<std::mutex> lk(g_placement_mu);
    if (g_placement[dev] == 0) {
        const int n = 2 * n_cu;
        DevBuf<unsigned> d;
        HIPCHK(ctx, d.ensure((size_t)2 * n));
        HIPCHK(ctx, hipFuncSetAttribute((const void*)placement_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 73728));
        std::vector<unsigned> h((size_t)2 * n);
        bool ok = true;
        for (int rep = 0; rep < 2 && ok; ++rep) {          // (twice: the rule has to hold on every launch, not on the first)
            hipLaunchKernelGGL(placement_probe_kernel, dim3(n), dim3(256), 73728, ctx->stream, d.p);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(h.data(), d.p, h.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, stream_wait(ctx->stream));
            for (int b = 0; b < n_cu && ok; ++b)
                ok = ((h[2 * b] >> 8) & 0xff) == ((h[2 * (b + n_cu)] >> 8) & 0xff) && (h[2 * b + 1] & 0xf) == (h[2 * (b + n_cu) + 1] & 0xf);      // (HW_ID: CU 11:8, SH 12, SE 15:13; XCC_ID 3:0)
        }
        d.release();
        g_placement[dev] = ok ? 1 : 2;
    }
    *holds = g_placement[dev] == 1;
    return MXE_OK;
}

// the environment overrides of the launch plan (A/B runs and tests): the only environment reads of mxe_chains_upload's decisions
void read_plan_env(mxe::PlanEnv& env)
{
    if (const char* e = getenv("MXE_TAPER")) env.taper = std::max(0.2, atof(e));
    if (const char* e = getenv("MXE_LADDER_RATIO")) env.ladder_ratio = std::max(1.05, atof(e));
    env.no_lds_basis = getenv("MXE_NO_LDS_BASIS") != nullptr; env.no_split_by_kind = getenv("MXE_NO_SPLIT_BY_KIND") != nullptr;
    env.no_ladder = getenv("MXE_NO_LADDER") != nullptr; env.no_na64 = getenv("MXE_NO_NA64") != nullptr; env.no_sorted_static = getenv("MXE_NO_SORTED_STATIC") != nullptr;
}
// ... and of the plan of the finishing pass: the only environment reads of mxe_chains_finish's decisions (plan_finish clamps)
void read_finish_env(mxe::FinishEnv& env)
{
    if (const char* e = getenv("MXE_FIN_RATIO")) env.ratio = atof(e);
    if (const char* e = getenv("MXE_FIN_RUNG_ITERS")) env.rung_iters = atoi(e);
    env.no_ladder = getenv("MXE_NO_FINISH_LADDER") != nullptr;
}
// ... and of a launch of a chain kernel (mxe_chains_launch, mxe_chains_finish): the only environment reads of either.  Once per
// launch -- tests set MXE_COUNT_ROUNDS for a single one --, except MXE_POISON_LDS, which is read once per process as ever
void read_launch_env(mxe::LaunchEnv& env)
{
    static const int poison = getenv("MXE_POISON_LDS") ? atoi(getenv("MXE_POISON_LDS")) : 0;
    env.poison_lds = poison;
    env.count_rounds = getenv("MXE_COUNT_ROUNDS") != nullptr; env.debug_occ = getenv("MXE_DEBUG_OCC") != nullptr;
    if (const char* e = getenv("MXE_MC_MAXEVALS")) { env.has_mc_maxevals = true; env.mc_maxevals = atoi(e); }
    if (const char* e = getenv("MXE_STUCK_SKIP")) env.stuck_skip = atoi(e);
}
}  // namespace

// Stages the chains of a launch.  What is launched -- pieces, kernel, layout, order -- is decided by mxe::plan_launch
// (mxe_plan.h) from numbers alone; this function checks, asks, and then carries the plan out.
int mxe_chains_upload(mxe_ctx* ctx, int n_chain, int n_alpha,
                      const int32_t* elem_of_chain, const double* alpha_scaled,
                      const double* v0, const mxe_opts* opts)
try {
    // ---- 1. arguments and options (nothing of the context's staged launch is written before the plan stands)
    if (!ctx || n_chain < 1 || n_alpha < 1 || !elem_of_chain || !alpha_scaled || !v0) return MXE_ERR_ARG;
    if (ctx->n_elem < 1) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->ds_dirty) { int rc = upload_bases(ctx); if (rc != MXE_OK) return rc; }
    const int ns = ctx->n_s, NP = ctx->NP, nw = ctx->n_omega, nwp = ctx->nwp;
    const size_t P = (size_t)n_chain * n_alpha;
    mxe_opts o; if (opts) o = *opts; else mxe_opts_default(&o);
    if (o.maxiter < 1 || o.step_max <= 0 || o.mu_first <= 0 || o.mu_grow <= 1.0 || o.decouple_tol < 0) return MXE_ERR_ARG;
    if (o.waves_per_chain != 0 && o.waves_per_chain != 1 && o.waves_per_chain != 2 && o.waves_per_chain != 4 && o.waves_per_chain != 8) return MXE_ERR_ARG;
    if (o.chains_per_wg != 0 && o.chains_per_wg != 1 && o.chains_per_wg != 4) return MXE_ERR_ARG;
    if (o.alpha_split < 0 || o.wg_per_cu < 0 || o.wg_per_cu > 2 || o.in_flight < 0 || o.in_flight > 64) return MXE_ERR_ARG;
    if (o.precision != MXE_PRECISION_F64 && o.precision != MXE_PRECISION_F32) return MXE_ERR_ARG;
    if (o.precision == MXE_PRECISION_F32 && NP != 64) return MXE_ERR_LIMIT;
    if (!(o.chi2_factor > 0.0) || !std::isfinite(o.chi2_factor)) return MXE_ERR_ARG;
    for (int c = 0; c < n_chain; ++c) if (elem_of_chain[c] < 0 || elem_of_chain[c] >= ctx->n_elem) return MXE_ERR_ARG;
    for (size_t i = 0; i < P; ++i) if (!(alpha_scaled[i] > 0.0) || !std::isfinite(alpha_scaled[i])) return MXE_ERR_ARG;
    // ---- 2. the start vectors in the whitened basis of their data sets: v' = Q^T v
    std::vector<double> hv0((size_t)n_chain * NP, 0.0);
    for (int c = 0; c < n_chain; ++c) {
        const DataSet& DS = ctx->ds[ctx->elem_ds[elem_of_chain[c]]];
        for (int k = 0; k < ns; ++k) {
            double s = DS.identity_q ? v0[(size_t)c * ns + k] : 0.0;
            if (!DS.identity_q) for (int j = 0; j < ns; ++j) s += DS.Q[(size_t)j * ns + k] * v0[(size_t)c * ns + j];
            hv0[(size_t)c * NP + k] = s;
        }
    }
    // ---- 3. what the plan reads.  Q = eta chi2 / 2 - alpha S has the minimiser of chi2 / 2 - (alpha / eta) S: the device
    // iterates on alpha / eta and the fetch multiplies Q by eta (cost_function.py:60, bryan_cost_function.py:71)
    std::vector<double> alpha_dev(alpha_scaled, alpha_scaled + P);
    if (o.chi2_factor != 1.0) for (double& a : alpha_dev) a /= o.chi2_factor;
    std::vector<int> ds_rows(ctx->ds.size()); std::vector<double> ds_c32(ctx->ds.size(), 0.0);
    for (size_t d = 0; d < ctx->ds.size(); ++d) { ds_rows[d] = ctx->ds[d].n_rows; if (ns > 32) ds_c32[d] = ctx->ds[d].c[32]; }
    mxe::PlanInput in;
    in.n_chain = n_chain; in.n_alpha = n_alpha; in.elem_of_chain = elem_of_chain; in.alpha = alpha_dev.data();
    in.elem_kind = ctx->elem_kind.data(); in.elem_ds = ctx->elem_ds.data(); in.elem_sumD = ctx->h_sumD.data();
    in.n_ds = (int)ctx->ds.size(); in.ds_rows = ds_rows.data(); in.ds_c32 = ds_c32.data();
    in.n_s = ns; in.NP = NP; in.n_omega_pad = nwp; in.n_cu = ctx->n_cu; in.opts = o;
    in.wgpc_auto = ctx->wgpc_auto; in.mc_wgpc_hint = ctx->mc_wgpc_hint;
    read_plan_env(in.env);
    mxe::LaunchPlan plan;       // ---- 4. the plan
    if (const int rc = mxe::plan_launch(in, plan); rc != MXE_OK) {
        if (plan.uncovered || plan.covered_twice) fprintf(stderr, "mxe_chains_upload: %zu problems covered by no piece, %zu by two (layout %d, %zu pieces, %zu excluded)\n",
                                                          plan.uncovered, plan.covered_twice, plan.layout, plan.pieces.size(), plan.excluded.size());
        return rc;
    }
    // ---- 5. solo workgroups only where workgroups b and b + n_wg / 2 do share a CU on this device: probed once, see placement_rule_holds
    int n_solo = 0, placement_checked = 0;
    if (plan.solo_rule) {
        bool holds = false;
        if (plan.n_solo_wanted > 0) { const int rp = placement_rule_holds(ctx, ctx->n_cu, &holds); if (rp != MXE_OK) return rp; }
        placement_checked = holds ? 1 : 2; n_solo = (holds && plan.lv_mode != 2) ? plan.n_solo_wanted : 0;
    }
    // ---- 6. the plan becomes the context's staged launch (a failure from here on leaves nothing staged)
    ctx->chains_ready = false; ctx->launched = false; ctx->sel3_nc = 0; ctx->has_init = false;
    ctx->opts = o; ctx->opts.precision = plan.precision; ctx->chi2_factor = o.chi2_factor;
    ctx->n_chain = n_chain; ctx->n_alpha = n_alpha; ctx->chain_elem.assign(elem_of_chain, elem_of_chain + n_chain);
    const size_t n_sub = plan.pieces.size();
    for (auto* v : {&ctx->sub_elem, &ctx->sub_prob0, &ctx->sub_len, &ctx->sub_v0, &ctx->sub_pre, &ctx->sub_walk0}) v->resize(n_sub);
    ctx->n_sub = (int)n_sub; ctx->has_pre = false;
    for (size_t sc = 0; sc < n_sub; ++sc) {
        const mxe::Piece& p = plan.pieces[sc];
        ctx->sub_elem[sc] = p.elem; ctx->sub_prob0[sc] = p.prob0; ctx->sub_len[sc] = p.len; ctx->sub_v0[sc] = p.v0;
        ctx->sub_pre[sc] = p.pre; ctx->sub_walk0[sc] = p.walk0; ctx->has_pre |= p.pre > 0;
    }
    ctx->has_walk = !plan.walk_alpha.empty(); ctx->walk_alpha = std::move(plan.walk_alpha); ctx->excluded = std::move(plan.excluded);
    ctx->queue = std::move(plan.queue); ctx->wg_chains = std::move(plan.wg_chains); ctx->n_queue = (int)ctx->queue.size();
    ctx->mc_na = plan.mc_na; ctx->mc_wgpc = plan.mc_wgpc; ctx->mc_gst = plan.mc_gst; ctx->lv_mode = plan.lv_mode;
    ctx->wgpc_auto = plan.wgpc_auto; ctx->mc_wgpc_hint = plan.mc_wgpc_hint; ctx->n_wg = plan.n_wg; ctx->n_wg2 = plan.n_wg2; ctx->wgpc2 = plan.wgpc2;
    ctx->n_solo = n_solo; ctx->placement_checked = placement_checked;
    // ---- 7. buffers
    HIPCHK(ctx, ctx->dcounter.ensure(4)); HIPCHK(ctx, put(ctx, ctx->dqueue, ctx->queue));
    // both words of the counter pair start at what a launch of this plan draws from (mxe_chains_launch: counter0); from then on
    // every launch re-arms the word of the next one
    const int counter0 = (ctx->n_queue > 0 && ctx->mc_wgpc == 2 && n_solo > 0) ? (ctx->n_wg - n_solo) * 4 : 0;
    const std::vector<int> counter_words = {counter0, counter0, 0, 0};
    ctx->counter_armed = -1; ctx->counter_par = 0;
    HIPCHK(ctx, put(ctx, ctx->dcounter, counter_words));
    HIPCHK(ctx, put(ctx, ctx->dwg_chains, ctx->wg_chains));
    HIPCHK(ctx, put(ctx, ctx->dchain_elem, ctx->sub_elem)); HIPCHK(ctx, put(ctx, ctx->dsub_prob0, ctx->sub_prob0));
    HIPCHK(ctx, put(ctx, ctx->dsub_len, ctx->sub_len)); HIPCHK(ctx, put(ctx, ctx->dsub_v0, ctx->sub_v0));
    HIPCHK(ctx, ctx->dsub_pre.ensure(n_sub));
    if (ctx->has_pre || ctx->mc_gst) HIPCHK(ctx, put(ctx, ctx->dsub_pre, ctx->sub_pre));     // (the device-memory-state build is the LEAD build: it reads the array)
    if (ctx->has_walk && ctx->has_pre) { HIPCHK(ctx, put(ctx, ctx->dsub_walk0, ctx->sub_walk0)); HIPCHK(ctx, put(ctx, ctx->dwalk_alpha, ctx->walk_alpha)); }
    if (!ctx->excluded.empty()) HIPCHK(ctx, put(ctx, ctx->dexcluded, ctx->excluded));
    HIPCHK(ctx, put(ctx, ctx->dalpha, alpha_dev)); HIPCHK(ctx, put(ctx, ctx->dv0, hv0)); HIPCHK(ctx, ctx->dout_v.ensure(P * NP));
    // the logarithms of the mesh for linefit_kernel: this is the only writer of dalpha, so the table cannot go stale
    HIPCHK(ctx, ctx->dalpha_log.ensure(2 * P));
    hipLaunchKernelGGL(mxe::alpha_log_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dalpha.p, ctx->dalpha_log.p, P);
    HIPCHK(ctx, hipGetLastError());
    // one allocation: H [P][nw] | chi2 S Q [3P] | H of the analyzer's alpha [n_chain][nw] | its index [n_chain]
    // (everything behind H is the COMPACT result pack that a gather between GPUs moves)
    HIPCHK(ctx, ctx->dout_pack.ensure(P * nw + 3 * P + (size_t)n_chain * (nw + 1)));
    ctx->result_buffer = 0;
    ctx->dout_H.p = ctx->dout_pack.p; ctx->dout_chi2.p = ctx->dout_pack.p + P * nw;
    ctx->dout_S.p = ctx->dout_chi2.p + P; ctx->dout_Q.p = ctx->dout_S.p + P;
    HIPCHK(ctx, ctx->dout_niter.ensure(3 * P)); HIPCHK(ctx, ctx->dout_nact.ensure(P));
    ctx->dout_conv.p = ctx->dout_niter.p + P; ctx->dout_nevals.p = ctx->dout_conv.p + P;
    std::vector<int> e2, p2, l2;       // the second pass of lv_mode 2: every alpha a piece of its own, in the order of the problems
    if (ctx->lv_mode == 2) {
        e2.resize(P); p2.resize(P); l2.assign(P, 1);
        for (size_t i = 0; i < P; ++i) { e2[i] = elem_of_chain[i / n_alpha]; p2[i] = (int)i; }
        HIPCHK(ctx, put(ctx, ctx->d2_elem, e2)); HIPCHK(ctx, put(ctx, ctx->d2_len, l2));
        HIPCHK(ctx, put(ctx, ctx->d2_prob0, p2)); HIPCHK(ctx, put(ctx, ctx->d2_v0, p2)); HIPCHK(ctx, put(ctx, ctx->d2_queue, p2));
        HIPCHK(ctx, ctx->dcnt1_niter.ensure(P)); HIPCHK(ctx, ctx->dcnt1_nevals.ensure(P));
    }
    HIPCHK(ctx, stream_wait(ctx->stream));          // (the host vectors go out of scope)
    ctx->counter_armed = counter0;
    // ---- 8. the start states of the pieces
    { const int rc_init = build_init_table(ctx, n_chain, elem_of_chain, hv0); if (rc_init != MXE_OK) return rc_init; }
    ctx->chains_ready = true;
    return MXE_OK;
}
MXE_CATCH_ALL

// the kernel parameters of the staged chains (mxe_chains_launch; mxe_chains_finish replaces the chain arrays)
constexpr int MC_MAXITER = 32;       // iterations the lock-step kernel spends on one alpha before it gives it up (mxe_chains_finish)
static void fill_kparams(mxe_ctx* ctx, const mxe::LaunchEnv& env, KParams& kp)
{
    const mxe_opts& o = ctx->opts;
    kp.n_omega = ctx->n_omega; kp.n_omega_pad = ctx->nwp; kp.n_s = ctx->n_s; kp.NP = ctx->NP;
    kp.n_alpha = ctx->n_alpha; kp.n_chain = ctx->n_chain;
    kp.Vf = ctx->dVf.p; kp.Vtf = ctx->dVtf.p;
    kp.V = ctx->dV.p; kp.Vx = ctx->dVx.p; kp.Vt = ctx->dVt.p; kp.c = ctx->dc.p; kp.cinv = ctx->dcinv.p;
    kp.elem_ds = ctx->delem_ds.p; kp.elem_kind = ctx->delem_kind.p;
    kp.ghat = ctx->dghat.p; kp.cperp = ctx->dcperp.p; kp.D = ctx->dD.p; kp.sumD = ctx->dsumD.p;
    kp.chain_elem = ctx->dchain_elem.p; kp.alpha = ctx->dalpha.p; kp.v0 = ctx->dv0.p;
    kp.chain_prob0 = ctx->dsub_prob0.p; kp.chain_len = ctx->dsub_len.p; kp.chain_v0 = ctx->dsub_v0.p;
    kp.chain_lead = ((ctx->has_pre || ctx->mc_gst) && ctx->mc_na > 0) ? ctx->dsub_pre.p : nullptr;
    const bool walks = ctx->has_walk && ctx->has_pre && ctx->mc_na > 0;
    kp.chain_walk0 = walks ? ctx->dsub_walk0.p : nullptr;
    kp.walk_alpha = walks ? ctx->dwalk_alpha.p : nullptr;
    kp.init_tab = (ctx->has_init && ctx->mc_na > 0) ? ctx->dinit_tab.p : nullptr;
    kp.chain_init = ctx->dsub_init.p;
    kp.n_chain = ctx->n_sub;
    kp.out_v = ctx->dout_v.p; kp.out_H = ctx->dout_H.p; kp.out_chi2 = ctx->dout_chi2.p;
    kp.out_S = ctx->dout_S.p; kp.out_Q = ctx->dout_Q.p; kp.out_niter = ctx->dout_niter.p;
    kp.out_conv = ctx->dout_conv.p; kp.out_nevals = ctx->dout_nevals.p;
    kp.maxiter = o.maxiter; kp.miniter = o.miniter;
    kp.tol_h = o.tol_h; kp.tol_d = o.tol_d; kp.tol_relq = o.tol_relq; kp.stop_estimate = o.stop_estimate != 0;
    kp.step_max = o.step_max; kp.mu_first = o.mu_first; kp.mu_grow = o.mu_grow; kp.mu_max = o.mu_max;
    kp.theta = o.decouple_tol; kp.out_nact = ctx->dout_nact.p;
    kp.prof = nullptr;
    kp.gstate = nullptr;
    kp.mc_maxiter = std::min(o.maxiter, std::max(MC_MAXITER, o.miniter + 8));     // (a caller's miniter above the limit moves it)
    kp.mc_abandon = 1;
    kp.mc_maxevals = env.has_mc_maxevals ? env.mc_maxevals : 3 * kp.mc_maxiter;
    kp.prob_maxiter = nullptr;
    kp.out_index = nullptr;
    kp.dbg_hist = nullptr;
    kp.stuck_skip = env.stuck_skip;
}
// other pieces for the kernel parameters of the staged chains (the second pass of a two-pass launch, the finishing pass): n
// plain pieces -- nothing led, no walk, no start states -- whose start vectors are the rows v0[v0_row[.]]
static void set_pieces(KParams& kp, int n, const int* elem, const int* prob0, const int* len, const int* v0_row, const double* v0)
{
    kp.chain_elem = elem; kp.chain_prob0 = prob0; kp.chain_len = len; kp.chain_v0 = v0_row; kp.v0 = v0;
    kp.chain_lead = nullptr; kp.init_tab = nullptr; kp.chain_init = nullptr; kp.chain_walk0 = nullptr; kp.walk_alpha = nullptr;
    kp.n_chain = n;
}
// a one-chain build with its state in device memory: five omega arrays per chain (binary32 build: half of it used)
static int one_chain_state(mxe_ctx* ctx, const mxe::KernelBuild& b, KParams& kp)
{
    if (!b.gst) return MXE_OK;
    HIPCHK(ctx, ctx->dgstate.ensure((size_t)kp.n_chain * 5 * ctx->nwp));
    kp.gstate = ctx->dgstate.p;
    return MXE_OK;
}

namespace {
// one workgroup per problem the lock-step launch leaves out: its records say so until mxe_chains_finish has solved it
// (H, chi2, S, Q = NaN, not converged, no iterations; v = the start vector of its scan, where a chain that begins
// at the head of a scan starts from)
__global__ __launch_bounds__(256)
void clear_excluded_kernel(const int* __restrict__ idx, int n_alpha, int n_omega, int NP, const double* __restrict__ v0,
                           double* __restrict__ H, double* __restrict__ chi2, double* __restrict__ S, double* __restrict__ Q,
                           double* __restrict__ v, int* __restrict__ niter, int* __restrict__ conv, int* __restrict__ nevals, int* __restrict__ nact)
{
    const size_t pidx = (size_t)idx[blockIdx.x];
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < n_omega; i += blockDim.x) H[pidx * n_omega + i] = nan;
    const size_t chain = pidx / n_alpha;
    for (int k = threadIdx.x; k < NP; k += blockDim.x) v[pidx * NP + k] = v0[chain * NP + k];
    if (threadIdx.x == 0) { chi2[pidx] = nan; S[pidx] = nan; Q[pidx] = nan; niter[pidx] = 0; conv[pidx] = 0; nevals[pidx] = 0; nact[pidx] = 0; }
}
// the iteration counts of a two-pass launch (chain_kernel_lv, then chain_kernel_mc per alpha): both passes
__global__ __launch_bounds__(256)
void add_counts_kernel(int* __restrict__ niter, int* __restrict__ nevals, const int* __restrict__ niter1, const int* __restrict__ nevals1, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { niter[i] += niter1[i]; nevals[i] += nevals1[i]; }
}
}  // namespace

namespace {
// Diagnostic (MXE_POISON_LDS = 1: NaN, 2: a pattern of finite values that changes from launch to launch): every CU's LDS is
// written over before a chain kernel starts, so that nothing can lean on what an earlier kernel left there -- the LDS is not
// cleared between kernels, and a read of a cell nobody wrote gives the same answer run after run until the launches before it
// change.  One workgroup of the full 160 KB per CU, and a second wave of them for good measure.
__global__ __launch_bounds__(256)
void scribble_lds_kernel(unsigned long long pattern, int words, unsigned long long* sink)
{
    extern __shared__ unsigned long long sl[];
    for (int i = threadIdx.x; i < words; i += 256) sl[i] = pattern ? (0x3ff0000000000000ull | ((pattern + (unsigned long long)i * 0x9E3779B97F4A7C15ull) & 0x000fffffffffffffull)) : 0x7ff8000000000000ull;
    __syncthreads();
    if (sink && sl[(threadIdx.x * 7) % words] == 1) sink[0] = 1;       // (keeps the stores)
    __builtin_amdgcn_s_sleep(64);
}
hipError_t scribble_lds(hipStream_t s, int mode)
{
    if (!mode) return hipSuccess;
    static unsigned long long launches = 0;
    const int bytes = 160 * 1024;
    hipError_t e = hipFuncSetAttribute((const void*)scribble_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    ++launches;
    const unsigned long long pat = mode == 1 ? 0ull : (launches * 0x2545F4914F6CDD1Dull | 1ull);
    hipLaunchKernelGGL(scribble_lds_kernel, dim3(512), dim3(256), bytes, s, pat, bytes / 8, (unsigned long long*)nullptr);
    return hipGetLastError();
}
}  // namespace

// tolerance of the binary32 first pass of a two-pass launch: far enough above the rounding floor of h = V^T H in binary32
// (~2e-7 of |H|) to be reached without crawling, close enough for ONE binary64 Newton step to land below 1e-9
constexpr double LV_TOL1 = 1e-5;

// ---- What the three paths of mxe_chains_launch share.
// what a lock-step or lv kernel is handed besides KParams; the path sets the counter word, the rounds table and the state
static mxe::MCExtra mc_extra(const mxe_ctx* ctx)
{
    mxe::MCExtra ex;
    ex.wg_chains = ctx->dwg_chains.p; ex.n_wg = ctx->n_wg;
    ex.queue = ctx->dqueue.p; ex.n_queue = ctx->n_queue; ex.counter = nullptr;
    ex.stagger = 0;              // (a late start of the second half of the grid never paid: 0 ... 14 units measured; 5 cost 0.4 %; with the wave priorities of r03: 0 ... 24 units all within 0.5 %)
    ex.n_solo = 0; ex.gstate = nullptr; ex.gstate_stride = 0;
    return ex;
}
// sizes and clears the rounds per workgroup (mxe_launch_depth) of a launch of n0 workgroups and a second pass of n1; none: no node
static int arm_rounds(mxe_ctx* ctx, int n0, int n1)
{
    ctx->rounds_n[0] = n0; ctx->rounds_n[1] = n1;
    if (n0 + n1 == 0) return MXE_OK;
    HIPCHK(ctx, ctx->drounds.ensure((size_t)n0 + n1));
    HIPCHK(ctx, hipMemsetAsync(ctx->drounds.p, 0, ((size_t)n0 + n1) * sizeof(int), ctx->stream));
    return MXE_OK;
}
// what mxe_last_launch_info and mxe_last_kernel_name report (a two-pass launch: the waves and the LDS of its first pass)
static void record_build(mxe_ctx* ctx, const mxe::KernelBuild& b, const std::string& name)
{
    ctx->last_nw = b.waves(); ctx->last_lds = (int)b.lds; ctx->last_kernel = name;
}

// V^T resident in LDS as binary32 (mxe_kernel_lv.hip.h): the launch itself (precision = F32) or the first pass of a binary64
// launch that does not fill the GPU, whose second pass takes every alpha as a piece of its own in the binary64 lock-step
// kernel, from the v of the first
static int launch_lv(mxe_ctx* ctx, const mxe::LaunchEnv& env, const KParams& kp)
{
    const bool two_pass = ctx->lv_mode == 2;
    const mxe::KernelBuild b1 = mxe::lv_build(ctx->n_s, ctx->nwp);
    mxe::KernelBuild b2;
    if (two_pass) {
        if (const int rc = mxe::lockstep_build(32, ctx->wgpc2, false, false, ctx->nwp, 0, b2); rc != MXE_OK) return rc;
        if (mxe::build_index(b2) < 0) return MXE_ERR_STATE;
    }
    mxe::MCExtra ex = mc_extra(ctx);
    // (words 2 and 3, one per pass, zeroed by a reset node as before: the pair of the lock-step launches is not touched.  The
    //  second pass -- chain_kernel_mc drawing from word 3 -- stores its 0 into word 2, which the first pass has finished with.)
    ex.counter = ctx->dcounter.p + 2;
    HIPCHK(ctx, hipMemsetAsync(ctx->dcounter.p + 2, 0, 2 * sizeof(int), ctx->stream));
    if (const int rc = arm_rounds(ctx, ctx->n_wg, two_pass ? ctx->n_wg2 : 0); rc != MXE_OK) return rc;
    if (ex.n_queue > 0) ex.wg_chains = ctx->drounds.p;          // (dynamic layout: the rounds of every workgroup come back here)
    else ctx->rounds_n[0] = 0;
    KParams k1 = kp;
    if (two_pass) {
        k1.tol_h = std::max(kp.tol_h, LV_TOL1);
        k1.out_H = nullptr;
        k1.out_niter = ctx->dcnt1_niter.p; k1.out_nevals = ctx->dcnt1_nevals.p;
    }
    record_build(ctx, b1, two_pass ? mxe::two_pass_name(b1, b2) : mxe::build_name(b1));
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (const int rc = launch_build(ctx, env, b1, ctx->n_wg, k1, &ex); rc != MXE_OK) return rc;
    if (!two_pass) return MXE_OK;
    const size_t Pn = (size_t)ctx->n_chain * ctx->n_alpha;
    KParams k2 = kp;
    set_pieces(k2, (int)Pn, ctx->d2_elem.p, ctx->d2_prob0.p, ctx->d2_len.p, ctx->d2_v0.p, ctx->dout_v.p);
    k2.prof = nullptr;                  // (diagnostic build: the stamps of the first pass stay)
    mxe::MCExtra e2 = ex;
    e2.n_wg = ctx->n_wg2;
    e2.queue = ctx->d2_queue.p; e2.n_queue = (int)Pn; e2.counter = ctx->dcounter.p + 3;
    e2.wg_chains = ctx->drounds.p + ctx->rounds_n[0];
    if (const int rc = launch_build(ctx, env, b2, ctx->n_wg2, k2, &e2); rc != MXE_OK) return rc;
    hipLaunchKernelGGL(add_counts_kernel, dim3((unsigned)((Pn + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->dout_niter.p, ctx->dout_nevals.p, ctx->dcnt1_niter.p, ctx->dcnt1_nevals.p, (int)Pn);
    HIPCHK(ctx, hipGetLastError());
    return MXE_OK;
}

// four chains per workgroup, lock-step (mxe_kernel_mc.hip.h)
static int launch_lockstep(mxe_ctx* ctx, const mxe::LaunchEnv& env, const KParams& kp)
{
    const bool lead = kp.chain_lead != nullptr;
    mxe::KernelBuild b;
    if (const int rc = mxe::lockstep_build(ctx->mc_na, ctx->mc_wgpc, lead, ctx->mc_gst, ctx->nwp, ctx->opts.waves_per_chain, b); rc != MXE_OK) return rc;
    if (mxe::build_index(b) < 0) return MXE_ERR_STATE;
    mxe::MCExtra ex = mc_extra(ctx);
    if (b.gst) {
        ex.gstate_stride = mxe::mc_gstate_doubles(ctx->nwp);
        HIPCHK(ctx, ctx->dgstate_mc.ensure((size_t)ctx->n_wg * ex.gstate_stride + 4096));
        ex.gstate = ctx->dgstate_mc.p;
    }
    ex.counter = ctx->dcounter.p + ctx->counter_par;
    // rounds per workgroup (mxe_launch_depth): the builds for launches that do not fill the GPU write them, in the dynamic
    // layout (MCExtra: the pointer is the table of chain ids in the static one).  Not <32, 2> without led pieces -- the batch
    // that fills the GPU: the memset node alone is 1.5 us of its 812 (A/B: profiles/r04_experiments.txt)
    // (MXE_COUNT_ROUNDS: there as well -- a diagnostic launch, bench.py: launch_depth)
    const bool counts = ex.n_queue > 0 && (lead || b.WGPC == 1 || env.count_rounds);
    if (const int rc = arm_rounds(ctx, counts ? ctx->n_wg : 0, 0); rc != MXE_OK) return rc;
    if (counts) ex.wg_chains = ctx->drounds.p;
    int counter0 = 0;
    if (ex.n_queue > 0 && b.WGPC == 2 && ctx->n_solo > 0) {
        ex.n_solo = ctx->n_solo;
        counter0 = (ctx->n_wg - ex.n_solo) * 4;
    }
    // No reset node: launch k draws from word k & 1 of the pair, which mxe_chains_upload (k = 0, 1) or launch k - 1 set to counter0.
    // (Never taken: a launch whose start value is not the one the pair is armed with sets both words itself.)
    if (ctx->counter_armed != counter0) {
        HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->dcounter.p, counter0, 2, ctx->stream));
        ctx->counter_armed = counter0;
    }
    if (!ctx->excluded.empty()) {
        hipLaunchKernelGGL(clear_excluded_kernel, dim3((unsigned)ctx->excluded.size()), dim3(256), 0, ctx->stream,
                           ctx->dexcluded.p, ctx->n_alpha, ctx->n_omega, ctx->NP, ctx->dv0.p, ctx->dout_H.p, ctx->dout_chi2.p,
                           ctx->dout_S.p, ctx->dout_Q.p, ctx->dout_v.p, ctx->dout_niter.p, ctx->dout_conv.p,
                           ctx->dout_nevals.p, ctx->dout_nact.p);
        HIPCHK(ctx, hipGetLastError());
    }
    record_build(ctx, b, mxe::build_name(b));
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (const int rc = launch_build(ctx, env, b, ctx->n_wg, kp, &ex); rc != MXE_OK) return rc;
    ctx->counter_par ^= 1;       // (only behind a launch that was enqueued: a failed one re-armed nothing)
    return MXE_OK;
}

// one chain per workgroup (mxe_kernel.hip.h)
static int launch_one_chain(mxe_ctx* ctx, const mxe::LaunchEnv& env, KParams& kp)
{
    mxe::KernelBuild b;
    const bool f32 = ctx->opts.precision == MXE_PRECISION_F32;
    if (const int rc = mxe::one_chain_build(ctx->NP, ctx->nwp, mxe::first_waves(ctx->opts.waves_per_chain, ctx->n_sub), 1, f32, b); rc != MXE_OK) return rc;
    if (mxe::build_index(b) < 0) return MXE_ERR_STATE;
    if (const int rc = arm_rounds(ctx, 0, 0); rc != MXE_OK) return rc;
    if (const int rc = one_chain_state(ctx, b, kp); rc != MXE_OK) return rc;
    record_build(ctx, b, mxe::build_name(b));
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return launch_build(ctx, env, b, kp.n_chain, kp, nullptr);
}

// Launches the staged chains: check, choose the build (mxe_plan.h), arm what the kernel draws from, launch
int mxe_chains_launch(mxe_ctx* ctx)
try {
    if (!ctx) return MXE_ERR_ARG;
    if (!ctx->chains_ready) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->pre_d = nullptr; ctx->pre_i = nullptr; ctx->pre_rows = nullptr; ctx->pre_index = false;
    mxe::LaunchEnv env;
    read_launch_env(env);
    KParams kp;
    fill_kparams(ctx, env, kp);
    HIPCHK(ctx, scribble_lds(ctx->stream, env.poison_lds));      // (diagnostic, MXE_POISON_LDS)
    if (env.count_rounds && ctx->mc_na > 0 && kp.chain_lead == nullptr && ctx->lv_mode == 0) {
        // a diagnostic launch that counts the rounds of its workgroups (mxe_launch_depth) also where the shipped build does not --
        // <32, 2> without led pieces compiles the store out --: the build for led pieces with no piece led, the same schedule
        HIPCHK(ctx, hipMemsetAsync(ctx->dsub_pre.p, 0, (size_t)std::max(ctx->n_sub, 1) * sizeof(int), ctx->stream));
        kp.chain_lead = ctx->dsub_pre.p;
    }
#ifdef MXE_PROFILE
    HIPCHK(ctx, ctx->dprof.ensure(((size_t)ctx->n_sub + 8 * 1024) * 8));   // rows: chain (v2) or workgroup*8 + wave (lock-step)
    HIPCHK(ctx, hipMemsetAsync(ctx->dprof.p, 0, ((size_t)ctx->n_sub + 8 * 1024) * 64, ctx->stream));
    kp.prof = ctx->dprof.p;
#endif
    const int rc = ctx->mc_na == 0 ? launch_one_chain(ctx, env, kp) : ctx->lv_mode != 0 ? launch_lv(ctx, env, kp) : launch_lockstep(ctx, env, kp);
    if (rc != MXE_OK) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->launched = true;
    return MXE_OK;
}
MXE_CATCH_ALL

int mxe_sync(mxe_ctx* ctx)
{
    if (!ctx) return MXE_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}

// Alphas that the lock-step layout gave up on are solved again in the one-chain layout, from the state they were
// left in.  The lock-step kernel forms its Gram matrices from binary16 products (21 bits): an inexact
// Newton matrix that costs nothing where the system is well conditioned and stalls the iteration where it is not
// (few data points, small alpha: tens to hundreds of iterations per alpha where the binary64 Gram matrix of the
// one-chain kernel takes five); it stops an alpha after MC_MAXITER iterations.  Blocking; a no-op after a launch of
// the one-chain layout and when everything converged.  Which alphas, as which warm chains, over which rungs and with what
// budgets is decided by mxe::plan_finish (mxe_plan.h) from numbers alone; this function checks, reads the records back,
// asks, and carries the plan out.
int mxe_chains_finish(mxe_ctx* ctx, int32_t* n_resolved)
try {
    // ---- 1. checks
    if (n_resolved) *n_resolved = 0;
    if (!ctx) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    if (ctx->mc_na == 0) return MXE_OK;                       // the launch was in the one-chain layout
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, stream_wait(ctx->stream));
    // ---- 2. the records of the lock-step pass (the flags first: when everything converged nothing else is read)
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    const int NP = ctx->NP;
    std::vector<int> conv(P), nit(P), nev(P);
    HIPCHK(ctx, hipMemcpy(conv.data(), ctx->dout_conv.p, P * sizeof(int), hipMemcpyDeviceToHost));
    if (std::find(conv.begin(), conv.end(), 0) == conv.end()) return MXE_OK;
    std::vector<double> halpha(P);
    HIPCHK(ctx, hipMemcpy(nit.data(), ctx->dout_niter.p, P * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(nev.data(), ctx->dout_nevals.p, P * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(halpha.data(), ctx->dalpha.p, P * sizeof(double), hipMemcpyDeviceToHost));
    // ---- 3. the plan
    std::vector<int> chain_rows(ctx->n_chain);
    for (int c = 0; c < ctx->n_chain; ++c) chain_rows[c] = ctx->ds[ctx->elem_ds[ctx->chain_elem[c]]].n_rows;
    mxe::FinishInput in;
    in.n_chain = ctx->n_chain; in.n_alpha = ctx->n_alpha; in.maxiter = ctx->opts.maxiter;
    in.alpha = halpha.data(); in.converged = conv.data(); in.n_iter = nit.data(); in.n_evals = nev.data();
    in.chain_elem = ctx->chain_elem.data(); in.chain_rows = chain_rows.data();
    read_finish_env(in.env);
    mxe::FinishPlan plan;
    mxe::plan_finish(in, plan);
    if (plan.n_open == 0) return MXE_OK;
    ctx->pre_d = nullptr; ctx->pre_i = nullptr; ctx->pre_rows = nullptr; ctx->pre_index = false;   // (what was copied out behind the launch is about to change)
    // ---- 4. the runs as pieces of the one-chain kernel: one upload per array, start vectors (whitened basis, row stride NP)
    const int nr = (int)plan.runs.size();
    std::vector<int> f_elem(nr), f_prob0(nr), f_len(nr), f_v0(nr);
    for (int k = 0; k < nr; ++k) { const mxe::FinishRun& r = plan.runs[k]; f_elem[k] = r.elem; f_prob0[k] = r.entry0; f_len[k] = r.len; f_v0[k] = k; }
    HIPCHK(ctx, put(ctx, ctx->dfin_elem, f_elem)); HIPCHK(ctx, put(ctx, ctx->dfin_prob0, f_prob0));
    HIPCHK(ctx, put(ctx, ctx->dfin_len, f_len)); HIPCHK(ctx, put(ctx, ctx->dfin_v0, f_v0));
    HIPCHK(ctx, put(ctx, ctx->dfin_alpha, plan.entry_alpha)); HIPCHK(ctx, put(ctx, ctx->dfin_out, plan.entry_out));
    HIPCHK(ctx, put(ctx, ctx->dfin_budget, plan.entry_budget));
    HIPCHK(ctx, ctx->dfin_start.ensure((size_t)nr * NP));
    for (int k = 0; k < nr; ++k) {
        const mxe::FinishStart& st = plan.runs[k].start;
        const double* from = (st.from_v0 ? ctx->dv0.p : ctx->dout_v.p) + (size_t)st.index * NP;
        HIPCHK(ctx, hipMemcpyAsync(ctx->dfin_start.p + (size_t)k * NP, from, NP * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIPCHK(ctx, stream_wait(ctx->stream));          // (the host vectors are locals)
    mxe::LaunchEnv env;
    read_launch_env(env);
    KParams kp;
    fill_kparams(ctx, env, kp);
    set_pieces(kp, nr, ctx->dfin_elem.p, ctx->dfin_prob0.p, ctx->dfin_len.p, ctx->dfin_v0.p, ctx->dfin_start.p);
    kp.alpha = ctx->dfin_alpha.p; kp.out_index = ctx->dfin_out.p; kp.prob_maxiter = ctx->dfin_budget.p;
#ifdef MXE_DEBUG_HIST
    const size_t ne = plan.entry_alpha.size();
    DevBuf<double> dhist;
    if (getenv("MXE_DEBUG_HIST_FILE")) {
        HIPCHK(ctx, dhist.ensure(ne * 48));
        HIPCHK(ctx, hipMemsetAsync(dhist.p, 0, ne * 48 * sizeof(double), ctx->stream));
        kp.dbg_hist = dhist.p;
    }
#endif
#ifdef MXE_PROFILE
    // (diagnostic build: the stamps of THIS pass, rows 0 .. nr - 1 -- tools/finish_phases.py; those of the lock-step launch are gone)
    if (ctx->dprof.p && (size_t)nr <= (size_t)ctx->n_sub + 8 * 1024) {
        HIPCHK(ctx, hipMemsetAsync(ctx->dprof.p, 0, ((size_t)ctx->n_sub + 8 * 1024) * 64, ctx->stream));
        kp.prof = ctx->dprof.p;
    }
#endif
    // ---- 5. the launch: binary64, four waves per chain whatever the mesh (a frequency mesh beyond the LDS -- the lock-step
    // launch kept its state in device memory --: so does this one)
    HIPCHK(ctx, scribble_lds(ctx->stream, env.poison_lds));      // (diagnostic, MXE_POISON_LDS)
    mxe::KernelBuild b;
    if (const int rc = mxe::one_chain_build(NP, ctx->nwp, 4, 4, false, b); rc != MXE_OK) return rc;
    if (const int rc = one_chain_state(ctx, b, kp); rc != MXE_OK) return rc;
    if (const int rc = launch_build(ctx, env, b, kp.n_chain, kp, nullptr); rc != MXE_OK) return rc;
    HIPCHK(ctx, stream_wait(ctx->stream));
#ifdef MXE_DEBUG_HIST
    if (kp.dbg_hist) {
        std::vector<double> hh(ne * 48);
        HIPCHK(ctx, hipMemcpy(hh.data(), dhist.p, ne * 48 * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<int> cv(P);
        HIPCHK(ctx, hipMemcpy(cv.data(), ctx->dout_conv.p, P * sizeof(int), hipMemcpyDeviceToHost));
        std::vector<int> ni(P);
        HIPCHK(ctx, hipMemcpy(ni.data(), ctx->dout_niter.p, P * sizeof(int), hipMemcpyDeviceToHost));
        if (FILE* f = fopen(getenv("MXE_DEBUG_HIST_FILE"), "a")) {
            for (size_t en = 0; en < ne; ++en) {
                const int out = plan.entry_out[en];
                if (out < 0) continue;
                fprintf(f, "%d %d %d %.6e", out, cv[out], ni[out], plan.entry_alpha[en]);
                for (int m = 0; m < 48; ++m) fprintf(f, "%s%.3e", (m % 16 == 0) ? " | " : " ", hh[en * 48 + m]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
        dhist.release();
    }
#endif
    // ---- 6. the counters of the records: both passes (whole arrays: one copy each way)
    std::vector<int> nit2(P), nev2(P);
    HIPCHK(ctx, hipMemcpy(nit2.data(), ctx->dout_niter.p, P * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(nev2.data(), ctx->dout_nevals.p, P * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < P; ++i) if (plan.open[i]) { nit2[i] += nit[i]; nev2[i] += nev[i]; }
    HIPCHK(ctx, hipMemcpy(ctx->dout_niter.p, nit2.data(), P * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->dout_nevals.p, nev2.data(), P * sizeof(int), hipMemcpyHostToDevice));
    if (n_resolved) *n_resolved = plan.n_open;
    return MXE_OK;
}
MXE_CATCH_ALL

int mxe_chains_fetch(mxe_ctx* ctx, double* out_v, double* out_H, double* out_chi2,
                     double* out_S, double* out_Q, int32_t* out_niter,
                     int32_t* out_converged, int32_t* out_nevals)
try {
    if (!ctx) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, stream_wait(ctx->stream));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    const int ns = ctx->n_s, NP = ctx->NP, nw = ctx->n_omega;
    if (out_H) HIPCHK(ctx, d2h_pipelined(out_H, ctx->dout_H.p, P * nw * 8, ctx->stream));
    // (chi2 | S | Q and niter | converged | nevals are one block each on the device: a caller whose arrays lie the same way --
    //  maxent_amd.device.DeviceContext.fetch allocates them so -- gets each block in ONE copy; six copies of 100-200 KB
    //  cost 0.15 ms behind a launch of 0.8 ms)
    const bool pre = ctx->pre_d && out_chi2 == ctx->pre_d && out_S == out_chi2 + P && out_Q == out_S + P &&
                     out_niter == ctx->pre_i && out_converged == out_niter + P && out_nevals == out_converged + P;
    if (pre) {}                                  // (mxe_chains_prefetch queued both blocks behind the launch: they are there)
    else if (out_chi2 && out_S == out_chi2 + P && out_Q == out_S + P)
        HIPCHK(ctx, hipMemcpy(out_chi2, ctx->dout_chi2.p, 3 * P * 8, hipMemcpyDeviceToHost));
    else {
        if (out_chi2) HIPCHK(ctx, hipMemcpy(out_chi2, ctx->dout_chi2.p, P * 8, hipMemcpyDeviceToHost));
        if (out_S) HIPCHK(ctx, hipMemcpy(out_S, ctx->dout_S.p, P * 8, hipMemcpyDeviceToHost));
        if (out_Q) HIPCHK(ctx, hipMemcpy(out_Q, ctx->dout_Q.p, P * 8, hipMemcpyDeviceToHost));
    }
    if (out_Q && ctx->chi2_factor != 1.0 && !(pre && ctx->pre_scaled)) for (size_t i = 0; i < P; ++i) out_Q[i] *= ctx->chi2_factor;
    if (pre) ctx->pre_scaled = true;
    if (pre) {}
    else if (out_niter && out_converged == out_niter + P && out_nevals == out_converged + P)
        HIPCHK(ctx, hipMemcpy(out_niter, ctx->dout_niter.p, 3 * P * 4, hipMemcpyDeviceToHost));
    else {
        if (out_niter) HIPCHK(ctx, hipMemcpy(out_niter, ctx->dout_niter.p, P * 4, hipMemcpyDeviceToHost));
        if (out_converged) HIPCHK(ctx, hipMemcpy(out_converged, ctx->dout_conv.p, P * 4, hipMemcpyDeviceToHost));
        if (out_nevals) HIPCHK(ctx, hipMemcpy(out_nevals, ctx->dout_nevals.p, P * 4, hipMemcpyDeviceToHost));
    }
    if (out_v) {
        std::vector<double> hv(P * NP);
        HIPCHK(ctx, hipMemcpy(hv.data(), ctx->dout_v.p, P * NP * 8, hipMemcpyDeviceToHost));
        for (size_t pidx = 0; pidx < P; ++pidx) {
            const int chain = (int)(pidx / ctx->n_alpha);
            const DataSet& DS = ctx->ds[ctx->elem_ds[ctx->chain_elem[chain]]];
            for (int k = 0; k < ns; ++k) {
                double s;
                if (DS.identity_q) s = hv[pidx * NP + k];
                else {   // v = Q v'
                    s = 0.0;
                    for (int j = 0; j < ns; ++j) s += DS.Q[(size_t)k * ns + j] * hv[pidx * NP + j];
                }
                out_v[pidx * ns + k] = s;
            }
        }
    }
    return MXE_OK;
}
MXE_CATCH_ALL

namespace {
// Results written into page-locked host memory by the compute queue (mxe_chains_prefetch, mxe_select3_prefetch_rows).  A
// hipMemcpyAsync behind a kernel parks a DMA engine until that kernel is through, and the uploads of the NEXT job (new data on
// another context's stream) queued up behind it: mxe_elements_update_data took 0.9 ms instead of 0.3 with four jobs in flight.
struct CopySeg { const uint32_t* src; uint32_t* dst; size_t words; };
__global__ __launch_bounds__(256)
void copy_out_kernel(CopySeg a, CopySeg b)
{
    const size_t stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = t0; i < a.words; i += stride) a.dst[i] = a.src[i];
    for (size_t i = t0; i < b.words; i += stride) b.dst[i] = b.src[i];
}
hipError_t copy_out(void* dst_a, const void* src_a, size_t bytes_a, void* dst_b, const void* src_b, size_t bytes_b, bool mapped, hipStream_t s)
{
    if (!mapped || (bytes_a & 3) || (bytes_b & 3)) {
        hipError_t e = bytes_a ? hipMemcpyAsync(dst_a, src_a, bytes_a, hipMemcpyDeviceToHost, s) : hipSuccess;
        if (e == hipSuccess && bytes_b) e = hipMemcpyAsync(dst_b, src_b, bytes_b, hipMemcpyDeviceToHost, s);
        return e;
    }
    CopySeg a{(const uint32_t*)src_a, (uint32_t*)dst_a, bytes_a / 4}, b{(const uint32_t*)src_b, (uint32_t*)dst_b, bytes_b / 4};
    const size_t words = std::max(a.words, b.words);
    const int blocks = (int)std::min<size_t>(64, (words + 255) / 256);
    hipLaunchKernelGGL(copy_out_kernel, dim3(std::max(blocks, 1)), dim3(256), 0, s, a, b);
    return hipGetLastError();
}
}

int mxe_chains_prefetch(mxe_ctx* ctx, double* out_chi2_S_Q, int32_t* out_niter_converged_nevals)
try {
    if (!ctx || !out_chi2_S_Q || !out_niter_converged_nevals) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    ctx->pre_d = nullptr; ctx->pre_i = nullptr;
    const bool mapped = g_host.holds(out_chi2_S_Q, 3 * P * 8) && g_host.holds(out_niter_converged_nevals, 3 * P * 4);
    HIPCHK(ctx, copy_out(out_chi2_S_Q, ctx->dout_chi2.p, 3 * P * 8, out_niter_converged_nevals, ctx->dout_niter.p, 3 * P * 4, mapped, ctx->stream));
    ctx->pre_d = out_chi2_S_Q; ctx->pre_i = out_niter_converged_nevals; ctx->pre_scaled = false;
    return MXE_OK;
}
MXE_CATCH_ALL

int mxe_chains_fetch_nact(mxe_ctx* ctx, int32_t* out_nact)
{
    if (!ctx || !out_nact) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, stream_wait(ctx->stream));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    HIPCHK(ctx, hipMemcpy(out_nact, ctx->dout_nact.p, P * 4, hipMemcpyDeviceToHost));
    return MXE_OK;
}

int mxe_solve_chains(mxe_ctx* ctx, int n_chain, int n_alpha,
                     const int32_t* elem_of_chain, const double* alpha_scaled,
                     const double* v0, const mxe_opts* opts,
                     double* out_v, double* out_H, double* out_chi2,
                     double* out_S, double* out_Q, int32_t* out_niter,
                     int32_t* out_converged, int32_t* out_nevals)
{
    int rc = mxe_chains_upload(ctx, n_chain, n_alpha, elem_of_chain, alpha_scaled, v0, opts);
    if (rc != MXE_OK) return rc;
    rc = mxe_chains_launch(ctx);
    if (rc != MXE_OK) return rc;
    rc = mxe_chains_finish(ctx, nullptr);
    if (rc != MXE_OK) return rc;
    return mxe_chains_fetch(ctx, out_v, out_H, out_chi2, out_S, out_Q, out_niter, out_converged, out_nevals);
}

int mxe_result_device_ptrs(mxe_ctx* ctx, void** d_H, void** d_chi2, void** d_S, void** d_Q,
                           void** d_v, void** d_niter, void** d_converged)
{
    if (!ctx) return MXE_ERR_ARG;
    if (!ctx->chains_ready) return MXE_ERR_STATE;
    if (d_H) *d_H = ctx->dout_H.p;
    if (d_chi2) *d_chi2 = ctx->dout_chi2.p;
    if (d_S) *d_S = ctx->dout_S.p;
    if (d_Q) *d_Q = ctx->dout_Q.p;
    if (d_v) *d_v = ctx->dout_v.p;
    if (d_niter) *d_niter = ctx->dout_niter.p;
    if (d_converged) *d_converged = ctx->dout_conv.p;
    return MXE_OK;
}

int mxe_ns_padded(mxe_ctx* ctx) { return ctx ? ctx->NP : MXE_ERR_ARG; }

int mxe_set_result_buffer(mxe_ctx* ctx, int which)
{
    if (!ctx || (which != 0 && which != 1)) return MXE_ERR_ARG;
    if (!ctx->chains_ready) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha, nw = ctx->n_omega;
    if (which == 1) HIPCHK(ctx, ctx->dout_pack2.ensure(P * nw + 3 * P + (size_t)ctx->n_chain * (nw + 1)));
    double* base = which ? ctx->dout_pack2.p : ctx->dout_pack.p;
    ctx->result_buffer = which;
    ctx->dout_H.p = base; ctx->dout_chi2.p = base + P * nw; ctx->dout_S.p = ctx->dout_chi2.p + P; ctx->dout_Q.p = ctx->dout_S.p + P;
    return MXE_OK;
}

int mxe_last_kernel_ms(mxe_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return MXE_OK;
}

const char* mxe_last_kernel_name(mxe_ctx* ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

void* mxe_stream(mxe_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int mxe_timing_mark(mxe_ctx* ctx)
{
    if (!ctx) return MXE_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventRecord(ctx->ev_mark, ctx->stream));
    return MXE_OK;
}

int mxe_ms_since_mark(mxe_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev_mark, ctx->ev1));
    return MXE_OK;
}

int mxe_last_launch_info(mxe_ctx* ctx, int* waves_per_chain, int* n_workgroups, int* lds_bytes)
{
    if (!ctx) return MXE_ERR_ARG;
    if (waves_per_chain) *waves_per_chain = ctx->last_nw;
    if (n_workgroups) *n_workgroups = ctx->n_wg;
    if (lds_bytes) *lds_bytes = ctx->last_lds;
    return MXE_OK;
}

int mxe_schedule_info(mxe_ctx* ctx, int* n_solo, int* placement_rule)
{
    if (!ctx) return MXE_ERR_ARG;
    if (n_solo) *n_solo = ctx->n_solo;
    if (placement_rule) *placement_rule = ctx->placement_checked;
    return MXE_OK;
}

// depth of the last lock-step launch in rounds (a round = one Newton iteration of the four slots of a workgroup): maximum and
// mean over its workgroups, [0] the launch (or its first pass), [1] the second pass of a two-pass launch (0 when there is none;
// both 0 after a launch of the one-chain layout).  Blocking.
int mxe_launch_depth(mxe_ctx* ctx, int32_t* max_rounds, double* mean_rounds)
try {
    if (!ctx || !max_rounds || !mean_rounds) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, stream_wait(ctx->stream));
    const size_t n = (size_t)ctx->rounds_n[0] + ctx->rounds_n[1];
    std::vector<int> h(n ? n : 1, 0);
    if (n) HIPCHK(ctx, hipMemcpy(h.data(), ctx->drounds.p, n * sizeof(int), hipMemcpyDeviceToHost));
    size_t off = 0;
    for (int k = 0; k < 2; ++k) {
        int mx = 0; double sum = 0.0; int busy = 0;
        for (int i = 0; i < ctx->rounds_n[k]; ++i) { mx = std::max(mx, h[off + i]); sum += h[off + i]; busy += h[off + i] > 0; }
        max_rounds[k] = mx; mean_rounds[k] = busy ? sum / busy : 0.0;
        off += ctx->rounds_n[k];
    }
    return MXE_OK;
}
MXE_CATCH_ALL

} // extern "C"

#ifdef MXE_PROFILE
// diagnostic build only: per-chain phase cycle counters of the last launch
extern "C" int mxe_prof_fetch(mxe_ctx* ctx, long long* out /*[n_sub + 8192][8]*/)
{
    if (!ctx || !out) return MXE_ERR_ARG;
    HIPCHK(ctx, stream_wait(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, ctx->dprof.p, ((size_t)ctx->n_sub + 8 * 1024) * 64, hipMemcpyDeviceToHost));
    return MXE_OK;
}
// the stamps of the last mxe_select_launch / mxe_select3_launch
extern "C" int mxe_prof_linefit_fetch(mxe_ctx* ctx, long long* out /*[n_chain][4][10]*/)
{
    if (!ctx || !out) return MXE_ERR_ARG;
    if (!ctx->dprof_lf.p) return MXE_ERR_STATE;
    HIPCHK(ctx, stream_wait(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, ctx->dprof_lf.p, (size_t)ctx->n_chain * 40 * sizeof(long long), hipMemcpyDeviceToHost));
    return MXE_OK;
}
#endif

// ---- the kernels that factorise B = c W c + a I per problem (mxe_factor.hip.h): logdet, posterior variances, samples ----
#include "mxe_factor.hip.h"

// one workgroup per problem with lds bytes of dynamic LDS; k4 / k8: the 64-row and the 128-row build of the kernel
template <typename... KArgs, typename... Args>
static hipError_t launch_factor_kernel(void (*k4)(KArgs...), void (*k8)(KArgs...), const mxe_ctx* ctx, size_t P, size_t lds,
                                       Args... args)
{
    return launch_lds(ctx->NP == 64 ? k4 : k8, dim3((unsigned)P), dim3(256), lds, ctx->stream, args...);
}

extern "C" int mxe_logdet(mxe_ctx* ctx, double* out_logdet)
try {
    if (!ctx || !out_logdet) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    HIPCHK(ctx, ctx->dlogdet.ensure(P));
    HIPCHK(ctx, ctx->dparent_elem.ensure(ctx->chain_elem.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dparent_elem.p, ctx->chain_elem.data(), ctx->chain_elem.size() * sizeof(int),
                               hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = mxe::logdet_lds_bytes(ctx->NP, ctx->nwp);
    if (lds > 160 * 1024) return MXE_ERR_LIMIT;
    HIPCHK(ctx, launch_factor_kernel(mxe::logdet_kernel<4>, mxe::logdet_kernel<8>, ctx, P, lds,
                                     ctx->dV.p, ctx->dc.p, ctx->delem_ds.p, ctx->delem_kind.p, ctx->dD.p, ctx->dparent_elem.p,
                                     ctx->dalpha.p, ctx->dout_H.p, ctx->dlogdet.p, ctx->n_alpha, ctx->n_omega, ctx->nwp, ctx->n_s));
    HIPCHK(ctx, hipMemcpyAsync(out_logdet, ctx->dlogdet.p, P * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- cost function and derivatives at caller-supplied points; audit of a launch ----------
namespace {
size_t eval_lds_bytes(int NP, int nwp) { return ((size_t)NP * (NP + 1) + 2 * (size_t)nwp + 7 * (size_t)NP + 16) * sizeof(double); }

int launch_eval(mxe_ctx* ctx, const mxe::EvalParams& ep, size_t P)
{
    const size_t lds = eval_lds_bytes(ctx->NP, ctx->nwp);
    if (lds > 160 * 1024) return MXE_ERR_LIMIT;
    HIPCHK(ctx, launch_lds(ctx->NP == 64 ? mxe::eval_kernel<4> : mxe::eval_kernel<8>, dim3((unsigned)P), dim3(256), lds,
                           ctx->stream, ep));
    return MXE_OK;
}

void eval_params_base(mxe_ctx* ctx, mxe::EvalParams& ep)
{
    std::memset(&ep, 0, sizeof(ep));
    ep.nw = ctx->n_omega; ep.nwp = ctx->nwp; ep.ns = ctx->n_s; ep.NP = ctx->NP;
    ep.V = ctx->dV.p; ep.Vt = ctx->dVt.p; ep.c = ctx->dc.p;
    ep.elem_ds = ctx->delem_ds.p; ep.elem_kind = ctx->delem_kind.p;
    ep.ghat = ctx->dghat.p; ep.cperp = ctx->dcperp.p; ep.D = ctx->dD.p;
    ep.eta = 1.0; ep.elem_div = 1;
}
} // namespace

extern "C" int mxe_eval_batch(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                              const double* x, int input_is_H, double chi2_factor,
                              double* out_Q, double* out_chi2, double* out_S,
                              double* out_H, double* out_u, double* out_w, double* out_q,
                              double* out_h, double* out_g, double* out_W, double* out_W2)
try {
    if (!ctx || P < 1 || !elem_of_problem || !alpha_scaled || !x) return MXE_ERR_ARG;
    if (ctx->n_elem < 1) return MXE_ERR_STATE;
    if (!(chi2_factor > 0.0) || !std::isfinite(chi2_factor)) return MXE_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->ds_dirty) { int rc = upload_bases(ctx); if (rc != MXE_OK) return rc; }
    const int ns = ctx->n_s, NP = ctx->NP, nw = ctx->n_omega;
    const size_t xs = input_is_H ? (size_t)nw : (size_t)NP;
    std::vector<double> hx((size_t)P * xs, 0.0);
    for (int p = 0; p < P; ++p) {
        const int e = elem_of_problem[p];
        if (e < 0 || e >= ctx->n_elem) return MXE_ERR_ARG;
        if (!(alpha_scaled[p] >= 0.0) || !std::isfinite(alpha_scaled[p])) return MXE_ERR_ARG;
        if (input_is_H) { std::copy(x + (size_t)p * nw, x + (size_t)(p + 1) * nw, hx.begin() + (size_t)p * nw); continue; }
        const DataSet& DS = ctx->ds[ctx->elem_ds[e]];
        for (int k = 0; k < ns; ++k) {
            double s;
            if (DS.identity_q) s = x[(size_t)p * ns + k];
            else { s = 0.0; for (int j = 0; j < ns; ++j) s += DS.Q[(size_t)j * ns + k] * x[(size_t)p * ns + j]; }   // v' = Q^T v
            hx[(size_t)p * NP + k] = s;
        }
    }
    const bool wantW = out_W != nullptr, wantW2 = out_W2 != nullptr;
    HIPCHK(ctx, ctx->ev_x.ensure(hx.size()));
    HIPCHK(ctx, ctx->ev_alpha.ensure(P));
    HIPCHK(ctx, ctx->ev_elem.ensure(P));
    HIPCHK(ctx, ctx->ev_scal.ensure((size_t)5 * P));
    HIPCHK(ctx, ctx->ev_vecw.ensure((size_t)4 * P * nw));
    HIPCHK(ctx, ctx->ev_vecs.ensure((size_t)2 * P * NP));
    HIPCHK(ctx, ctx->ev_mat.ensure((size_t)(wantW ? 1 : 0) * P * NP * NP + (size_t)(wantW2 ? 1 : 0) * P * NP * NP));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ev_x.p, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ev_alpha.p, alpha_scaled, (size_t)P * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ev_elem.p, elem_of_problem, (size_t)P * 4, hipMemcpyHostToDevice, ctx->stream));
    mxe::EvalParams ep;
    eval_params_base(ctx, ep);
    ep.elem = ctx->ev_elem.p; ep.alpha = ctx->ev_alpha.p; ep.x = ctx->ev_x.p; ep.x_stride = (int)xs;
    ep.input_is_H = input_is_H ? 1 : 0; ep.eta = chi2_factor;
    ep.want_gram = wantW; ep.want_gram2 = wantW2;
    ep.Q = ctx->ev_scal.p; ep.chi2 = ep.Q + P; ep.S = ep.chi2 + P;
    ep.H = ctx->ev_vecw.p; ep.u = ep.H + (size_t)P * nw; ep.w = ep.u + (size_t)P * nw;
    ep.q = out_q ? ep.w + (size_t)P * nw : nullptr;
    ep.h = ctx->ev_vecs.p; ep.g = ep.h + (size_t)P * NP;
    ep.W = wantW ? ctx->ev_mat.p : nullptr;
    ep.W2 = wantW2 ? ctx->ev_mat.p + (size_t)(wantW ? 1 : 0) * P * NP * NP : nullptr;
    int rc = launch_eval(ctx, ep, (size_t)P);
    if (rc != MXE_OK) return rc;
    if (out_Q) HIPCHK(ctx, hipMemcpyAsync(out_Q, ep.Q, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_chi2) HIPCHK(ctx, hipMemcpyAsync(out_chi2, ep.chi2, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_S) HIPCHK(ctx, hipMemcpyAsync(out_S, ep.S, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_H) HIPCHK(ctx, hipMemcpyAsync(out_H, ep.H, (size_t)P * nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_u) HIPCHK(ctx, hipMemcpyAsync(out_u, ep.u, (size_t)P * nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_w) HIPCHK(ctx, hipMemcpyAsync(out_w, ep.w, (size_t)P * nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_q) HIPCHK(ctx, hipMemcpyAsync(out_q, ep.q, (size_t)P * nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> hh, hg, hW, hW2;
    if (out_h) { hh.resize((size_t)P * NP); HIPCHK(ctx, hipMemcpyAsync(hh.data(), ep.h, hh.size() * 8, hipMemcpyDeviceToHost, ctx->stream)); }
    if (out_g) { hg.resize((size_t)P * NP); HIPCHK(ctx, hipMemcpyAsync(hg.data(), ep.g, hg.size() * 8, hipMemcpyDeviceToHost, ctx->stream)); }
    if (wantW) { hW.resize((size_t)P * NP * NP); HIPCHK(ctx, hipMemcpyAsync(hW.data(), ep.W, hW.size() * 8, hipMemcpyDeviceToHost, ctx->stream)); }
    if (wantW2) { hW2.resize((size_t)P * NP * NP); HIPCHK(ctx, hipMemcpyAsync(hW2.data(), ep.W2, hW2.size() * 8, hipMemcpyDeviceToHost, ctx->stream)); }
    HIPCHK(ctx, stream_wait(ctx->stream));
    // whitened basis -> caller basis:  x = Q x',  X = Q X' Q^T
    std::vector<double> tmp((size_t)ns * ns);
    for (int p = 0; p < P; ++p) {
        const DataSet& DS = ctx->ds[ctx->elem_ds[elem_of_problem[p]]];
        auto vec_out = [&](const std::vector<double>& src, double* dst) {
            for (int k = 0; k < ns; ++k) {
                double s;
                if (DS.identity_q) s = src[(size_t)p * NP + k];
                else { s = 0.0; for (int j = 0; j < ns; ++j) s += DS.Q[(size_t)k * ns + j] * src[(size_t)p * NP + j]; }
                dst[(size_t)p * ns + k] = s;
            }
        };
        auto mat_out = [&](const std::vector<double>& src, double* dst) {
            const double* Xp = src.data() + (size_t)p * NP * NP;
            double* out = dst + (size_t)p * ns * ns;
            if (DS.identity_q) {
                for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) out[(size_t)i * ns + j] = Xp[(size_t)i * NP + j];
                return;
            }
            for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) {        // tmp = X' Q^T
                double s = 0.0;
                for (int k = 0; k < ns; ++k) s += Xp[(size_t)i * NP + k] * DS.Q[(size_t)j * ns + k];
                tmp[(size_t)i * ns + j] = s;
            }
            for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) {        // out = Q tmp
                double s = 0.0;
                for (int k = 0; k < ns; ++k) s += DS.Q[(size_t)i * ns + k] * tmp[(size_t)k * ns + j];
                out[(size_t)i * ns + j] = s;
            }
        };
        if (out_h) vec_out(hh, out_h);
        if (out_g) vec_out(hg, out_g);
        if (wantW) mat_out(hW, out_W);
        if (wantW2) mat_out(hW2, out_W2);
    }
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- posterior variances of linear functionals of H and draws from the posterior (mxe_postvar.hip.h, mxe_postsample.hip.h) ----
#include "mxe_postvar.hip.h"
#include "mxe_postsample.hip.h"

namespace {
// the problems of a posterior call as they go to the device
struct PostStage {
    size_t lds = 0;
    std::vector<double> ha;     // [P] alpha~ / eta
    std::vector<int> hi;        // [P] element | [P] row of H
};

// Checks the state and the problems (elem, alpha, chi2_factor, row) of the posterior calls, opens sg on the context
// and fills st; uploads the bases when they are stale.  n_max: the largest element count among the call's arrays;
// z: n_z host values (or NULL) that must be finite before the device is touched.
int stage_posterior(Stage& sg, mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled, const double* H,
                    const int32_t* problem_index, double chi2_factor, size_t n_max, const double* z, size_t n_z, PostStage& st)
{
    if (ctx->n_elem < 1) return MXE_ERR_STATE;
    if (!H && !ctx->launched) return MXE_ERR_STATE;
    if (!(chi2_factor > 0.0) || !std::isfinite(chi2_factor)) return MXE_ERR_ARG;
    if (n_max > 0x7fffffffull) return MXE_ERR_ARG;
    st.lds = mxe::postvar_lds_bytes(ctx->NP, ctx->nwp);
    if (st.lds > 160 * 1024) return MXE_ERR_LIMIT;
    if (z && !all_finite(z, n_z)) return MXE_ERR_ARG;
    if (int rc = sg.open(ctx); rc != MXE_OK) return rc;
    if (ctx->ds_dirty) if (int rc = upload_bases(ctx); rc != MXE_OK) return rc;
    st.ha.resize(P);
    st.hi.resize((size_t)2 * P);
    for (int p = 0; p < P; ++p) {
        const int e = elem_of_problem[p];
        if (e < 0 || e >= ctx->n_elem) return MXE_ERR_ARG;
        if (!(alpha_scaled[p] > 0.0) || !std::isfinite(alpha_scaled[p])) return MXE_ERR_ARG;
        st.ha[p] = alpha_scaled[p] / chi2_factor;
        st.hi[p] = e;
        st.hi[(size_t)P + p] = p;
    }
    if (!H && !launch_rows(problem_index, P, (size_t)ctx->n_chain * ctx->n_alpha, st.hi.data() + P)) return MXE_ERR_ARG;
    return MXE_OK;
}

// st and the H rows (when handed in) into the block of the call (alpha at dalpha, the rows at dH) and pv_i; fp: what
// the kernels share
int upload_posterior(Stage& sg, const PostStage& st, int P, const double* H, double* dalpha, double* dH, mxe::FactorParams& fp)
{
    mxe_ctx* ctx = sg.ctx;
    const int nw = ctx->n_omega;
    STGCHK(sg, ctx->pv_i.ensure((size_t)2 * P));
    STGCHK(sg, sg.upload(dalpha, st.ha.data(), (size_t)P)); STGCHK(sg, sg.upload(dH, H, (size_t)P * nw));
    STGCHK(sg, sg.upload(ctx->pv_i.p, st.hi.data(), st.hi.size()));
    fp.V = ctx->dV.p; fp.c = ctx->dc.p; fp.elem_ds = ctx->delem_ds.p; fp.elem_kind = ctx->delem_kind.p; fp.D = ctx->dD.p;
    fp.elem = ctx->pv_i.p; fp.alpha = dalpha;
    fp.H = H ? dH : ctx->dout_H.p; fp.row = H ? nullptr : ctx->pv_i.p + P;
    fp.nw = nw; fp.nwp = ctx->nwp; fp.ns = ctx->n_s;
    return MXE_OK;
}
} // namespace

extern "C" int mxe_posterior_var(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                                 const double* H, const int32_t* problem_index, double chi2_factor,
                                 int n_f, const double* F, double* out_var, double* out_diag, double* out_prior,
                                 float* out_ms)
try {
    if (!ctx || P < 1 || !elem_of_problem || !alpha_scaled || n_f < 0 || (n_f > 0 && (!F || !out_var))) return MXE_ERR_ARG;
    if (n_f == 0 && !out_diag) return MXE_ERR_ARG;
    if (out_prior && n_f == 0) return MXE_ERR_ARG;
    const size_t nw = ctx->n_omega, np = P, nf = n_f;
    Stage sg;
    PostStage st;
    // n_max bounds what the kernel indexes with 32 bits: var / prior [P][n_f], diag [P][nw] and F [n_f][nw]
    const size_t n_max = std::max({np * std::max<size_t>(nf, 1), np * nw, nf * nw});
    if (int rc = stage_posterior(sg, ctx, P, elem_of_problem, alpha_scaled, H, problem_index, chi2_factor, n_max, nullptr, 0, st);
        rc != MXE_OK) return rc;
    if (!all_finite(F, nf * nw)) return MXE_ERR_ARG;
    Block b;                                                  // pv_d
    const size_t oA = b.add(np);                              // alpha [P]
    const size_t oH = b.add(H ? np * nw : 0);                 // H [P][nw], when handed in
    const size_t oF = b.add(nf * nw);                         // F [n_f][nw]
    const size_t oV = b.add(np * nf);                         // var [P][n_f]
    const size_t oP = b.add(out_prior ? np * nf : 0);         // prior [P][n_f]
    const size_t oD = b.add(out_diag ? np * nw : 0);          // diag [P][nw]
    STGCHK(sg, ctx->pv_d.ensure(b.total));
    double* d = ctx->pv_d.p;
    mxe::PostVarParams pp;
    if (int rc = upload_posterior(sg, st, P, H, d + oA, d + oH, pp); rc != MXE_OK) return rc;
    STGCHK(sg, sg.upload(d + oF, F, nf * nw));
    pp.F = n_f ? d + oF : nullptr;
    pp.out_var = d + oV; pp.out_prior = out_prior ? d + oP : nullptr; pp.out_diag = out_diag ? d + oD : nullptr;
    pp.n_f = n_f;
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    STGCHK(sg, launch_factor_kernel(mxe::postvar_kernel<4>, mxe::postvar_kernel<8>, ctx, np, st.lds, pp));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_var, d + oV, np * nf)); STGCHK(sg, sg.fetch(out_prior, d + oP, np * nf));
    STGCHK(sg, sg.fetch(out_diag, d + oD, np * nw));
    STGCHK(sg, sg.finish(out_ms));
    if (chi2_factor != 1.0) {         // Gamma(eta, alpha~) = Gamma(1, alpha~ / eta) / eta
        for (size_t i = 0; i < np * nf; ++i) { out_var[i] /= chi2_factor; if (out_prior) out_prior[i] /= chi2_factor; }
        if (out_diag) for (size_t i = 0; i < np * nw; ++i) out_diag[i] /= chi2_factor;
    }
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_posterior_sample(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                                    const double* H, const int32_t* problem_index, double chi2_factor,
                                    int n_samples, uint64_t seed, const uint64_t* stream, const double* z,
                                    double* out_dH, float* out_ms)
try {
    if (!ctx || P < 1 || !elem_of_problem || !alpha_scaled || !out_dH || n_samples < 1 || (!z && !stream)) return MXE_ERR_ARG;
    const int nw = ctx->n_omega, nz = nw + ctx->n_s;
    const size_t np = P, n_z = np * n_samples * nz, n_out = np * n_samples * nw;
    Stage sg;
    PostStage st;
    // n_max = n_z bounds the kernel's 32-bit indices: z [P][n_samples][nz] is the largest array of the call
    if (int rc = stage_posterior(sg, ctx, P, elem_of_problem, alpha_scaled, H, problem_index, chi2_factor, n_z, z, n_z, st);
        rc != MXE_OK) return rc;
    Block b;                                                  // ps_d
    const size_t oA = b.add(np);                              // alpha [P]
    const size_t oS = b.add(np);                              // stream ids [P] (64-bit words)
    const size_t oH = b.add(H ? np * nw : 0);                 // H [P][nw], when handed in
    const size_t oZ = b.add(n_z);                             // z [P][n_samples][nz]
    const size_t oO = b.add(n_out);                           // samples [P][n_samples][nw]
    STGCHK(sg, ctx->ps_d.ensure(b.total));
    double* d = ctx->ps_d.p;
    mxe::PostSampleParams pp;
    if (int rc = upload_posterior(sg, st, P, H, d + oA, d + oH, pp); rc != MXE_OK) return rc;
    if (z) STGCHK(sg, sg.upload(d + oZ, z, n_z));
    else STGCHK(sg, sg.upload((uint64_t*)(d + oS), stream, np));
    pp.z = d + oZ; pp.out = d + oO; pp.scale = 1.0 / std::sqrt(chi2_factor);
    pp.n_samples = n_samples;
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    if (!z) {
        const size_t per = (size_t)n_samples * ((nz + 1) / 2);
        const unsigned gx = (unsigned)std::min<size_t>((per + 255) / 256, 1024), gy = (unsigned)std::min(P, 65535);
        hipLaunchKernelGGL(mxe::normals_kernel, dim3(gx, gy), dim3(256), 0, ctx->stream, seed, (const uint64_t*)(d + oS),
                           (uint64_t)0, P, n_samples, nz, d + oZ);
        STGCHK(sg, hipGetLastError());
    }
    STGCHK(sg, launch_factor_kernel(mxe::postsample_kernel<4>, mxe::postsample_kernel<8>, ctx, np, st.lds, pp));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_dH, d + oO, n_out));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- diagnostics of a fit: leverages, number of good data, whitened residuals (mxe_fitdiag.hip.h) -----------------------
#include "mxe_fitdiag.hip.h"

extern "C" int mxe_fit_diagnostics(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                                   const double* H, const int32_t* problem_index, double chi2_factor, int ld,
                                   double* out_ngood, double* out_chi2, double* out_resid, double* out_lev, float* out_ms)
try {
    if (!ctx || P < 1 || !elem_of_problem || !alpha_scaled || ld < 1) return MXE_ERR_ARG;
    const size_t nw = ctx->n_omega, np = P, nl = ld;
    Stage sg;
    PostStage st;
    // n_max bounds what the kernel's callers index: residuals / leverages [P][ld] and the H rows [P][nw]
    if (int rc = stage_posterior(sg, ctx, P, elem_of_problem, alpha_scaled, H, problem_index, chi2_factor,
                             std::max(np * nl, np * nw), nullptr, 0, st); rc != MXE_OK) return rc;
    for (int p = 0; p < P; ++p)
        if (ctx->ds[ctx->elem_ds[elem_of_problem[p]]].n_rows > ld) return MXE_ERR_ARG;
    // Uhat of the data sets and rperp of the elements: at the first call and after any change of either
    if (int rc = upload_projection(ctx); rc != MXE_OK) return rc;
    if (int rc = upload_row_offsets(ctx); rc != MXE_OK) return rc;
    if (ctx->rperp_dirty) {
        STGCHK(sg, sg.upload(ctx->drperp.p, ctx->h_rperp.data(), ctx->h_rperp.size()));
        STGCHK(sg, stream_wait(ctx->stream));
        ctx->rperp_dirty = false;
    }
    Block b;                                                  // pv_d
    const size_t oA = b.add(np);                              // alpha [P]
    const size_t oH = b.add(H ? np * nw : 0);                 // H [P][nw], when handed in
    const size_t oN = b.add(np);                              // N_g [P]
    const size_t oC = b.add(np);                              // chi2 [P]
    const size_t oR = b.add(np * nl);                         // residuals [P][ld]
    const size_t oL = b.add(np * nl);                         // leverages [P][ld]
    STGCHK(sg, ctx->pv_d.ensure(b.total));
    double* d = ctx->pv_d.p;
    mxe::FitDiagParams pp;
    if (int rc = upload_posterior(sg, st, P, H, d + oA, d + oH, pp); rc != MXE_OK) return rc;
    pp.ghat = ctx->dghat.p; pp.U = ctx->dproj_U.p; pp.ds_off = ctx->dproj_off.p;
    pp.rperp = ctx->drperp.p; pp.elem_roff = ctx->delem_roff.p;
    pp.out_ngood = d + oN; pp.out_chi2 = d + oC; pp.out_resid = d + oR; pp.out_lev = d + oL;
    pp.ld = ld;
    const size_t lds = mxe::fitdiag_lds_bytes(ctx->NP, ctx->nwp);      // (below postvar_kernel's, which stage_posterior checked)
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    STGCHK(sg, launch_factor_kernel(mxe::fitdiag_kernel<4>, mxe::fitdiag_kernel<8>, ctx, np, lds, pp));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_ngood, d + oN, np)); STGCHK(sg, sg.fetch(out_chi2, d + oC, np));
    STGCHK(sg, sg.fetch(out_resid, d + oR, np * nl)); STGCHK(sg, sg.fetch(out_lev, d + oL, np * nl));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- linear response of the minimiser: resolution operator, response to the data (mxe_response.hip.h) -------------------
#include "mxe_response.hip.h"

extern "C" int mxe_response(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                            const double* H, const int32_t* problem_index, double chi2_factor,
                            int space, int weighted, int n_rhs, int ld, const double* F, double* out_X, float* out_ms)
try {
    if (!ctx || P < 1 || !elem_of_problem || !alpha_scaled || !F || !out_X || n_rhs < 1 || ld < 1) return MXE_ERR_ARG;
    if (space != 0 && space != 1) return MXE_ERR_ARG;
    const size_t nw = ctx->n_omega, np = P;
    if (space == 0 && (size_t)ld < nw) return MXE_ERR_ARG;
    // n_max bounds the arrays of the call: F [P][n_rhs][ld] and X [P][n_rhs][nw]
    if (np * (size_t)n_rhs > 0x7fffffffull) return MXE_ERR_ARG;       // (the products below stay within 64 bits)
    const size_t n_F = np * (size_t)n_rhs * (size_t)ld, n_X = np * (size_t)n_rhs * nw;
    Stage sg;
    PostStage st;
    if (int rc = stage_posterior(sg, ctx, P, elem_of_problem, alpha_scaled, H, problem_index, chi2_factor, std::max(n_F, n_X), F,
                                 n_F, st); rc != MXE_OK) return rc;
    if (space == 1) {
        for (int p = 0; p < P; ++p)
            if (ctx->ds[ctx->elem_ds[elem_of_problem[p]]].n_rows > ld) return MXE_ERR_ARG;
        // Uhat of the data sets: at the first call and after any change of them
        if (int rc = upload_projection(ctx); rc != MXE_OK) return rc;
    }
    Block b;                                                  // pv_d
    const size_t oA = b.add(np);                              // alpha [P]
    const size_t oH = b.add(H ? np * nw : 0);                 // H [P][nw], when handed in
    const size_t oF = b.add(n_F);                             // F [P][n_rhs][ld]
    const size_t oX = b.add(n_X);                             // X [P][n_rhs][nw]
    STGCHK(sg, ctx->pv_d.ensure(b.total));
    double* d = ctx->pv_d.p;
    mxe::ResponseParams pp;
    if (int rc = upload_posterior(sg, st, P, H, d + oA, d + oH, pp); rc != MXE_OK) return rc;
    STGCHK(sg, sg.upload(d + oF, F, n_F));
    pp.F = d + oF; pp.out = d + oX;
    pp.U = space ? ctx->dproj_U.p : nullptr; pp.ds_off = space ? ctx->dproj_off.p : nullptr;
    pp.n_rhs = n_rhs; pp.ld = ld; pp.space = space; pp.weighted = weighted ? 1 : 0;
    const size_t lds = mxe::response_lds_bytes(ctx->NP, ctx->nwp);     // (below postvar_kernel's, which stage_posterior checked)
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    STGCHK(sg, launch_factor_kernel(mxe::response_kernel<4>, mxe::response_kernel<8>, ctx, np, lds, pp));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_X, d + oX, n_X));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_normals(int device, uint64_t seed, uint64_t stream, int n_samples, int n, double* out_z)
try {
    if (n_samples < 1 || n < 1 || !out_z || (size_t)n_samples * (size_t)n > 0x7fffffffull) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    double* dz;
    STGCHK(sg, sg.alloc(&dz, (size_t)n_samples * n));
    const size_t per = (size_t)n_samples * ((n + 1) / 2);
    hipLaunchKernelGGL(mxe::normals_kernel, dim3((unsigned)std::min<size_t>((per + 255) / 256, 1024), 1), dim3(256), 0, sg.stream,
                       seed, (const uint64_t*)nullptr, stream, 1, n_samples, n, dz);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.fetch(out_z, dz, (size_t)n_samples * n));
    STGCHK(sg, sg.finish(nullptr));
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_entropy(int device, int kind, int n_omega, int P, const double* H, const double* D,
                           double* out_S, double* out_dS, double* out_ddS)
try {
    if (n_omega < 1 || P < 1 || !H || !D || (kind != MXE_ENTROPY_NORMAL && kind != MXE_ENTROPY_PLUSMINUS)) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    const size_t n = n_omega, np = P;
    double *dH, *dD, *dS, *dd, *ddd;
    STGCHK(sg, sg.alloc(&dH, np * n)); STGCHK(sg, sg.alloc(&dD, n)); STGCHK(sg, sg.alloc(&dS, np));
    STGCHK(sg, sg.alloc(&dd, np * n)); STGCHK(sg, sg.alloc(&ddd, np * n));
    STGCHK(sg, sg.upload(dH, H, np * n)); STGCHK(sg, sg.upload(dD, D, n));
    hipLaunchKernelGGL(mxe::entropy_kernel, dim3((unsigned)P), dim3(256), 0, sg.stream, kind, n_omega, dH, dD, dS, dd, ddd);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.fetch(out_S, dS, np)); STGCHK(sg, sg.fetch(out_dS, dd, np * n));
    STGCHK(sg, sg.fetch(out_ddS, ddd, np * n));
    STGCHK(sg, sg.finish(nullptr));
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_audit(mxe_ctx* ctx, double* out_corr, double* out_gmax)
try {
    if (!ctx || (!out_corr && !out_gmax)) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    HIPCHK(ctx, ctx->ev_scal.ensure(2 * P));
    HIPCHK(ctx, ctx->dparent_elem.ensure(ctx->chain_elem.size()));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dparent_elem.p, ctx->chain_elem.data(), ctx->chain_elem.size() * sizeof(int),
                               hipMemcpyHostToDevice, ctx->stream));
    mxe::EvalParams ep;
    eval_params_base(ctx, ep);
    ep.elem = ctx->dparent_elem.p; ep.elem_div = ctx->n_alpha;
    ep.alpha = ctx->dalpha.p;                 // alpha / eta, as the chain kernel iterated on it
    ep.x = ctx->dout_v.p; ep.x_stride = ctx->NP;
    ep.want_audit = 1;
    ep.corr = ctx->ev_scal.p; ep.gmax = ctx->ev_scal.p + P;
    int rc = launch_eval(ctx, ep, P);
    if (rc != MXE_OK) return rc;
    if (out_corr) HIPCHK(ctx, hipMemcpyAsync(out_corr, ep.corr, P * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_gmax) HIPCHK(ctx, hipMemcpyAsync(out_gmax, ep.gmax, P * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- the default analyzer's alpha on the device, and the compact result pack ----------------
#ifdef MXE_PROFILE
// (diagnostic build: linefit_kernel stamps its phases, [n_chain][4 waves][10] clock values; mxe_prof_linefit_fetch, tools/profile_linefit.py)
#define MXE_LINEFIT_PROF_ENSURE(ctx) HIPCHK(ctx, (ctx)->dprof_lf.ensure((size_t)(ctx)->n_chain * 40))
#define MXE_LINEFIT_PROF_ARG(ctx) , (ctx)->dprof_lf.p
#else
#define MXE_LINEFIT_PROF_ENSURE(ctx) do {} while (0)
#define MXE_LINEFIT_PROF_ARG(ctx)
#endif
extern "C" int mxe_select_launch(mxe_ctx* ctx, int p2_deg)
try {
    if (!ctx || (p2_deg != 0 && p2_deg != 1)) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    double* sel = ctx->dout_Q.p + P;
    double* idx = sel + (size_t)ctx->n_chain * ctx->n_omega;
    MXE_LINEFIT_PROF_ENSURE(ctx);
    hipLaunchKernelGGL(mxe::linefit_kernel, dim3(ctx->n_chain), dim3(256), ((size_t)11 * ctx->n_alpha + 6 + 28) * sizeof(double), ctx->stream,
                       ctx->dalpha_log.p, ctx->dout_chi2.p, ctx->dout_H.p, ctx->n_alpha, ctx->n_omega, p2_deg, sel, idx,
                       nullptr, 0.2, nullptr, nullptr MXE_LINEFIT_PROF_ARG(ctx));
    HIPCHK(ctx, hipGetLastError());
    return MXE_OK;
}
MXE_CATCH_ALL

// The three default analyzers of the reference in one small launch: the line fit as above (its row and index also land in
// the compact pack), the alpha of the largest curvature of log10 chi2 over gamma log10 alpha, the alpha of the flattest
// entropy -- indices and the three H rows per scan in a buffer of their own, fetched with ONE copy (mxe_select3_fetch).
extern "C" int mxe_select3_launch(mxe_ctx* ctx, int p2_deg, double gamma)
try {
    if (!ctx || (p2_deg != 0 && p2_deg != 1) || !(gamma > 0.0)) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha, nc = ctx->n_chain, nw = ctx->n_omega;
    double* sel = ctx->dout_Q.p + P;
    double* idx = sel + nc * nw;
    HIPCHK(ctx, ctx->dsel3.ensure(3 * nc * (nw + 1)));
    ctx->pre_rows = nullptr; ctx->pre_index = false;
    MXE_LINEFIT_PROF_ENSURE(ctx);
    hipLaunchKernelGGL(mxe::linefit_kernel, dim3(ctx->n_chain), dim3(256), ((size_t)11 * ctx->n_alpha + 6 + 28) * sizeof(double), ctx->stream,
                       ctx->dalpha_log.p, ctx->dout_chi2.p, ctx->dout_H.p, ctx->n_alpha, ctx->n_omega, p2_deg, sel, idx,
                       ctx->dout_S.p, gamma, ctx->dsel3.p, ctx->dsel3.p + 3 * nc MXE_LINEFIT_PROF_ARG(ctx));
    HIPCHK(ctx, hipGetLastError());
    ctx->sel3_nc = ctx->n_chain;
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_select3_fetch_rows(mxe_ctx* ctx, int32_t* out_index /*[3][n_chain] or NULL*/, int first, int count,
                                      double* out_H_selected /*[count][n_chain][n_omega] or NULL*/)
try {
    if (!ctx || first < 0 || count < 0 || first + count > 3 || (!out_index && !out_H_selected)) return MXE_ERR_ARG;
    if (!ctx->launched || !ctx->dsel3.p || ctx->sel3_nc != ctx->n_chain) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nc = ctx->n_chain, nw = ctx->n_omega;
    if (ctx->pre_index && ctx->h_sel3_pinned_n >= 3 * nc && (count == 0 || (out_H_selected == ctx->pre_rows && first == ctx->pre_first && count == ctx->pre_count))) {
        // (mxe_select3_prefetch_rows queued these copies behind the selection kernel)
        HIPCHK(ctx, stream_wait(ctx->stream));
        if (out_index) for (size_t i = 0; i < 3 * nc; ++i) out_index[i] = (int32_t)ctx->h_sel3_pinned[i];
        return MXE_OK;
    }
    if (out_index) {
        ctx->h_sel3.resize(3 * nc);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_sel3.data(), ctx->dsel3.p, 3 * nc * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, stream_wait(ctx->stream));       // (the selection kernel has finished before any path of the row copy starts)
    if (out_H_selected && count > 0)
        HIPCHK(ctx, d2h_pipelined(out_H_selected, ctx->dsel3.p + 3 * nc + (size_t)first * nc * nw, (size_t)count * nc * nw * 8, ctx->stream));
    if (out_index) for (size_t i = 0; i < 3 * nc; ++i) out_index[i] = (int32_t)ctx->h_sel3[i];
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_select3_prefetch_rows(mxe_ctx* ctx, int first, int count, double* out_H_selected /*[count][n_chain][n_omega] or NULL*/)
try {
    if (!ctx || first < 0 || count < 0 || first + count > 3 || (count > 0 && !out_H_selected)) return MXE_ERR_ARG;
    if (!ctx->launched || !ctx->dsel3.p || ctx->sel3_nc != ctx->n_chain) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nc = ctx->n_chain, nw = ctx->n_omega;
    ctx->pre_rows = nullptr; ctx->pre_index = false;
    if (ctx->h_sel3_pinned_n < 3 * nc) {
        if (ctx->h_sel3_pinned) { (void)hipHostFree(ctx->h_sel3_pinned); ctx->h_sel3_pinned = nullptr; ctx->h_sel3_pinned_n = 0; }
        HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_sel3_pinned, 3 * nc * 8, hipHostMallocDefault));
        ctx->h_sel3_pinned_n = 3 * nc;
    }
    const size_t row_bytes = (size_t)count * nc * nw * 8;
    const bool mapped = count == 0 || g_host.holds(out_H_selected, row_bytes);
    if (mapped)
        HIPCHK(ctx, copy_out(ctx->h_sel3_pinned, ctx->dsel3.p, 3 * nc * 8, out_H_selected, ctx->dsel3.p + 3 * nc + (size_t)first * nc * nw, row_bytes, true, ctx->stream));
    else {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_sel3_pinned, ctx->dsel3.p, 3 * nc * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(out_H_selected, ctx->dsel3.p + 3 * nc + (size_t)first * nc * nw, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    ctx->pre_index = true; ctx->pre_rows = count > 0 ? out_H_selected : nullptr; ctx->pre_first = first; ctx->pre_count = count;
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_select3_fetch(mxe_ctx* ctx, int32_t* out_index /*[3][n_chain]*/, double* out_H_selected /*[3][n_chain][n_omega]*/)
{
    if (!ctx || !out_index) return MXE_ERR_ARG;
    return mxe_select3_fetch_rows(ctx, out_index, 0, out_H_selected ? 3 : 0, out_H_selected);
}

extern "C" int mxe_select_fetch(mxe_ctx* ctx, int32_t* out_index, double* out_H_selected)
try {
    if (!ctx) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha, nc = ctx->n_chain, nw = ctx->n_omega;
    const double* sel = ctx->dout_Q.p + P;
    HIPCHK(ctx, stream_wait(ctx->stream));
    if (out_H_selected) HIPCHK(ctx, hipMemcpy(out_H_selected, sel, nc * nw * 8, hipMemcpyDeviceToHost));
    if (out_index) {
        std::vector<double> hi(nc);
        HIPCHK(ctx, hipMemcpy(hi.data(), sel + nc * nw, nc * 8, hipMemcpyDeviceToHost));
        for (size_t c = 0; c < nc; ++c) out_index[c] = (int32_t)hi[c];
    }
    return MXE_OK;
}
MXE_CATCH_ALL

namespace {
// one workgroup per requested row: out[r][:] = H[idx[r]][:]
__global__ __launch_bounds__(256)
void rows_gather_kernel(const double* __restrict__ H, const int* __restrict__ idx, int n_omega, double* __restrict__ out)
{
    const double* src = H + (size_t)idx[blockIdx.x] * n_omega;
    double* dst = out + (size_t)blockIdx.x * n_omega;
    for (int i = threadIdx.x; i < n_omega; i += 256) dst[i] = src[i];
}
}  // namespace

extern "C" int mxe_fetch_rows(mxe_ctx* ctx, int n_rows, const int32_t* problem_index, double* out_H)
try {
    if (!ctx || n_rows < 1 || !problem_index || !out_H) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha, nw = ctx->n_omega;
    for (int r = 0; r < n_rows; ++r)
        if (problem_index[r] < 0 || (size_t)problem_index[r] >= P) return MXE_ERR_ARG;
    // the rows are collected on the device and come over in ONE copy (a copy per row cost 7 us each: 5 ms for the
    // 768 rows the analyzers of a 16 x 16 job pick)
    HIPCHK(ctx, ctx->rows_idx.ensure(n_rows));
    HIPCHK(ctx, ctx->rows_out.ensure((size_t)n_rows * nw));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rows_idx.p, problem_index, (size_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(rows_gather_kernel, dim3(n_rows), dim3(256), 0, ctx->stream,
                       (const double*)ctx->dout_H.p, (const int*)ctx->rows_idx.p, (int)nw, ctx->rows_out.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_H, ctx->rows_out.p, (size_t)n_rows * nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- gather between GPUs: RCCL over xGMI, called directly (no framework in between) --------
#include <rccl/rccl.h>
#include <dlfcn.h>
namespace {
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load() {
        if (lib) return true;
        const char* names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
        for (const char* n : names) { lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) return false;
#define MXE_SYM(field, name) field = reinterpret_cast<decltype(field)>(dlsym(lib, name)); if (!field) { dlclose(lib); lib = nullptr; return false; }
        MXE_SYM(GetUniqueId, "ncclGetUniqueId"); MXE_SYM(CommInitRank, "ncclCommInitRank"); MXE_SYM(CommInitAll, "ncclCommInitAll");
        MXE_SYM(CommDestroy, "ncclCommDestroy"); MXE_SYM(Send, "ncclSend"); MXE_SYM(Recv, "ncclRecv");
        MXE_SYM(AllReduce, "ncclAllReduce"); MXE_SYM(GroupStart, "ncclGroupStart"); MXE_SYM(GroupEnd, "ncclGroupEnd"); MXE_SYM(GetErrorString, "ncclGetErrorString");
#undef MXE_SYM
        return true;
    }
};
Rccl g_rccl;
#define NCCLCHK(ctx, call) do { ncclResult_t r__ = (call); if (r__ != ncclSuccess) { \
    (ctx)->hip_err = std::string(#call) + ": " + g_rccl.GetErrorString(r__); return MXE_ERR_HIP; } } while (0)
} // namespace

struct mxe_comm_state {
    ncclComm_t comm = nullptr;
    int n_ranks = 1, rank = 0;
    bool copy_transport = false;                 // ranks of ONE process on one device: plain device copies
    bool loopback = false;                       // mxe_comm_set_loopback: the root's own pack goes through ncclSend / ncclRecv to itself
    std::vector<mxe_ctx*> local;                 // ... the contexts of that process, by rank
    DevBuf<double> recv;                         // root: [sum of counts]
    DevBuf<double> small;                        // mxe_comm_allreduce
};

extern "C" int mxe_comm_unique_id(char* out_id128)
{
    if (!out_id128) return MXE_ERR_ARG;
    if (!g_rccl.load()) return MXE_ERR_NODEVICE;
    ncclUniqueId id;
    if (g_rccl.GetUniqueId(&id) != ncclSuccess) return MXE_ERR_HIP;
    std::memcpy(out_id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return MXE_OK;
}

extern "C" int mxe_comm_init(mxe_ctx* ctx, int n_ranks, int rank, const char* id128)
try {
    if (!ctx || n_ranks < 1 || rank < 0 || rank >= n_ranks || !id128) return MXE_ERR_ARG;
    if (!g_rccl.load()) { ctx->hip_err = "librccl.so.1 could not be loaded"; return MXE_ERR_NODEVICE; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    comm_release(ctx);
    ctx->comm = new mxe_comm_state();
    ctx->comm->n_ranks = n_ranks; ctx->comm->rank = rank;
    ncclUniqueId id;
    std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    NCCLCHK(ctx, g_rccl.CommInitRank(&ctx->comm->comm, n_ranks, id, rank));
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_comm_init_local(mxe_ctx** ctxs, int n)
try {
    if (!ctxs || n < 1) return MXE_ERR_ARG;
    for (int r = 0; r < n; ++r) if (!ctxs[r]) return MXE_ERR_ARG;
    bool distinct = true;
    for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) if (ctxs[a]->device == ctxs[b]->device) distinct = false;
    std::vector<ncclComm_t> comms(n, nullptr);
    if (distinct && n > 1) {
        if (!g_rccl.load()) { ctxs[0]->hip_err = "librccl.so.1 could not be loaded"; return MXE_ERR_NODEVICE; }
        std::vector<int> devs(n);
        for (int r = 0; r < n; ++r) devs[r] = ctxs[r]->device;
        // xGMI peers reach each other directly; where a pair cannot (hipDeviceCanAccessPeer), RCCL stages through the host --
        // slower, still correct.  Said once on stderr; an error only when the caller insists (MXE_REQUIRE_PEER_ACCESS)
        for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) {
            int can = 1;
            if (a != b && hipDeviceCanAccessPeer(&can, devs[a], devs[b]) == hipSuccess && !can) {
                if (getenv("MXE_REQUIRE_PEER_ACCESS")) {
                    ctxs[0]->hip_err = "device " + std::to_string(devs[a]) + " cannot access device " + std::to_string(devs[b]) + " directly (hipDeviceCanAccessPeer)";
                    return MXE_ERR_HIP;
                }
                static bool said = false;
                if (!said) { said = true; fprintf(stderr, "[mxe] devices %d and %d have no direct peer access: the gather goes through host memory\n", devs[a], devs[b]); }
            }
        }
        NCCLCHK(ctxs[0], g_rccl.CommInitAll(comms.data(), n, devs.data()));
    }
    for (int r = 0; r < n; ++r) {
        comm_release(ctxs[r]);
        ctxs[r]->comm = new mxe_comm_state();
        ctxs[r]->comm->n_ranks = n; ctxs[r]->comm->rank = r;
        ctxs[r]->comm->comm = comms[r];
        ctxs[r]->comm->copy_transport = !(distinct && n > 1);
        ctxs[r]->comm->local.assign(ctxs, ctxs + n);
    }
    return MXE_OK;
}
MXE_CATCH_ALL

static void comm_release(mxe_ctx* ctx)
{
    if (!ctx || !ctx->comm) return;
    if (ctx->comm->comm && g_rccl.lib) g_rccl.CommDestroy(ctx->comm->comm);
    ctx->comm->recv.release();
    ctx->comm->small.release();
    delete ctx->comm;
    ctx->comm = nullptr;
}

// Test plumbing for a box with ONE GPU: with it on, the root's own pack travels through ncclSend / ncclRecv to itself
// (inside ncclGroupStart / ncclGroupEnd) instead of a device copy and mxe_comm_allreduce runs ncclAllReduce with the
// one rank -- every RCCL call of the multi-GPU path executes.  Communicators of mxe_comm_init only.
extern "C" int mxe_comm_set_loopback(mxe_ctx* ctx, int on)
{
    if (!ctx) return MXE_ERR_ARG;
    if (!ctx->comm || !ctx->comm->comm || !ctx->comm->local.empty()) return MXE_ERR_STATE;
    ctx->comm->loopback = on != 0;
    return MXE_OK;
}

extern "C" int mxe_comm_destroy(mxe_ctx* ctx)
{
    if (!ctx) return MXE_ERR_ARG;
    hipSetDevice(ctx->device);
    comm_release(ctx);
    return MXE_OK;
}

// what a rank contributes: the compact pack (chi2, S, Q of every alpha + the H row and index of the
// analyzer's alpha per scan) or the full one (all H in front of it)
static void gather_span(mxe_ctx* ctx, int what, double** p, size_t* count)
{
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha, nw = ctx->n_omega, nc = ctx->n_chain;
    const size_t compact = 3 * P + nc * (nw + 1);
    if (what == MXE_GATHER_FULL) { *p = ctx->dout_H.p; *count = P * nw + compact; }
    else { *p = ctx->dout_chi2.p; *count = compact; }
}

// enqueue this rank's part of the gather on its stream (inside a group when called for several local ranks)
static int gather_enqueue(mxe_ctx* ctx, int root, int what, const int64_t* counts)
{
    mxe_comm_state* cm = ctx->comm;
    double* mine; size_t n_mine;
    gather_span(ctx, what, &mine, &n_mine);
    if ((int64_t)n_mine != counts[cm->rank]) return MXE_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (cm->rank == root) {
        // (the root's receive buffer was sized by the caller BEFORE ncclGroupStart: gather_reserve -- an allocation, i.e. a
        //  possible device synchronisation, has no place between the calls of a group)
        size_t off = 0;
        for (int r = 0; r < cm->n_ranks; ++r) {
            if (r == root && cm->loopback && !cm->copy_transport) {
                // (send and receive of one rank to itself, matched inside the caller's group: the same calls a peer's pack takes)
                NCCLCHK(ctx, g_rccl.Send(mine, n_mine, ncclDouble, root, cm->comm, ctx->stream));
                NCCLCHK(ctx, g_rccl.Recv(cm->recv.p + off, n_mine, ncclDouble, root, cm->comm, ctx->stream));
            }
            else if (r == root) HIPCHK(ctx, hipMemcpyAsync(cm->recv.p + off, mine, n_mine * 8, hipMemcpyDeviceToDevice, ctx->stream));
            else if (!cm->copy_transport) NCCLCHK(ctx, g_rccl.Recv(cm->recv.p + off, (size_t)counts[r], ncclDouble, r, cm->comm, ctx->stream));
            off += (size_t)counts[r];
        }
    } else if (!cm->copy_transport) {
        NCCLCHK(ctx, g_rccl.Send(mine, n_mine, ncclDouble, root, cm->comm, ctx->stream));
    }
    return MXE_OK;
}

// the root's receive buffer for a gather of these counts (outside any RCCL group)
static int gather_reserve(mxe_ctx* root_ctx, int n_ranks, const int64_t* counts)
{
    size_t total = 0;
    for (int r = 0; r < n_ranks; ++r) { if (counts[r] < 0) return MXE_ERR_ARG; total += (size_t)counts[r]; }
    HIPCHK(root_ctx, hipSetDevice(root_ctx->device));
    HIPCHK(root_ctx, root_ctx->comm->recv.ensure(total));
    return MXE_OK;
}

extern "C" int mxe_gather(mxe_ctx* ctx, int root, int what, const int64_t* counts, double* recv_host)
try {
    if (!ctx || !counts || (what != MXE_GATHER_COMPACT && what != MXE_GATHER_FULL)) return MXE_ERR_ARG;
    if (!ctx->comm || !ctx->launched) return MXE_ERR_STATE;
    mxe_comm_state* cm = ctx->comm;
    if (root < 0 || root >= cm->n_ranks) return MXE_ERR_ARG;
    if (!cm->local.empty()) return MXE_ERR_STATE;            // ranks of one process gather together: mxe_gather_local
    if (cm->rank == root) { const int rr = gather_reserve(ctx, cm->n_ranks, counts); if (rr != MXE_OK) return rr; }
    const bool grouped = cm->n_ranks > 1 || cm->loopback;
    if (grouped) NCCLCHK(ctx, g_rccl.GroupStart());
    const int rc = gather_enqueue(ctx, root, what, counts);
    if (grouped) NCCLCHK(ctx, g_rccl.GroupEnd());
    if (rc != MXE_OK) return rc;
    if (recv_host && cm->rank == root) {
        size_t total = 0;
        for (int r = 0; r < cm->n_ranks; ++r) total += (size_t)counts[r];
        HIPCHK(ctx, hipMemcpyAsync(recv_host, cm->recv.p, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, stream_wait(ctx->stream));
    }
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_gather_local(mxe_ctx** ctxs, int n, int root, int what, const int64_t* counts, double* recv_host)
try {
    if (!ctxs || n < 1 || root < 0 || root >= n || !counts || (what != MXE_GATHER_COMPACT && what != MXE_GATHER_FULL)) return MXE_ERR_ARG;
    for (int r = 0; r < n; ++r)
        if (!ctxs[r] || !ctxs[r]->comm || ctxs[r]->comm->n_ranks != n || ctxs[r]->comm->rank != r || !ctxs[r]->launched) return MXE_ERR_STATE;
    mxe_ctx* rt = ctxs[root];
    const bool copy = rt->comm->copy_transport;
    { const int rr = gather_reserve(rt, n, counts); if (rr != MXE_OK) return rr; }
    if (copy) {
        // ranks that share a device (or a single rank): the root waits for the others' launches with events
        // and copies their packs itself
        for (int r = 0; r < n; ++r) {
            if (r == root) continue;
            HIPCHK(ctxs[r], hipSetDevice(ctxs[r]->device));
            HIPCHK(ctxs[r], hipEventRecord(ctxs[r]->ev_mark, ctxs[r]->stream));
            HIPCHK(rt, hipSetDevice(rt->device));
            HIPCHK(rt, hipStreamWaitEvent(rt->stream, ctxs[r]->ev_mark, 0));
        }
    } else {
        NCCLCHK(rt, g_rccl.GroupStart());
    }
    int rc = MXE_OK;
    for (int r = 0; r < n && rc == MXE_OK; ++r) rc = gather_enqueue(ctxs[r], root, what, counts);
    if (!copy) NCCLCHK(rt, g_rccl.GroupEnd());
    if (rc != MXE_OK) return rc;
    if (copy) {
        HIPCHK(rt, hipSetDevice(rt->device));
        size_t off = 0;
        for (int r = 0; r < n; ++r) {
            if (r != root) {
                double* src; size_t cnt;
                gather_span(ctxs[r], what, &src, &cnt);
                HIPCHK(rt, hipMemcpyAsync(rt->comm->recv.p + off, src, cnt * 8, hipMemcpyDeviceToDevice, rt->stream));
            }
            off += (size_t)counts[r];
        }
    }
    if (recv_host) {
        size_t total = 0;
        for (int r = 0; r < n; ++r) total += (size_t)counts[r];
        HIPCHK(rt, hipSetDevice(rt->device));
        HIPCHK(rt, hipMemcpyAsync(recv_host, rt->comm->recv.p, total * 8, hipMemcpyDeviceToHost, rt->stream));
        HIPCHK(rt, stream_wait(rt->stream));
    }
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_comm_allreduce(mxe_ctx* ctx, double* inout_host, int n, int op)
try {
    if (!ctx || !inout_host || n < 1 || n > 64 || (op != 0 && op != 1)) return MXE_ERR_ARG;
    if (!ctx->comm) return MXE_ERR_STATE;
    mxe_comm_state* cm = ctx->comm;
    if ((cm->n_ranks == 1 && !cm->loopback) || !cm->local.empty()) return MXE_OK;        // one process: nothing to agree on
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, cm->small.ensure(64));
    HIPCHK(ctx, hipMemcpyAsync(cm->small.p, inout_host, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    NCCLCHK(ctx, g_rccl.AllReduce(cm->small.p, cm->small.p, (size_t)n, ncclDouble, op == 0 ? ncclSum : ncclMax, cm->comm, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(inout_host, cm->small.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}
MXE_CATCH_ALL

// element e -> rank e mod n_ranks (an element's alpha scan stays on one device); pure host arithmetic
extern "C" int mxe_shard_plan(int n_elem, int n_ranks, int32_t* rank_of_elem, int32_t* local_index, int32_t* n_local)
{
    if (n_elem < 0 || n_ranks < 1 || !rank_of_elem || !local_index || !n_local) return MXE_ERR_ARG;
    for (int r = 0; r < n_ranks; ++r) n_local[r] = 0;
    for (int e = 0; e < n_elem; ++e) {
        const int r = e % n_ranks;
        rank_of_elem[e] = r;
        local_index[e] = n_local[r]++;
    }
    return MXE_OK;
}

// ---- output map A = B H ----------------------------------------------------
namespace mxe {
// one workgroup per problem; thread j computes A_j = sum_k B[j][k] H[k]
// with Bt (= B^T, [k][j]) so that the loads are coalesced along j.
__global__ __launch_bounds__(256)
void output_map_kernel(const double* __restrict__ Bt, const double* __restrict__ H,
                       double* __restrict__ A, int nw)
{
    extern __shared__ double hs[];
    const double* Hp = H + (size_t)blockIdx.x * nw;
    for (int k = threadIdx.x; k < nw; k += blockDim.x) hs[k] = Hp[k];
    __syncthreads();
    for (int j = threadIdx.x; j < nw; j += blockDim.x) {
        double a0 = 0.0, a1 = 0.0;
        int k = 0;
        for (; k + 1 < nw; k += 2) {
            a0 = fma(Bt[(size_t)k * nw + j], hs[k], a0);
            a1 = fma(Bt[(size_t)(k + 1) * nw + j], hs[k + 1], a1);
        }
        if (k < nw) a0 = fma(Bt[(size_t)k * nw + j], hs[k], a0);
        A[(size_t)blockIdx.x * nw + j] = a0 + a1;
    }
}
} // namespace mxe

extern "C" int mxe_apply_output_map(mxe_ctx* ctx, const double* B, double* out_A)
try {
    if (!ctx || !B || !out_A) return MXE_ERR_ARG;
    if (!ctx->launched) return MXE_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nw = ctx->n_omega;
    const size_t P = (size_t)ctx->n_chain * ctx->n_alpha;
    std::vector<double> Bt((size_t)nw * nw);
    for (int j = 0; j < nw; ++j) for (int k = 0; k < nw; ++k) Bt[(size_t)k * nw + j] = B[(size_t)j * nw + k];
    HIPCHK(ctx, ctx->dB.ensure(Bt.size()));
    HIPCHK(ctx, ctx->dA.ensure(P * nw));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dB.p, Bt.data(), Bt.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(mxe::output_map_kernel, dim3((unsigned)P), dim3(256), (size_t)nw * 8, ctx->stream,
                       ctx->dB.p, ctx->dout_H.p, ctx->dA.p, nw);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_A, ctx->dA.p, P * nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx->stream));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- kernel matrix staging on the device: fill, preblur product, truncated SVD -------------
#include "mxe_svd.hip.h"


namespace {
// the LDS of the decomposition: m_rows values of a column, 16 + 8 of the reductions, SVD_RCAP + SVD_RCAP / 2 of the
// QR stage -- at most SVD_LDS_LIMIT bytes (device.SVD_MAX_ROWS is the largest m_rows that fits)
constexpr size_t SVD_LDS_LIMIT = 60 * 1024;
constexpr size_t svd_lds_bytes(int m_rows)
{
    return ((size_t)m_rows + 16 + 8 + mxe::SVD_RCAP + mxe::SVD_RCAP / 2) * sizeof(double);
}

// what every mxe_kernel_svd* entry asks of its arguments before its own checks
bool svd_args_ok(int n_grid, int n_omega, int n_b, const double* grid, const double* omega, const double* delta,
                 const double* preblur_b, double threshold, int ns_max, const double* out_U, const double* out_S,
                 const double* out_V, const int32_t* out_ns)
{
    return n_grid >= 1 && n_omega >= 1 && n_b >= 1 && grid && omega && delta && preblur_b && out_U && out_S && out_V &&
           out_ns && ns_max >= 1 && ns_max <= mxe::SVD_RCAP && threshold >= 0.0;
}

// the fill of a kernel whose threads each write one entry (or one column): ``kernel(args...)`` over nel of them
template <class Kern, class... Args>
void launch_fill(Kern kernel, hipStream_t st, int nel, Args... args)
{
    hipLaunchKernelGGL(kernel, dim3((nel + 255) / 256), dim3(256), 0, st, args...);
}

// mxe_kernel_svd and its siblings after their argument checks: ``fill(stream, dgrid, domega, dKt)`` writes the
// unblurred K^T (n_omega columns of m_rows values) from the row grid (n_grid values: tau, iomega, or the rows of a
// caller's matrix); the preblur
// stages, the decomposition and the copy-out are the same for every kernel
template <class Fill>
int kernel_svd_common(int device, int n_grid, int m_rows, int n_omega, const double* grid, const double* omega,
                      const double* delta, int n_b, const double* preblur_b, double threshold, int ns_max,
                      double* out_K, double* out_U, double* out_S, double* out_V, int32_t* out_ns,
                      int32_t* out_info, float* out_ms, Fill fill)
{
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    const size_t lds = svd_lds_bytes(m_rows);
    if (lds > SVD_LDS_LIMIT) return MXE_ERR_LIMIT;
    const size_t m = m_rows, n = n_omega, R = mxe::SVD_RCAP, nb = n_b;
    double *dgrid, *dom, *ddel, *dKt0, *dr1, *ddc, *dB;
    mxe::SvdParams sp;
    sp.m = m_rows; sp.n = n_omega; sp.ns_max = ns_max; sp.threshold = threshold;
    STGCHK(sg, sg.alloc(&dgrid, (size_t)n_grid)); STGCHK(sg, sg.alloc(&dom, n)); STGCHK(sg, sg.alloc(&ddel, n));
    STGCHK(sg, sg.alloc(&dKt0, n * m)); STGCHK(sg, sg.alloc(&dr1, n)); STGCHK(sg, sg.alloc(&ddc, n)); STGCHK(sg, sg.alloc(&dB, n * n));
    STGCHK(sg, sg.alloc(&sp.A, nb * n * m)); STGCHK(sg, sg.alloc(&sp.Vh, nb * R * m));
    STGCHK(sg, sg.alloc(&sp.Rm, nb * R * n)); STGCHK(sg, sg.alloc(&sp.Jt, nb * R * R));
    STGCHK(sg, sg.alloc(&sp.Qc, nb * R * m)); STGCHK(sg, sg.alloc(&sp.cn2, nb * n));
    STGCHK(sg, sg.alloc(&sp.perm, nb * n));
    STGCHK(sg, sg.alloc(&sp.out_U, nb * m * ns_max)); STGCHK(sg, sg.alloc(&sp.out_S, nb * ns_max));
    STGCHK(sg, sg.alloc(&sp.out_V, nb * n * ns_max)); STGCHK(sg, sg.alloc(&sp.out_info, nb * 4));
    STGCHK(sg, sg.upload(dgrid, grid, (size_t)n_grid)); STGCHK(sg, sg.upload(dom, omega, n)); STGCHK(sg, sg.upload(ddel, delta, n));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    fill(sg.stream, dgrid, dom, dKt0);
    STGCHK(sg, hipGetLastError());
    for (int ib = 0; ib < n_b; ++ib) {
        double* Ai = sp.A + (size_t)ib * n * m;
        const double b = preblur_b[ib];
        if (b > 0.0) {
            hipLaunchKernelGGL(mxe::preblur_rows, dim3(n_omega), dim3(256), 0, sg.stream, dom, ddel, b, n_omega, dr1);
            hipLaunchKernelGGL(mxe::preblur_cols, dim3(n_omega), dim3(256), 0, sg.stream, dom, ddel, b, n_omega, dr1, ddc);
            hipLaunchKernelGGL(mxe::preblur_matrix, dim3((n_omega * n_omega + 255) / 256), dim3(256), 0, sg.stream, dom, b, n_omega, dr1, ddc, dB);
            hipLaunchKernelGGL(mxe::preblur_product, dim3(n_omega), dim3(256), n * 8, sg.stream, dKt0, ddel, dB, m_rows, n_omega, Ai);
            STGCHK(sg, hipGetLastError());
        } else {
            STGCHK(sg, hipMemcpyAsync(Ai, dKt0, n * m * 8, hipMemcpyDeviceToDevice, sg.stream));
        }
    }
    // K^T and the info words go through host vectors: K is transposed, the info words are unpacked below
    std::vector<double> hKt(out_K ? nb * n * m : 0);
    STGCHK(sg, sg.fetch(hKt.data(), sp.A, hKt.size()));
    STGCHK(sg, launch_lds(mxe::svd_kernel, dim3(n_b), dim3(mxe::SVD_T), lds, sg.stream, sp));
    STGCHK(sg, sg.time_end());
    std::vector<int> hinfo(nb * 4);
    STGCHK(sg, sg.fetch(out_U, sp.out_U, nb * m * ns_max)); STGCHK(sg, sg.fetch(out_S, sp.out_S, nb * ns_max));
    STGCHK(sg, sg.fetch(out_V, sp.out_V, nb * n * ns_max)); STGCHK(sg, sg.fetch(hinfo.data(), sp.out_info, hinfo.size()));
    STGCHK(sg, sg.finish(out_ms));
    int rc = MXE_OK;
    for (int ib = 0; ib < n_b; ++ib) {
        out_ns[ib] = hinfo[(size_t)ib * 4];
        if (out_info) { out_info[ib * 3] = hinfo[(size_t)ib * 4 + 1]; out_info[ib * 3 + 1] = hinfo[(size_t)ib * 4 + 2]; out_info[ib * 3 + 2] = hinfo[(size_t)ib * 4 + 3]; }
        const int status = hinfo[(size_t)ib * 4 + 3];
        if (status == 2 || status == 3) rc = MXE_ERR_LIMIT;       // (3: more than SVD_RCAP significant directions)
        else if (status == 1 && rc == MXE_OK) rc = MXE_ERR_NUMERIC;
        // a NaN that entered with the grids or the matrix passes every comparison of the decomposition as "false"
        // and comes out in S: never MXE_OK
        for (int k = 0; k < ns_max && rc == MXE_OK; ++k)
            if (std::isnan(out_S[(size_t)ib * ns_max + k])) rc = MXE_ERR_NUMERIC;
    }
    if (out_K)
        for (size_t ib = 0; ib < nb; ++ib)
            for (size_t j = 0; j < n; ++j)
                for (size_t i = 0; i < m; ++i)
                    out_K[(ib * m + i) * n + j] = hKt[(ib * n + j) * m + i];
    return rc;
}
} // namespace

extern "C" int mxe_kernel_svd(int device, int n_tau, int n_omega, const double* tau, const double* omega,
                              const double* delta, double beta, int n_b, const double* preblur_b,
                              double threshold, int ns_max, double* out_K, double* out_U, double* out_S,
                              double* out_V, int32_t* out_ns, int32_t* out_info, float* out_ms)
try {
    if (!svd_args_ok(n_tau, n_omega, n_b, tau, omega, delta, preblur_b, threshold, ns_max, out_U, out_S, out_V, out_ns))
        return MXE_ERR_ARG;
    return kernel_svd_common(device, n_tau, n_tau, n_omega, tau, omega, delta, n_b, preblur_b, threshold, ns_max,
                             out_K, out_U, out_S, out_V, out_ns, out_info, out_ms,
                             [=](hipStream_t st, const double* dtau, const double* dom, double* dKt0) {
        launch_fill(mxe::tau_kernel_fill, st, n_tau * n_omega, dtau, dom, beta, n_tau, n_omega, dKt0);
    });
}
MXE_CATCH_ALL

extern "C" int mxe_kernel_svd_iw(int device, int n_iw, int n_omega, const double* iomega, const double* omega,
                                 const double* delta, int n_b, const double* preblur_b, double threshold, int ns_max,
                                 double* out_K, double* out_U, double* out_S, double* out_V, int32_t* out_ns,
                                 int32_t* out_info, float* out_ms)
try {
    if (!svd_args_ok(n_iw, n_omega, n_b, iomega, omega, delta, preblur_b, threshold, ns_max, out_U, out_S, out_V, out_ns) ||
        n_iw > (1 << 29) / n_omega) return MXE_ERR_ARG;
    return kernel_svd_common(device, n_iw, 2 * n_iw, n_omega, iomega, omega, delta, n_b, preblur_b, threshold, ns_max,
                             out_K, out_U, out_S, out_V, out_ns, out_info, out_ms,
                             [=](hipStream_t st, const double* diw, const double* dom, double* dKt0) {
        launch_fill(mxe::iomega_kernel_fill, st, n_iw * n_omega, diw, dom, n_iw, n_omega, dKt0);
    });
}
MXE_CATCH_ALL

// BosonicTauKernel: K(tau, w) = w e^{-tau w} / (1 - e^{-beta w}); symmetric != 0: K(tau, w) + K(tau, -w) on w >= 0
extern "C" int mxe_kernel_svd_boson(int device, int n_tau, int n_omega, const double* tau, const double* omega,
                                    const double* delta, double beta, int symmetric, int n_b, const double* preblur_b,
                                    double threshold, int ns_max, double* out_K, double* out_U, double* out_S,
                                    double* out_V, int32_t* out_ns, int32_t* out_info, float* out_ms)
try {
    if (!svd_args_ok(n_tau, n_omega, n_b, tau, omega, delta, preblur_b, threshold, ns_max, out_U, out_S, out_V, out_ns) ||
        !(beta > 0.0) || n_tau > (1 << 30) / n_omega) return MXE_ERR_ARG;
    if (symmetric)
        for (int j = 0; j < n_omega; ++j) if (!(omega[j] >= 0.0)) return MXE_ERR_ARG;
    return kernel_svd_common(device, n_tau, n_tau, n_omega, tau, omega, delta, n_b, preblur_b, threshold, ns_max,
                             out_K, out_U, out_S, out_V, out_ns, out_info, out_ms,
                             [=](hipStream_t st, const double* dtau, const double* dom, double* dKt0) {
        launch_fill(mxe::boson_tau_kernel_fill, st, n_tau * n_omega, dtau, dom, beta, symmetric ? 1 : 0, n_tau, n_omega,
                    dKt0);
    });
}
MXE_CATCH_ALL

// BosonicIOmegaKernel: K(i nu_n, w) = w / (w - i nu_n), stacked real of 2 n_inu rows; symmetric != 0: the real
// 2 w^2 / (w^2 + nu_n^2) of n_inu rows on w >= 0
extern "C" int mxe_kernel_svd_boson_iw(int device, int n_inu, int n_omega, const double* inu, const double* omega,
                                       const double* delta, int symmetric, int n_b, const double* preblur_b,
                                       double threshold, int ns_max, double* out_K, double* out_U, double* out_S,
                                       double* out_V, int32_t* out_ns, int32_t* out_info, float* out_ms)
try {
    if (!svd_args_ok(n_inu, n_omega, n_b, inu, omega, delta, preblur_b, threshold, ns_max, out_U, out_S, out_V, out_ns) ||
        n_inu > (1 << 29) / n_omega) return MXE_ERR_ARG;
    if (symmetric)
        for (int j = 0; j < n_omega; ++j) if (!(omega[j] >= 0.0)) return MXE_ERR_ARG;
    return kernel_svd_common(device, n_inu, symmetric ? n_inu : 2 * n_inu, n_omega, inu, omega, delta, n_b, preblur_b,
                             threshold, ns_max, out_K, out_U, out_S, out_V, out_ns, out_info, out_ms,
                             [=](hipStream_t st, const double* dnu, const double* dom, double* dKt0) {
        launch_fill(mxe::boson_iomega_kernel_fill, st, n_inu * n_omega, dnu, dom, symmetric ? 1 : 0, n_inu, n_omega, dKt0);
    });
}
MXE_CATCH_ALL

// LegendreKernel: K(l, w) = -beta sqrt(2l+1) (-sgn w)^l i_l(beta |w| / 2) / (2 cosh(beta w / 2)), n_l rows.  The orders
// travel as the "row grid" of kernel_svd_common, followed by the row indices sorted by ascending order (the fill walks
// the orders downwards and upwards).  Everything the fill's loops depend on is checked here, before any launch.
extern "C" int mxe_kernel_svd_legendre(int device, int n_l, int n_omega, const double* l, const double* omega,
                                       const double* delta, double beta, int n_b, const double* preblur_b,
                                       double threshold, int ns_max, double* out_K, double* out_U, double* out_S,
                                       double* out_V, int32_t* out_ns, int32_t* out_info, float* out_ms)
try {
    if (!svd_args_ok(n_l, n_omega, n_b, l, omega, delta, preblur_b, threshold, ns_max, out_U, out_S, out_V, out_ns) ||
        !(beta > 0.0) || !std::isfinite(beta) || n_l > (1 << 29) / n_omega) return MXE_ERR_ARG;
    int l_max = 0;
    for (int i = 0; i < n_l; ++i) {
        if (!(l[i] >= 0.0) || !(l[i] <= (double)mxe::LEGENDRE_L_MAX) || l[i] != std::floor(l[i])) return MXE_ERR_ARG;
        l_max = std::max(l_max, (int)l[i]);
    }
    for (int j = 0; j < n_omega; ++j)
        if (!(beta * std::fabs(omega[j]) / 2.0 <= mxe::LEGENDRE_A_MAX)) return MXE_ERR_ARG;      // (also a NaN)
    std::vector<int> order(n_l);
    for (int i = 0; i < n_l; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [l](int x, int y) { return l[x] < l[y]; });
    for (int i = 1; i < n_l; ++i)
        if (l[order[i]] == l[order[i - 1]]) return MXE_ERR_ARG;                                  // (an order twice)
    std::vector<double> lgrid((size_t)2 * n_l);
    for (int i = 0; i < n_l; ++i) { lgrid[i] = l[i]; lgrid[(size_t)n_l + i] = (double)order[i]; }
    return kernel_svd_common(device, 2 * n_l, n_l, n_omega, lgrid.data(), omega, delta, n_b, preblur_b, threshold, ns_max,
                             out_K, out_U, out_S, out_V, out_ns, out_info, out_ms,
                             [=](hipStream_t st, const double* dl, const double* dom, double* dKt0) {
        launch_fill(mxe::legendre_kernel_fill, st, n_omega, dl, dom, beta, l_max, n_l, n_omega, dKt0);
    });
}
MXE_CATCH_ALL

// DataKernel: the decomposition (and the preblur products) of a matrix the caller filled; K: n_rows x n_omega, host,
// row-major.  It travels as the "row grid" of kernel_svd_common, and the fill is its transposition on the device.
extern "C" int mxe_kernel_svd_data(int device, int n_rows, int n_omega, const double* K, const double* omega,
                                   const double* delta, int n_b, const double* preblur_b, double threshold, int ns_max,
                                   double* out_K, double* out_U, double* out_S, double* out_V, int32_t* out_ns,
                                   int32_t* out_info, float* out_ms)
try {
    if (!svd_args_ok(n_rows, n_omega, n_b, K, omega, delta, preblur_b, threshold, ns_max, out_U, out_S, out_V, out_ns) ||
        n_rows > (1 << 30) / n_omega) return MXE_ERR_ARG;
    // (before the matrix is copied: kernel_svd_common would refuse the same rows after its own check)
    if (svd_lds_bytes(n_rows) > SVD_LDS_LIMIT) return MXE_ERR_LIMIT;
    // a caller's matrix may hold anything: NaN and Inf are refused before the launch
    if (!all_finite(K, (size_t)n_rows * n_omega)) return MXE_ERR_NUMERIC;
    return kernel_svd_common(device, n_rows * n_omega, n_rows, n_omega, K, omega, delta, n_b, preblur_b, threshold,
                             ns_max, out_K, out_U, out_S, out_V, out_ns, out_info, out_ms,
                             [=](hipStream_t st, const double* dK, const double*, double* dKt0) {
        hipLaunchKernelGGL(mxe::data_kernel_transpose, dim3((n_omega + 31) / 32, (n_rows + 31) / 32), dim3(32, 8), 0, st,
                           dK, n_rows, n_omega, dKt0);
    });
}
MXE_CATCH_ALL

// ---- the broadened Kramers-Kronig sum of get_G_w_from_A_w (mxe_kk.hip.h) -------------------
#include "mxe_kk.hip.h"

namespace {
template <int TS>
void kk_launch(hipStream_t st, const mxe::KKParams& p, int n_o_tiles, bool split)
{
    const dim3 grid((p.n_spec + TS - 1) / TS, n_o_tiles, split ? p.n_slice : 1);
    if (split) hipLaunchKernelGGL((mxe::kk_partial<TS, false>), grid, dim3(mxe::KK_T), 0, st, p);
    else       hipLaunchKernelGGL((mxe::kk_partial<TS, true>), grid, dim3(mxe::KK_T), 0, st, p);
}
} // namespace

extern "C" int mxe_kramers_kronig(int device, int n_w, const double* w, const double* weight, const double* eta,
                                  int n_out, const double* w_out, int n_spec, const double* A,
                                  double* out_G, float* out_ms)
try {
    if (n_w < 1 || n_out < 1 || n_spec < 1 || !w || !weight || !eta || !w_out || !A || !out_G) return MXE_ERR_ARG;
    if ((int64_t)n_spec * n_out > INT32_MAX || (int64_t)n_spec * n_w > INT32_MAX) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    const int TS = n_spec <= 2 ? 2 : n_spec <= 8 ? 8 : 16;        // spectra per workgroup tile
    const int n_slice = (n_w + mxe::KK_SLICE - 1) / mxe::KK_SLICE;
    const int n_o_tiles = (n_out + mxe::KK_T - 1) / mxe::KK_T;
    const size_t n_res = (size_t)n_spec * n_out;                  // complex values of the result
    // few workgroups without splitting (few spectra): one workgroup per j slice, the partials added by kk_combine
    // (the same operations in the same order as one workgroup adding them as it goes: the same bits)
    const int64_t wgs = (int64_t)((n_spec + TS - 1) / TS) * n_o_tiles;
    const bool split = n_slice > 1 && n_slice <= 65535 && wgs < 1024 && (int64_t)n_slice * n_res * 16 <= ((int64_t)1 << 30);
    if (n_o_tiles > 65535) return MXE_ERR_LIMIT;                   // (the grid's y extent)
    double *dw, *dwt, *deta, *dwo, *dA, *dG, *dP = nullptr;
    const size_t nwz = n_w, n_A = (size_t)n_spec * n_w;
    STGCHK(sg, sg.alloc(&dw, nwz)); STGCHK(sg, sg.alloc(&dwt, nwz)); STGCHK(sg, sg.alloc(&deta, nwz));
    STGCHK(sg, sg.alloc(&dwo, (size_t)n_out)); STGCHK(sg, sg.alloc(&dA, n_A)); STGCHK(sg, sg.alloc(&dG, 2 * n_res));
    if (split) STGCHK(sg, sg.alloc(&dP, 2 * n_res * n_slice));
    STGCHK(sg, sg.upload(dw, w, nwz)); STGCHK(sg, sg.upload(dwt, weight, nwz)); STGCHK(sg, sg.upload(deta, eta, nwz));
    STGCHK(sg, sg.upload(dwo, w_out, (size_t)n_out)); STGCHK(sg, sg.upload(dA, A, n_A));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    mxe::KKParams p;
    p.w = dw; p.weight = dwt; p.eta = deta; p.w_out = dwo; p.A = dA; p.out = split ? dP : dG;
    p.n_w = n_w; p.n_out = n_out; p.n_spec = n_spec; p.n_slice = n_slice;
    if (TS == 2) kk_launch<2>(sg.stream, p, n_o_tiles, split);
    else if (TS == 8) kk_launch<8>(sg.stream, p, n_o_tiles, split);
    else kk_launch<16>(sg.stream, p, n_o_tiles, split);
    STGCHK(sg, hipGetLastError());
    if (split) {
        hipLaunchKernelGGL(mxe::kk_combine, dim3((unsigned)((n_res + 255) / 256)), dim3(256), 0, sg.stream,
                           (const double2*)dP, n_slice, n_res, (double2*)dG);
        STGCHK(sg, hipGetLastError());
    }
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_G, dG, 2 * n_res));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- binned Monte Carlo data: mean and covariance eigenbasis of every set in one launch (mxe_bins.hip.h) ----
#include "mxe_bins.hip.h"

extern "C" int mxe_bins_eig(int device, int n_sets, int n_bins, int n_data, const double* bins, double threshold,
                            double* out_mean, double* out_var, double* out_T, int32_t* out_rank, int32_t* out_sweeps)
try {
    if (n_sets < 1 || n_bins < 2 || n_data < 1 || n_data > mxe::BINS_NMAX || !bins || !out_mean || !out_var || !out_T ||
        !out_rank || !out_sweeps || !(threshold >= 0.0) || !std::isfinite(threshold)) return MXE_ERR_ARG;
    if ((int64_t)n_bins * n_data > INT32_MAX) return MXE_ERR_ARG;
    const size_t m = n_bins, n = n_data, ns = n_sets, nel = ns * m * n;
    if (!all_finite(bins, nel)) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::BinsParams p;
    p.m = n_bins; p.n = n_data;
    p.rcap = (std::min(n_bins, n_data) + 1) & ~1;
    p.scale = 1.0 / std::sqrt((double)n_bins * (double)(n_bins - 1));
    p.threshold = threshold;
    const double floor1 = (double)std::max(n_bins, n_data) * 2.220446049250313e-16;
    p.floor2 = floor1 * floor1;
    double* dbins;
    STGCHK(sg, sg.alloc(&dbins, nel));
    p.bins = dbins;
    STGCHK(sg, sg.alloc(&p.A, (n_bins > n_data) ? nel : 1));
    STGCHK(sg, sg.alloc(&p.Rm, ns * p.rcap * n)); STGCHK(sg, sg.alloc(&p.vk, ns * m));
    STGCHK(sg, sg.alloc(&p.part, ns * mxe::BINS_NWAVE * n * 2)); STGCHK(sg, sg.alloc(&p.cn2, ns * n));
    STGCHK(sg, sg.alloc(&p.perm, ns * n));
    STGCHK(sg, sg.alloc(&p.out_mean, ns * n)); STGCHK(sg, sg.alloc(&p.out_var, ns * n));
    STGCHK(sg, sg.alloc(&p.out_T, ns * n * n)); STGCHK(sg, sg.alloc(&p.out_info, ns * 4));
    STGCHK(sg, sg.upload(dbins, bins, nel));
    hipLaunchKernelGGL(mxe::bins_eig_kernel, dim3(n_sets), dim3(mxe::BINS_T), 0, sg.stream, p);
    STGCHK(sg, hipGetLastError());
    std::vector<int> hinfo(ns * 4);                           // (through a host vector: rank and sweeps are picked out of it below)
    STGCHK(sg, sg.fetch(out_mean, p.out_mean, ns * n)); STGCHK(sg, sg.fetch(out_var, p.out_var, ns * n));
    STGCHK(sg, sg.fetch(out_T, p.out_T, ns * n * n)); STGCHK(sg, sg.fetch(hinfo.data(), p.out_info, hinfo.size()));
    STGCHK(sg, sg.finish(nullptr));
    int rc = MXE_OK;
    for (size_t s = 0; s < ns; ++s) {
        out_rank[s] = hinfo[s * 4];
        out_sweeps[s] = hinfo[s * 4 + 2];
        if (hinfo[s * 4 + 3] != 0) rc = MXE_ERR_NUMERIC;      // (Jacobi sweeps exhausted, or squares that overflow)
    }
    return rc;
}
MXE_CATCH_ALL

// ---- few bins: shrinkage intensity and the eigenbasis of the shrunk covariance of the mean (mxe_shrink.hip.h) ----
#include "mxe_shrink.hip.h"

extern "C" int mxe_bins_eig_shrunk(int device, int n_sets, int n_bins, int n_data, const double* bins, double threshold,
                                   double lambda_in, double* out_mean, double* out_var, double* out_T, int32_t* out_rank,
                                   int32_t* out_sweeps, double* out_lambda, double* out_lambda_raw, double* out_diag,
                                   float* out_ms)
try {
    if (n_sets < 1 || n_bins < 2 || n_data < 1 || n_data > mxe::BINS_NMAX || !bins || !out_mean || !out_var || !out_T ||
        !out_rank || !out_sweeps || !(threshold >= 0.0) || !std::isfinite(threshold)) return MXE_ERR_ARG;
    if (!out_lambda || !out_lambda_raw || !out_diag || !(lambda_in <= 1.0)) return MXE_ERR_ARG;   // (a NaN fails the comparison)
    const bool estimate = lambda_in < 0.0;
    if (estimate && n_bins < 4) return MXE_ERR_ARG;
    if ((int64_t)n_bins * n_data > INT32_MAX) return MXE_ERR_ARG;
    const size_t m = n_bins, n = n_data, ns = n_sets, nel = ns * m * n;
    const size_t M = m + n;                                   // rows of Y
    if (!all_finite(bins, nel)) return MXE_ERR_ARG;
    mxe::ShrinkParams sp;
    sp.m = n_bins; sp.n = n_data;
    sp.mp = (n_bins + 3) & ~3; sp.np = (n_data + 15) & ~15;
    const int ct = sp.np / 16;
    sp.nt = ct * (ct + 1) / 2;
    sp.wgs = (sp.nt + mxe::SHRINK_TW - 1) / mxe::SHRINK_TW;
    if ((int64_t)sp.wgs * n_sets > INT32_MAX) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::BinsParams p;
    p.m = n_bins; p.n = n_data;
    p.rcap = (n_data + 1) & ~1;
    p.scale = 1.0 / std::sqrt((double)n_bins * (double)(n_bins - 1));
    p.threshold = threshold;
    const double floor1 = (double)(n_bins + n_data) * 2.220446049250313e-16;
    p.floor2 = floor1 * floor1;
    double *dbins, *dlam, *draw, *ddiag;
    STGCHK(sg, sg.alloc(&dbins, nel));
    p.bins = dbins;
    STGCHK(sg, sg.alloc(&p.A, ns * n * M));
    STGCHK(sg, sg.alloc(&p.Rm, ns * p.rcap * n)); STGCHK(sg, sg.alloc(&p.vk, ns * M));
    STGCHK(sg, sg.alloc(&p.part, ns * mxe::BINS_NWAVE * n * 2)); STGCHK(sg, sg.alloc(&p.cn2, ns * n));
    STGCHK(sg, sg.alloc(&p.perm, ns * n));
    STGCHK(sg, sg.alloc(&p.out_mean, ns * n)); STGCHK(sg, sg.alloc(&p.out_var, ns * n));
    STGCHK(sg, sg.alloc(&p.out_T, ns * n * n)); STGCHK(sg, sg.alloc(&p.out_info, ns * 4));
    STGCHK(sg, sg.alloc(&dlam, ns)); STGCHK(sg, sg.alloc(&draw, ns)); STGCHK(sg, sg.alloc(&ddiag, ns * n));
    std::vector<double> hlam;                                 // (a fixed lambda: lives until the stream is waited for)
    if (estimate) {
        sp.bins = dbins; sp.part = p.part; sp.out_mean = p.out_mean; sp.lambda = dlam; sp.lambda_raw = draw;
        STGCHK(sg, sg.alloc(&sp.Z, ns * sp.mp * sp.np)); STGCHK(sg, sg.alloc(&sp.tpart, ns * sp.nt * 2));
    } else {
        hlam.assign(2 * ns, lambda_in);
        std::fill(hlam.begin() + ns, hlam.end(), std::nan(""));
        STGCHK(sg, sg.upload(dlam, hlam.data(), ns)); STGCHK(sg, sg.upload(draw, hlam.data() + ns, ns));
    }
    STGCHK(sg, sg.upload(dbins, bins, nel));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    if (estimate) {
        hipLaunchKernelGGL(mxe::shrink_prep_kernel, dim3(n_sets), dim3(mxe::BINS_T), 0, sg.stream, sp);
        STGCHK(sg, hipGetLastError());
        hipLaunchKernelGGL(mxe::shrink_gram_kernel, dim3((unsigned)(sp.wgs * n_sets)), dim3(64 * mxe::SHRINK_TW), 0, sg.stream, sp);
        STGCHK(sg, hipGetLastError());
        hipLaunchKernelGGL(mxe::shrink_lambda_kernel, dim3(n_sets), dim3(64), 0, sg.stream, sp);
        STGCHK(sg, hipGetLastError());
    }
    hipLaunchKernelGGL(mxe::bins_eig_shrunk_kernel, dim3(n_sets), dim3(mxe::BINS_T), 0, sg.stream, p,
                       (const double*)dlam, ddiag);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    std::vector<int> hinfo(ns * 4);
    STGCHK(sg, sg.fetch(out_mean, p.out_mean, ns * n)); STGCHK(sg, sg.fetch(out_var, p.out_var, ns * n));
    STGCHK(sg, sg.fetch(out_T, p.out_T, ns * n * n)); STGCHK(sg, sg.fetch(hinfo.data(), p.out_info, hinfo.size()));
    STGCHK(sg, sg.fetch(out_lambda, dlam, ns)); STGCHK(sg, sg.fetch(out_lambda_raw, draw, ns));
    STGCHK(sg, sg.fetch(out_diag, ddiag, ns * n));
    STGCHK(sg, sg.finish(out_ms));
    int rc = MXE_OK;
    for (size_t s = 0; s < ns; ++s) {
        out_rank[s] = hinfo[s * 4];
        out_sweeps[s] = hinfo[s * 4 + 2];
        if (hinfo[s * 4 + 3] != 0) rc = MXE_ERR_NUMERIC;
    }
    return rc;
}
MXE_CATCH_ALL

// ---- resampling of the bins: the rotated data of every jackknife / bootstrap resample, and the reduction of the
// ---- H rows they were continued to (mxe_resample.hip.h) ----
#include "mxe_resample.hip.h"

extern "C" int mxe_bins_resample(int device, int n_sets, int n_bins, int n_data, const double* bins,
                                 int n_res, const int32_t* counts, const double* T, const int32_t* rank,
                                 double* out_mean, double* out_G, double* out_dev, float* out_ms)
try {
    if (n_sets < 1 || n_bins < 2 || n_data < 1 || n_data > mxe::BINS_NMAX || !bins || n_res < 1 || !counts || !T || !rank ||
        !out_mean || !out_G) return MXE_ERR_ARG;
    if ((int64_t)n_bins * n_data > INT32_MAX || (int64_t)n_res * n_bins > INT32_MAX || (int64_t)n_res * n_data > INT32_MAX)
        return MXE_ERR_ARG;
    const size_t m = n_bins, n = n_data, ns = n_sets, nr = n_res, nel = ns * m * n;
    std::vector<double> hNr(nr);
    for (size_t r = 0; r < nr; ++r) {
        int64_t s = 0;
        for (size_t b = 0; b < m; ++b) {
            const int32_t c = counts[r * m + b];
            if (c < 0) return MXE_ERR_ARG;
            s += c;
        }
        if (s <= 0) return MXE_ERR_ARG;
        hNr[r] = (double)s;
    }
    for (size_t s = 0; s < ns; ++s) if (rank[s] < 0 || rank[s] > n_data) return MXE_ERR_ARG;
    if (!all_finite(bins, nel) || !all_finite(T, ns * n * n)) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::ResampleParams p;
    p.m = n_bins; p.n = n_data; p.n_res = n_res;
    double *dbins, *dNr, *dT;
    int *dcounts, *drank;
    STGCHK(sg, sg.alloc(&dbins, nel)); STGCHK(sg, sg.alloc(&dcounts, nr * m)); STGCHK(sg, sg.alloc(&dNr, nr));
    STGCHK(sg, sg.alloc(&dT, ns * n * n)); STGCHK(sg, sg.alloc(&drank, ns));
    STGCHK(sg, sg.alloc(&p.part, ns * mxe::BINS_NWAVE * n * 2)); STGCHK(sg, sg.alloc(&p.D, ns * nr * n));
    STGCHK(sg, sg.alloc(&p.out_mean, ns * n)); STGCHK(sg, sg.alloc(&p.out_G, ns * nr * n)); STGCHK(sg, sg.alloc(&p.out_dev, ns * nr * n));
    p.bins = dbins; p.counts = dcounts; p.Nr = dNr; p.T = dT; p.rank = drank;
    STGCHK(sg, sg.upload(dbins, bins, nel)); STGCHK(sg, sg.upload(dcounts, counts, nr * m));
    STGCHK(sg, sg.upload(dNr, hNr.data(), nr)); STGCHK(sg, sg.upload(dT, T, ns * n * n)); STGCHK(sg, sg.upload(drank, rank, ns));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    hipLaunchKernelGGL(mxe::bins_resample_kernel, dim3(n_sets), dim3(mxe::BINS_T), 0, sg.stream, p);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_mean, p.out_mean, ns * n)); STGCHK(sg, sg.fetch(out_G, p.out_G, ns * nr * n));
    STGCHK(sg, sg.fetch(out_dev, p.out_dev, ns * nr * n));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_resample_reduce(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, const double* H,
                                   const int32_t* problem_index, const double* scale, int n_f, const double* F,
                                   double* out_mean, double* out_var, double* out_fval, double* out_fmean, double* out_fcov,
                                   int32_t* out_used, float* out_ms)
try {
    if (!ctx || n_groups < 1 || !group_offset || !scale || n_f < 0 || (n_f > 0 && !F)) return MXE_ERR_ARG;
    if (!group_offsets_ok(group_offset, n_groups) || !all_finite(scale, n_groups)) return MXE_ERR_ARG;
    if (!H && !ctx->launched) return MXE_ERR_STATE;
    const size_t rows = (size_t)group_offset[n_groups], nw = ctx->n_omega, nf = n_f, ng = n_groups;
    if (rows * nw > 0x7fffffffull || rows * std::max<size_t>(nf, 1) > 0x7fffffffull || nf * nw > 0x7fffffffull ||
        ng * nw > 0x7fffffffull || ng * nf * nf > 0x7fffffffull) return MXE_ERR_ARG;
    Block bi;                                                 // rr_i
    const size_t iO = bi.add(ng + 1);                         // offsets [ng + 1]
    const size_t iK = bi.add(rows);                           // scratch flags [rows]
    const size_t iU = bi.add(ng);                             // used [ng]
    const size_t iR = bi.add(H ? 0 : rows);                   // rows of the launch [rows] (H == NULL)
    std::vector<int> hi(group_offset, group_offset + ng + 1);
    hi.resize(bi.total, 0);
    if (!H && !launch_rows(problem_index, rows, (size_t)ctx->n_chain * ctx->n_alpha, hi.data() + iR)) return MXE_ERR_ARG;
    if (!all_finite(F, nf * nw)) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(ctx); rc != MXE_OK) return rc;
    Block b;                                                  // rr_d
    const size_t oS = b.add(ng);                              // scale [ng]
    const size_t oH = b.add(H ? rows * nw : 0);               // H [rows][nw], when handed in
    const size_t oF = b.add(nf * nw);                         // F [nf][nw]
    const size_t oV = b.add(rows * nf);                       // fval [rows][nf]
    const size_t oM = b.add(ng * nw);                         // mean [ng][nw]
    const size_t oVar = b.add(ng * nw);                       // var [ng][nw]
    const size_t oFm = b.add(ng * nf);                        // fmean [ng][nf]
    const size_t oFc = b.add(ng * nf * nf);                   // fcov [ng][nf][nf]
    STGCHK(sg, ctx->rr_d.ensure(b.total));
    STGCHK(sg, ctx->rr_i.ensure(bi.total));
    double* d = ctx->rr_d.p;
    int* di = ctx->rr_i.p;
    STGCHK(sg, sg.upload(d + oS, scale, ng)); STGCHK(sg, sg.upload(d + oH, H, rows * nw));
    STGCHK(sg, sg.upload(d + oF, F, nf * nw)); STGCHK(sg, sg.upload(di, hi.data(), bi.total));
    mxe::ReduceParams rp;
    rp.H = H ? d + oH : ctx->dout_H.p; rp.row = H ? nullptr : di + iR;
    rp.off = di + iO; rp.scale = d + oS; rp.F = d + oF; rp.nw = (int)nw; rp.n_f = n_f;
    rp.ok = di + iK; rp.fval = d + oV; rp.mean = d + oM; rp.var = d + oVar; rp.fmean = d + oFm; rp.fcov = d + oFc; rp.used = di + iU;
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    hipLaunchKernelGGL(mxe::resample_reduce_kernel, dim3((unsigned)n_groups), dim3(256), 0, ctx->stream, rp);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_mean, d + oM, ng * nw)); STGCHK(sg, sg.fetch(out_var, d + oVar, ng * nw));
    STGCHK(sg, sg.fetch(out_fval, d + oV, rows * nf)); STGCHK(sg, sg.fetch(out_fmean, d + oFm, ng * nf));
    STGCHK(sg, sg.fetch(out_fcov, d + oFc, ng * nf * nf));
    std::vector<int> hused(out_used ? ng : 0);                // (int32_t for the caller: through a host vector)
    STGCHK(sg, sg.fetch(hused.data(), di + iU, hused.size()));
    STGCHK(sg, sg.finish(out_ms));
    std::copy(hused.begin(), hused.end(), out_used);
    return MXE_OK;
}
MXE_CATCH_ALL

extern "C" int mxe_resample_quantiles(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, const double* H,
                                      const int32_t* problem_index, int n_q, const double* q,
                                      double* out_q, int32_t* out_used, float* out_ms)
try {
    static_assert(mxe::RQ_MAX_ROWS == MXE_QUANTILE_MAX_ROWS, "the cap the header names is the one the kernel is built for");
    if (!ctx || n_groups < 1 || !group_offset || n_q < 1 || !q) return MXE_ERR_ARG;
    int longest = 0;
    if (!group_offsets_ok(group_offset, n_groups, &longest)) return MXE_ERR_ARG;
    for (int k = 0; k < n_q; ++k) if (!(q[k] >= 0.0 && q[k] <= 1.0)) return MXE_ERR_ARG;
    if (!H && !ctx->launched) return MXE_ERR_STATE;
    const size_t rows = (size_t)group_offset[n_groups], nw = ctx->n_omega, nq = n_q, ng = n_groups;
    if (rows * nw > 0x7fffffffull || ng * nq * nw > 0x7fffffffull || (nw + mxe::RQ_COLS - 1) / mxe::RQ_COLS > 65535) return MXE_ERR_ARG;
    Block bi;                                                 // rr_i
    const size_t iO = bi.add(ng + 1);                         // offsets [ng + 1]
    const size_t iK = bi.add(rows);                           // flags [rows]
    const size_t iU = bi.add(ng);                             // used [ng]
    const size_t iR = bi.add(H ? 0 : rows);                   // rows of the launch [rows] (H == NULL)
    std::vector<int> hi(group_offset, group_offset + ng + 1);
    hi.resize(bi.total, 0);
    if (!H && !launch_rows(problem_index, rows, (size_t)ctx->n_chain * ctx->n_alpha, hi.data() + iR)) return MXE_ERR_ARG;
    if (longest > mxe::RQ_MAX_ROWS) return MXE_ERR_LIMIT;
    int padded = 2;
    while (padded < longest) padded <<= 1;
    const size_t lds = (size_t)padded * mxe::RQ_COLS * sizeof(double);
    Stage sg;
    if (int rc = sg.open(ctx); rc != MXE_OK) return rc;
    Block b;                                                  // rr_d
    const size_t oQ = b.add(nq);                              // q [nq]
    const size_t oH = b.add(H ? rows * nw : 0);               // H [rows][nw], when handed in
    const size_t oO = b.add(ng * nq * nw);                    // quantiles [ng][nq][nw]
    STGCHK(sg, ctx->rr_d.ensure(b.total));
    STGCHK(sg, ctx->rr_i.ensure(bi.total));
    double* d = ctx->rr_d.p;
    int* di = ctx->rr_i.p;
    STGCHK(sg, sg.upload(d + oQ, q, nq)); STGCHK(sg, sg.upload(d + oH, H, rows * nw));
    STGCHK(sg, sg.upload(di, hi.data(), bi.total));
    mxe::QuantileParams qp;
    qp.H = H ? d + oH : ctx->dout_H.p; qp.row = H ? nullptr : di + iR;
    qp.off = di + iO; qp.q = d + oQ; qp.nw = (int)nw; qp.n_q = n_q; qp.rows = (int)rows; qp.padded = padded;
    qp.ok = di + iK; qp.out = d + oO; qp.used = di + iU;
    STGCHK(sg, hipFuncSetAttribute((const void*)mxe::resample_quantile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    if (rows) {
        hipLaunchKernelGGL(mxe::rows_finite_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ctx->stream, qp);
        STGCHK(sg, hipGetLastError());
    }
    hipLaunchKernelGGL(mxe::resample_quantile_kernel, dim3((unsigned)n_groups, (unsigned)((nw + mxe::RQ_COLS - 1) / mxe::RQ_COLS)),
                       dim3(256), lds, ctx->stream, qp);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    std::vector<double> hq(out_q ? ng * nq * nw : 0);    // (nothing is written to the caller's arrays before the stream is through)
    std::vector<int> hused(out_used ? ng : 0);
    STGCHK(sg, sg.fetch(hq.data(), d + oO, hq.size())); STGCHK(sg, sg.fetch(hused.data(), di + iU, hused.size()));
    STGCHK(sg, sg.finish(out_ms));
    std::copy(hq.begin(), hq.end(), out_q);
    std::copy(hused.begin(), hused.end(), out_used);
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- parametric bootstrap: mock data drawn from a continued spectrum with the noise of the job (mxe_mock.hip.h) ----
#include "mxe_mock.hip.h"

extern "C" int mxe_mock_data(int device, int n_sets, int n_mock, int n_data, int n_omega,
                             const double* K, const double* H0, const double* err, const double* T, const int32_t* rank,
                             uint64_t seed, const uint64_t* stream, double* out_model, double* out_G, float* out_ms)
try {
    if (n_sets < 1 || n_mock < 1 || n_data < 1 || n_omega < 1 || !K || !H0 || !err || !stream || !out_model || !out_G)
        return MXE_ERR_ARG;
    if ((T == nullptr) != (rank == nullptr)) return MXE_ERR_ARG;
    const size_t ns = n_sets, nm = n_mock, n = n_data, nw = n_omega;
    if (n * nw > 0x7fffffffull || ns * nw > 0x7fffffffull || ns * nm * n > 0x7fffffffull || 16 * n > 0x7fffffffull ||
        (T && ns * n * n > 0x7fffffffull)) return MXE_ERR_ARG;
    if (!all_finite(K, n * nw) || !all_finite(H0, ns * nw) || !all_finite(err, ns * n)) return MXE_ERR_ARG;
    for (size_t i = 0; i < ns * n; ++i) if (!(err[i] > 0.0)) return MXE_ERR_ARG;
    if (T) {
        for (size_t s = 0; s < ns; ++s) if (rank[s] < 0 || rank[s] > n_data) return MXE_ERR_ARG;
        if (!all_finite(T, ns * n * n)) return MXE_ERR_ARG;
    }
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    // chunks of mocks: MOCK_CHUNK each, more where gridDim.y would pass 1024
    size_t chunk = mxe::MOCK_CHUNK;
    while ((nm + chunk - 1) / chunk > 1024) chunk *= 2;
    const size_t gy = (nm + chunk - 1) / chunk, gx = (ns + 15) / 16;
    if (16 * chunk * ((n + 1) / 2) > 0x7fffffffull || gy * ns * n > 0x7fffffffull) return MXE_ERR_ARG;
    mxe::MockParams p;
    p.n_sets = n_sets; p.n_mock = n_mock; p.n_data = n_data; p.nw = n_omega; p.chunk = (int)chunk; p.seed = seed;
    double *dK, *dH0, *derr, *dT = nullptr;
    int* drank = nullptr;
    uint64_t* dstream;
    STGCHK(sg, sg.alloc(&dK, n * nw)); STGCHK(sg, sg.alloc(&dH0, ns * nw)); STGCHK(sg, sg.alloc(&derr, ns * n));
    STGCHK(sg, sg.alloc(&dstream, ns));
    if (T) { STGCHK(sg, sg.alloc(&dT, ns * n * n)); STGCHK(sg, sg.alloc(&drank, ns)); }
    STGCHK(sg, sg.alloc(&p.kh, T ? gy * ns * n : 1)); STGCHK(sg, sg.alloc(&p.mdl, gy * ns * n));
    STGCHK(sg, sg.alloc(&p.out_model, ns * n)); STGCHK(sg, sg.alloc(&p.out_G, ns * nm * n));
    p.K = dK; p.H0 = dH0; p.err = derr; p.T = dT; p.rank = drank; p.stream = dstream;
    STGCHK(sg, sg.upload(dK, K, n * nw)); STGCHK(sg, sg.upload(dH0, H0, ns * nw)); STGCHK(sg, sg.upload(derr, err, ns * n));
    STGCHK(sg, sg.upload(dstream, stream, ns));
    STGCHK(sg, sg.upload(dT, T, ns * n * n)); STGCHK(sg, sg.upload(drank, rank, ns));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    hipLaunchKernelGGL(mxe::mock_data_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(mxe::MOCK_T), 0, sg.stream, p);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_model, p.out_model, ns * n)); STGCHK(sg, sg.fetch(out_G, p.out_G, ns * nm * n));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- cross-validation over the bins: the out-of-sample chi2 of the H rows of training scans (mxe_cv.hip.h) ----
#include "mxe_cv.hip.h"

extern "C" int mxe_cv_score(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, const double* H,
                            const int32_t* problem_index, int n_data, int n_omega, const double* K,
                            const double* T, const int32_t* rank, const double* Gval, const double* w,
                            double* out_score, double* out_z, int32_t* out_used, float* out_ms)
try {
    if (!ctx || n_groups < 1 || n_data < 1 || n_omega < 1 || !group_offset || !K || !Gval || !w || !out_score) return MXE_ERR_ARG;
    if ((T == nullptr) != (rank == nullptr)) return MXE_ERR_ARG;
    if (!group_offsets_ok(group_offset, n_groups)) return MXE_ERR_ARG;
    if (!H && !ctx->launched) return MXE_ERR_STATE;
    if (!H && n_omega != ctx->n_omega) return MXE_ERR_ARG;
    const size_t rows = (size_t)group_offset[n_groups], nw = n_omega, n = n_data, ng = n_groups;
    if (rows * nw > 0x7fffffffull || rows * n > 0x7fffffffull || n * nw > 0x7fffffffull || ng * n > 0x7fffffffull ||
        (T && ng * n * n > 0x7fffffffull)) return MXE_ERR_ARG;
    if (T) for (size_t g = 0; g < ng; ++g) if (rank[g] < 0 || rank[g] > n_data) return MXE_ERR_ARG;
    if (!all_finite(K, n * nw) || !all_finite(Gval, ng * n) || !all_finite(w, ng * n) || (T && !all_finite(T, ng * n * n)))
        return MXE_ERR_ARG;
    for (size_t i = 0; i < ng * n; ++i) if (!(w[i] >= 0.0)) return MXE_ERR_ARG;
    size_t nt = 0;                                            // tiles of 16 rows, none across two groups
    for (size_t g = 0; g < ng; ++g) nt += ((size_t)(group_offset[g + 1] - group_offset[g]) + 15) / 16;
    Block bi;                                                 // rr_i
    const size_t iO = bi.add(ng + 1);                         // offsets [ng + 1]
    const size_t iRk = bi.add(ng);                            // rank [ng]
    const size_t iTg = bi.add(nt);                            // group of a tile [nt]
    const size_t iT0 = bi.add(nt);                            // first row of a tile [nt]
    const size_t iK = bi.add(rows);                           // flags [rows]
    const size_t iU = bi.add(ng);                             // used [ng]
    const size_t iR = bi.add(H ? 0 : rows);                   // rows of the launch [rows] (H == NULL)
    std::vector<int> hi(group_offset, group_offset + ng + 1);
    hi.resize(bi.total, 0);
    if (!H && !launch_rows(problem_index, rows, (size_t)ctx->n_chain * ctx->n_alpha, hi.data() + iR)) return MXE_ERR_ARG;
    for (size_t g = 0, t = 0; g < ng; ++g) {
        hi[iRk + g] = rank ? rank[g] : n_data;
        for (int r = group_offset[g]; r < group_offset[g + 1]; r += 16, ++t) { hi[iTg + t] = (int)g; hi[iT0 + t] = r; }
    }
    Stage sg;
    if (int rc = sg.open(ctx); rc != MXE_OK) return rc;
    Block b;                                                  // rr_d
    const size_t oK = b.add(n * nw);                          // K [n][nw]
    const size_t oH = b.add(H ? rows * nw : 0);               // H [rows][nw], when handed in
    const size_t oT = b.add(T ? ng * n * n : 0);              // T [ng][n][n]
    const size_t oG = b.add(ng * n);                          // Gval [ng][n]
    const size_t oW = b.add(ng * n);                          // w [ng][n]
    const size_t oM = b.add(T ? rows * n : 0);                // K H before the rotation [rows][n]
    const size_t oZ = b.add(rows * n);                        // z [rows][n]
    const size_t oS = b.add(rows);                            // score [rows]
    STGCHK(sg, ctx->rr_d.ensure(b.total));
    STGCHK(sg, ctx->rr_i.ensure(bi.total));
    double* d = ctx->rr_d.p;
    int* di = ctx->rr_i.p;
    STGCHK(sg, sg.upload(d + oK, K, n * nw)); STGCHK(sg, sg.upload(d + oH, H, rows * nw));
    STGCHK(sg, sg.upload(d + oT, T, ng * n * n)); STGCHK(sg, sg.upload(d + oG, Gval, ng * n));
    STGCHK(sg, sg.upload(d + oW, w, ng * n)); STGCHK(sg, sg.upload(di, hi.data(), bi.total));
    mxe::CvParams cp;
    cp.n = n_data; cp.nw = n_omega; cp.n_groups = n_groups;
    cp.K = d + oK; cp.H = H ? d + oH : ctx->dout_H.p; cp.row = H ? nullptr : di + iR;
    cp.off = di + iO; cp.tile_g = di + iTg; cp.tile_r0 = di + iT0;
    cp.T = T ? d + oT : nullptr; cp.rank = di + iRk; cp.Gval = d + oG; cp.w = d + oW;
    cp.kh = d + oM; cp.z = d + oZ; cp.score = d + oS; cp.ok = di + iK; cp.used = di + iU;
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    if (nt) {
        hipLaunchKernelGGL(mxe::cv_score_kernel, dim3((unsigned)nt), dim3(mxe::CV_T), 0, ctx->stream, cp);
        STGCHK(sg, hipGetLastError());
    }
    hipLaunchKernelGGL(mxe::cv_used_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, cp);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    std::vector<double> hs(rows), hz(out_z ? rows * n : 0);   // (nothing is written to the caller's arrays before the stream is through)
    std::vector<int> hused(out_used ? ng : 0);
    STGCHK(sg, sg.fetch(hs.data(), d + oS, hs.size())); STGCHK(sg, sg.fetch(hz.data(), d + oZ, hz.size()));
    STGCHK(sg, sg.fetch(hused.data(), di + iU, hused.size()));
    STGCHK(sg, sg.finish(out_ms));
    std::copy(hs.begin(), hs.end(), out_score);
    std::copy(hz.begin(), hz.end(), out_z);
    std::copy(hused.begin(), hused.end(), out_used);
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- default-model scans: the evidence of every scan, the model averages of every group of scans (mxe_evidence.hip.h) ----
#include "mxe_evidence.hip.h"

extern "C" int mxe_evidence_reduce(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, int n_alpha, const double* H,
                                   const int32_t* chain_index, const double* logp, const double* log_quad,
                                   const double* log_mix, const double* log_prior, int row_mode, const int32_t* pick,
                                   int n_f, const double* F,
                                   double* out_logZ, int32_t* out_kmax, int32_t* out_ngood, double* out_walpha,
                                   double* out_row, double* out_fval, double* out_wmodel, double* out_mean,
                                   double* out_between, double* out_fmean, double* out_fcov, int32_t* out_used, float* out_ms)
try {
    if (!ctx || n_groups < 1 || !group_offset || n_alpha < 1 || !logp || !log_quad || !log_mix || n_f < 0 || (n_f > 0 && !F) ||
        row_mode < 0 || row_mode > 2 || (row_mode == 2 && !pick)) return MXE_ERR_ARG;
    if (!group_offsets_ok(group_offset, n_groups)) return MXE_ERR_ARG;
    const size_t ns = (size_t)group_offset[n_groups], na = n_alpha, nw = ctx->n_omega, nf = n_f, ng = n_groups;
    const size_t lim = 0x7fffffffull;
    if (ns * na > lim || (H && ns * na * nw > lim) || ns * nw > lim || ns * std::max<size_t>(nf, 1) > lim || nf * nw > lim ||
        ng * nw > lim || ng * nf * nf > lim) return MXE_ERR_ARG;
    if (!H && !ctx->launched) return MXE_ERR_STATE;
    std::vector<long long> hrow0(std::max<size_t>(ns, 1));
    if (!H) {
        if (n_alpha != ctx->n_alpha) return MXE_ERR_ARG;
        for (size_t s = 0; s < ns; ++s) {
            const int c = chain_index ? chain_index[s] : (int)s;
            if (c < 0 || c >= ctx->n_chain) return MXE_ERR_ARG;
            hrow0[s] = (long long)c * n_alpha;
        }
    } else {
        for (size_t s = 0; s < ns; ++s) hrow0[s] = (long long)(s * na);
    }
    if (row_mode == 2)
        for (size_t s = 0; s < ns; ++s) if (pick[s] >= n_alpha) return MXE_ERR_ARG;
    if (!all_finite(log_quad, na) || !all_finite(log_mix, na) || !all_finite(F, nf * nw)) return MXE_ERR_ARG;
    if (log_prior)
        for (size_t s = 0; s < ns; ++s)
            if (std::isnan(log_prior[s]) || log_prior[s] == INFINITY) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(ctx); rc != MXE_OK) return rc;
    Block b;                                                  // er_d
    const size_t oH = b.add(H ? ns * na * nw : 0);            // H [ns][na][nw], when handed in (first: its rows start on 16 bytes where nw is even)
    const size_t oP = b.add(ns * na);                         // logp [ns][na]
    const size_t oQ = b.add(na);                              // log_quad [na]
    const size_t oX = b.add(na);                              // log_mix [na]
    const size_t oPr = b.add(ns);                             // log_prior [ns]
    const size_t oF = b.add(nf * nw);                         // F [nf][nw]
    const size_t oZ = b.add(ns);                              // logZ [ns]
    const size_t oW = b.add(ns * na);                         // walpha [ns][na]
    const size_t oR = b.add(ns * nw);                         // row [ns][nw]
    const size_t oV = b.add(ns * nf);                         // fval [ns][nf]
    const size_t oU = b.add(ns);                              // wmodel [ns]
    const size_t oM = b.add(ng * nw);                         // mean [ng][nw]
    const size_t oB = b.add(ng * nw);                         // between [ng][nw]
    const size_t oFm = b.add(ng * nf);                        // fmean [ng][nf]
    const size_t oFc = b.add(ng * nf * nf);                   // fcov [ng][nf][nf]
    Block bi;                                                 // er_i
    const size_t iO = bi.add(ng + 1);                         // offsets [ng + 1]
    const size_t iP = bi.add(ns);                             // pick [ns]
    const size_t iG = bi.add(ns * na);                        // good [ns][na]
    const size_t iUs = bi.add(ns);                            // usable [ns]
    const size_t iK = bi.add(ns);                             // kmax [ns]
    const size_t iN = bi.add(ns);                             // ngood [ns], behind kmax: fetched with it
    const size_t iU = bi.add(ng);                             // used [ng]
    STGCHK(sg, ctx->er_d.ensure(b.total));
    STGCHK(sg, ctx->er_i.ensure(bi.total));
    STGCHK(sg, ctx->er_l.ensure(hrow0.size()));
    double* d = ctx->er_d.p;
    int* di = ctx->er_i.p;
    std::vector<int> hi(group_offset, group_offset + ng + 1);
    hi.resize(iG, 0);
    if (row_mode == 2) for (size_t s = 0; s < ns; ++s) hi[iP + s] = pick[s];
    std::vector<double> hprior(std::max<size_t>(ns, 1), 0.0);
    if (log_prior) for (size_t s = 0; s < ns; ++s) hprior[s] = log_prior[s];
    STGCHK(sg, sg.upload(d + oH, H, ns * na * nw)); STGCHK(sg, sg.upload(d + oP, logp, ns * na));
    STGCHK(sg, sg.upload(d + oQ, log_quad, na)); STGCHK(sg, sg.upload(d + oX, log_mix, na));
    STGCHK(sg, sg.upload(d + oPr, hprior.data(), ns)); STGCHK(sg, sg.upload(d + oF, F, nf * nw));
    STGCHK(sg, sg.upload(di + iO, hi.data(), iG)); STGCHK(sg, sg.upload(ctx->er_l.p, hrow0.data(), hrow0.size()));
    mxe::EvidenceParams ep;
    ep.H = H ? d + oH : ctx->dout_H.p; ep.row0 = ctx->er_l.p;
    ep.logp = d + oP; ep.log_quad = d + oQ; ep.log_mix = d + oX; ep.log_prior = d + oPr; ep.pick = di + iP; ep.off = di + iO;
    ep.F = d + oF; ep.n_alpha = n_alpha; ep.nw = (int)nw; ep.n_f = n_f; ep.row_mode = row_mode;
    ep.good = di + iG; ep.usable = di + iUs; ep.logZ = d + oZ; ep.kmax = di + iK; ep.ngood = di + iN; ep.walpha = d + oW;
    ep.row = d + oR; ep.fval = d + oV; ep.wmodel = d + oU; ep.mean = d + oM; ep.between = d + oB; ep.fmean = d + oFm;
    ep.fcov = d + oFc; ep.used = di + iU;
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    if (ns) {
        hipLaunchKernelGGL(mxe::evidence_scan_kernel, dim3((unsigned)ns), dim3(mxe::EV_T), 0, ctx->stream, ep);
        STGCHK(sg, hipGetLastError());
    }
    hipLaunchKernelGGL(mxe::evidence_group_kernel, dim3((unsigned)ng), dim3(mxe::EV_T), 0, ctx->stream, ep);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_logZ, d + oZ, ns)); STGCHK(sg, sg.fetch(out_walpha, d + oW, ns * na));
    STGCHK(sg, sg.fetch(out_row, d + oR, ns * nw)); STGCHK(sg, sg.fetch(out_fval, d + oV, ns * nf));
    STGCHK(sg, sg.fetch(out_wmodel, d + oU, ns)); STGCHK(sg, sg.fetch(out_mean, d + oM, ng * nw));
    STGCHK(sg, sg.fetch(out_between, d + oB, ng * nw)); STGCHK(sg, sg.fetch(out_fmean, d + oFm, ng * nf));
    STGCHK(sg, sg.fetch(out_fcov, d + oFc, ng * nf * nf));
    std::vector<int> hout(2 * ns + ng);                   // kmax | ngood (back to back on the device) | used
    STGCHK(sg, sg.fetch(hout.data(), di + iK, 2 * ns)); STGCHK(sg, sg.fetch(hout.data() + 2 * ns, di + iU, ng));
    STGCHK(sg, sg.finish(out_ms));
    for (size_t s = 0; s < ns; ++s) {
        if (out_kmax) out_kmax[s] = hout[s];
        if (out_ngood) out_ngood[s] = hout[ns + s];
    }
    if (out_used) for (size_t g = 0; g < ng; ++g) out_used[g] = hout[2 * ns + g];
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- bin checks: the blocking ladder and the normality of the block means of every set (mxe_bincheck.hip.h) ----
#include "mxe_bincheck.hip.h"

extern "C" int mxe_bins_check(int device, int n_sets, int n_bins, int n_data, const double* bins,
                              const double* T, const int32_t* rank,
                              double* out_mean, double* out_err2, double* out_skew, double* out_kurt,
                              int32_t* out_levels, float* out_ms)
try {
    if (n_sets < 1 || n_bins < 2 || n_data < 1 || n_data > mxe::BINS_NMAX || !bins || !out_mean || !out_err2 || !out_skew ||
        !out_kurt || !out_levels || (T == nullptr) != (rank == nullptr)) return MXE_ERR_ARG;
    if ((int64_t)n_bins * n_data > INT32_MAX) return MXE_ERR_ARG;
    const size_t m = n_bins, n = n_data, ns = n_sets, nel = ns * m * n;
    if (rank)
        for (size_t s = 0; s < ns; ++s) if (rank[s] < 0 || rank[s] > n_data) return MXE_ERR_ARG;
    if (!all_finite(bins, nel) || (T && !all_finite(T, ns * n * n))) return MXE_ERR_ARG;
    int L = 0;
    while ((n_bins >> (L + 1)) >= 1) ++L;                             // floor(log2 n_bins): every level has two blocks or more
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::BinCheckParams p;
    p.m = n_bins; p.n = n_data; p.L = L;
    const size_t nout = ns * (size_t)L * n;
    double *dbins, *dT = nullptr;
    int* drank = nullptr;
    STGCHK(sg, sg.alloc(&dbins, nel));
    if (T) { STGCHK(sg, sg.alloc(&dT, ns * n * n)); STGCHK(sg, sg.alloc(&drank, ns)); }
    STGCHK(sg, sg.alloc(&p.part, ns * mxe::BINS_NWAVE * n * 2)); STGCHK(sg, sg.alloc(&p.part2, ns * mxe::BINS_NWAVE * n * 3));
    STGCHK(sg, sg.alloc(&p.Y0, nel)); STGCHK(sg, sg.alloc(&p.Y1, ns * (m >> 1) * n));
    STGCHK(sg, sg.alloc(&p.out_mean, ns * n)); STGCHK(sg, sg.alloc(&p.out_err2, nout));
    STGCHK(sg, sg.alloc(&p.out_skew, nout)); STGCHK(sg, sg.alloc(&p.out_kurt, nout));
    p.bins = dbins; p.T = dT; p.rank = drank;
    STGCHK(sg, sg.upload(dbins, bins, nel)); STGCHK(sg, sg.upload(dT, T, ns * n * n)); STGCHK(sg, sg.upload(drank, rank, ns));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    hipLaunchKernelGGL(mxe::bins_check_kernel, dim3(n_sets), dim3(mxe::BINS_T), 0, sg.stream, p);
    STGCHK(sg, hipGetLastError());
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_mean, p.out_mean, ns * n)); STGCHK(sg, sg.fetch(out_err2, p.out_err2, nout));
    STGCHK(sg, sg.fetch(out_skew, p.out_skew, nout)); STGCHK(sg, sg.fetch(out_kurt, p.out_kurt, nout));
    STGCHK(sg, sg.finish(out_ms));
    out_levels[0] = L;
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- positivity of a matrix-valued spectral function: batched Hermitian eigenproblems (mxe_hermeig.hip.h) ----
#include "mxe_hermeig.hip.h"

extern "C" int mxe_hermitian_eig(int device, int n_mat, int m, int is_complex, const double* A, double floor,
                                 double* out_lambda, double* out_vec, double* out_proj, double* out_neg, double* out_dist,
                                 double* out_pair, double* out_asym, int32_t* out_info, float* out_ms)
try {
    static_assert(MXE_HERMEIG_MAX_M == mxe::HERMEIG_MAX_M, "the header and the kernel disagree on the largest matrix");
    if (n_mat < 1 || m < 1 || (is_complex != 0 && is_complex != 1) || !A || !std::isfinite(floor)) return MXE_ERR_ARG;
    if (m > mxe::HERMEIG_MAX_M) return MXE_ERR_LIMIT;
    const size_t nm = n_mat, mm = (size_t)m * m, w = is_complex ? 2 : 1;
    if (nm * mm * w > 0x7fffffffull) return MXE_ERR_ARG;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::HermEigParams p;
    std::memset(&p, 0, sizeof(p));
    p.n_mat = n_mat; p.m = m; p.floor = floor;
    double* dA;
    STGCHK(sg, sg.alloc(&dA, nm * mm * w));
    p.A = dA;
    if (out_lambda) STGCHK(sg, sg.alloc(&p.lambda, nm * m));
    if (out_vec) STGCHK(sg, sg.alloc(&p.vec, nm * mm * w));
    if (out_proj) STGCHK(sg, sg.alloc(&p.proj, nm * mm * w));
    if (out_neg) STGCHK(sg, sg.alloc(&p.neg, nm));
    if (out_dist) STGCHK(sg, sg.alloc(&p.dist, nm));
    if (out_pair) STGCHK(sg, sg.alloc(&p.pair, nm));
    if (out_asym) STGCHK(sg, sg.alloc(&p.asym, nm));
    if (out_info) STGCHK(sg, sg.alloc(&p.info, nm));
    STGCHK(sg, sg.upload(dA, A, nm * mm * w));
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    const bool wave = m <= mxe::HERMEIG_WAVE_M;
    const size_t slots = wave ? mxe::HERMEIG_T / 64 : 1;
    const size_t lds = slots * mxe::hermeig_slot_doubles(m, is_complex != 0) * sizeof(double);
    if (lds > 160 * 1024) return MXE_ERR_LIMIT;
    const auto kernel = is_complex ? (wave ? mxe::hermeig_kernel<true, 64> : mxe::hermeig_kernel<true, 256>)
                                   : (wave ? mxe::hermeig_kernel<false, 64> : mxe::hermeig_kernel<false, 256>);
    STGCHK(sg, launch_lds(kernel, dim3((unsigned)((nm + slots - 1) / slots)), dim3(mxe::HERMEIG_T), lds, sg.stream, p));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_lambda, p.lambda, nm * m)); STGCHK(sg, sg.fetch(out_vec, p.vec, nm * mm * w));
    STGCHK(sg, sg.fetch(out_proj, p.proj, nm * mm * w)); STGCHK(sg, sg.fetch(out_neg, p.neg, nm));
    STGCHK(sg, sg.fetch(out_dist, p.dist, nm)); STGCHK(sg, sg.fetch(out_pair, p.pair, nm));
    STGCHK(sg, sg.fetch(out_asym, p.asym, nm)); STGCHK(sg, sg.fetch(out_info, p.info, nm));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- whole-matrix continuation: H(omega) = D exp(Gamma(omega)), positive by construction (mxe_fullmatrix.hip.h) ----
#include "mxe_fullmatrix.hip.h"

// the two entries: c [n_s] (R and A NULL; the diagonal metric shared by all components) or R, A [P][n_s][n_s] (c NULL)
static int fullmatrix_solve_any(int device, int n_prob, int m, int is_complex, int n_omega, int n_s, int n_alpha,
                                const double* V, const double* c, const double* R, const double* A, bool metric,
                                const double* D, const double* alpha,
                                const double* ghat, const double* cperp, const double* u0, int maxiter, double tol_h,
                                double* out_u, double* out_H, double* out_chi2, double* out_S, double* out_Q,
                                int32_t* out_niter, int32_t* out_conv, float* out_ms)
{
    static_assert(MXE_FULLMATRIX_MAX_M == mxe::FM_MAX_M && MXE_FULLMATRIX_MAX_NS == mxe::FM_MAX_NS,
                  "the header and the kernel disagree on the limits");
    if (n_prob < 1 || m < 1 || (is_complex != 0 && is_complex != 1) || n_omega < 1 || n_s < 1 || n_alpha < 1 || maxiter < 0 ||
        !V || (metric ? (!R || !A) : !c) || !D || !alpha || !ghat || !cperp || !out_u || !out_H || !out_chi2 || !out_S || !out_Q || !out_niter ||
        !out_conv || !(tol_h > 0.0) || !std::isfinite(tol_h))
        return MXE_ERR_ARG;
    if (m > mxe::FM_MAX_M || n_s > mxe::FM_MAX_NS) return MXE_ERR_LIMIT;
    const bool cplx = is_complex != 0;
    const size_t np = n_prob, nw = n_omega, ns = n_s, na = n_alpha, P = mxe::fm_P(m, cplx), d = P * ns;
    const size_t mm = (size_t)m * m, hplanes = (cplx ? 2 : 1) * mm;
    const size_t scr = metric ? mxe::fm_scratch_doubles_metric(m, cplx, n_omega, n_s) : mxe::fm_scratch_doubles(m, cplx, n_omega, n_s);
    const size_t nc = metric ? 0 : ns, nr = metric ? P * ns * ns : 0;
    if (nw * ns > 0x7fffffffull || np * na * hplanes * nw > 0x7fffffffull || np * na * d > 0x7fffffffull ||
        P * (P + 1) / 2 * nw > 0x7fffffffull)
        return MXE_ERR_ARG;
    if (!all_finite(V, nw * ns) || (metric ? (!all_finite(R, nr) || !all_finite(A, nr)) : !all_finite(c, ns)) || !all_finite(D, nw) || !all_finite(alpha, na) ||
        !all_finite(ghat, np * d) || !all_finite(cperp, np) || (u0 && !all_finite(u0, np * d)))
        return MXE_ERR_ARG;
    for (size_t i = 0; i < nw; ++i) if (!(D[i] > 0.0)) return MXE_ERR_ARG;
    for (size_t k = 0; k < nc; ++k) if (!(c[k] > 0.0)) return MXE_ERR_ARG;
    for (size_t a = 0; a < na; ++a) if (!(alpha[a] > 0.0)) return MXE_ERR_ARG;
    const size_t lds = mxe::fm_lds_doubles((int)d) * sizeof(double);
    if (lds > 160 * 1024) return MXE_ERR_LIMIT;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::FullMatrixParams p;
    std::memset(&p, 0, sizeof(p));
    p.n_prob = n_prob; p.n_omega = n_omega; p.n_s = n_s; p.n_alpha = n_alpha; p.maxiter = maxiter;
    p.tol_h = tol_h; p.mu_first = 1e-3; p.mu_grow = 4.0; p.mu_max = 1e12;
    Block in;
    const size_t oV = in.add(nw * ns), oc = in.add(nc), oD = in.add(nw), oa = in.add(na), og = in.add(np * d),
                 op = in.add(np), o0 = in.add(u0 ? np * d : 0), oR = in.add(nr), oA = in.add(nr);
    double* din;
    STGCHK(sg, sg.alloc(&din, in.total));
    STGCHK(sg, sg.upload(din + oV, V, nw * ns)); STGCHK(sg, sg.upload(din + oc, c, nc));
    STGCHK(sg, sg.upload(din + oD, D, nw)); STGCHK(sg, sg.upload(din + oa, alpha, na));
    STGCHK(sg, sg.upload(din + og, ghat, np * d)); STGCHK(sg, sg.upload(din + op, cperp, np));
    STGCHK(sg, sg.upload(din + o0, u0, np * d));
    STGCHK(sg, sg.upload(din + oR, R, nr)); STGCHK(sg, sg.upload(din + oA, A, nr));
    p.V = din + oV; p.c = din + oc; p.D = din + oD; p.alpha = din + oa; p.ghat = din + og; p.cperp = din + op;
    p.u0 = u0 ? din + o0 : nullptr;
    if (metric) { p.c = nullptr; p.R = din + oR; p.A = din + oA; }
    STGCHK(sg, sg.alloc(&p.scratch, np * scr));
    Block out;
    const size_t ou = out.add(np * na * d), oH = out.add(np * na * hplanes * nw), ox = out.add(np * na), oS = out.add(np * na),
                 oQ = out.add(np * na);
    double* dout;
    STGCHK(sg, sg.alloc(&dout, out.total));
    int* dint;
    STGCHK(sg, sg.alloc(&dint, 2 * np * na));
    p.out_u = dout + ou; p.out_H = dout + oH; p.out_chi2 = dout + ox; p.out_S = dout + oS; p.out_Q = dout + oQ;
    p.out_niter = dint; p.out_conv = dint + np * na;
    typedef void (*kernel_t)(const mxe::FullMatrixParams);
    static const kernel_t kernels[2][4] = {
        {mxe::fullmatrix_kernel<1, false>, mxe::fullmatrix_kernel<2, false>, mxe::fullmatrix_kernel<3, false>,
         mxe::fullmatrix_kernel<4, false>},
        {mxe::fullmatrix_kernel<1, true>, mxe::fullmatrix_kernel<2, true>, mxe::fullmatrix_kernel<3, true>,
         mxe::fullmatrix_kernel<4, true>}};
    static const kernel_t metric_kernels[2][4] = {
        {mxe::fullmatrix_kernel<1, false, true>, mxe::fullmatrix_kernel<2, false, true>, mxe::fullmatrix_kernel<3, false, true>,
         mxe::fullmatrix_kernel<4, false, true>},
        {mxe::fullmatrix_kernel<1, true, true>, mxe::fullmatrix_kernel<2, true, true>, mxe::fullmatrix_kernel<3, true, true>,
         mxe::fullmatrix_kernel<4, true, true>}};
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    STGCHK(sg, launch_lds((metric ? metric_kernels : kernels)[cplx ? 1 : 0][m - 1], dim3((unsigned)np), dim3(mxe::FM_T), lds, sg.stream, p));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_u, p.out_u, np * na * d)); STGCHK(sg, sg.fetch(out_H, p.out_H, np * na * hplanes * nw));
    STGCHK(sg, sg.fetch(out_chi2, p.out_chi2, np * na)); STGCHK(sg, sg.fetch(out_S, p.out_S, np * na));
    STGCHK(sg, sg.fetch(out_Q, p.out_Q, np * na));
    STGCHK(sg, sg.fetch(out_niter, (int32_t*)p.out_niter, np * na)); STGCHK(sg, sg.fetch(out_conv, (int32_t*)p.out_conv, np * na));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}

extern "C" int mxe_fullmatrix_solve(int device, int n_prob, int m, int is_complex, int n_omega, int n_s, int n_alpha,
                                    const double* V, const double* c, const double* D, const double* alpha,
                                    const double* ghat, const double* cperp, const double* u0, int maxiter, double tol_h,
                                    double* out_u, double* out_H, double* out_chi2, double* out_S, double* out_Q,
                                    int32_t* out_niter, int32_t* out_conv, float* out_ms)
try {
    return fullmatrix_solve_any(device, n_prob, m, is_complex, n_omega, n_s, n_alpha, V, c, nullptr, nullptr, false, D, alpha,
                                ghat, cperp, u0, maxiter, tol_h, out_u, out_H, out_chi2, out_S, out_Q, out_niter, out_conv, out_ms);
}
MXE_CATCH_ALL

extern "C" int mxe_fullmatrix_solve_metric(int device, int n_prob, int m, int is_complex, int n_omega, int n_s, int n_alpha,
                                           const double* V, const double* R, const double* A, const double* D,
                                           const double* alpha, const double* ghat, const double* cperp, const double* u0,
                                           int maxiter, double tol_h, double* out_u, double* out_H, double* out_chi2,
                                           double* out_S, double* out_Q, int32_t* out_niter, int32_t* out_conv, float* out_ms)
try {
    return fullmatrix_solve_any(device, n_prob, m, is_complex, n_omega, n_s, n_alpha, V, nullptr, R, A, true, D, alpha,
                                ghat, cperp, u0, maxiter, tol_h, out_u, out_H, out_chi2, out_S, out_Q, out_niter, out_conv, out_ms);
}
MXE_CATCH_ALL

// ---- posterior variances of the whole-matrix continuation (mxe_fullmatrix_postvar.hip.h) ----
#include "mxe_fullmatrix_postvar.hip.h"

extern "C" int mxe_fullmatrix_posterior_var(int device, int n_job, int m, int is_complex, int n_omega, int n_s, int n_f,
                                            const double* V, const double* c, const double* D, const double* alpha,
                                            const double* u, const double* F, int want_diag,
                                            double* out_value, double* out_var, double* out_prior,
                                            double* out_diag_var, double* out_diag_prior, double* out_h, float* out_ms)
try {
    if (n_job < 1 || m < 1 || (is_complex != 0 && is_complex != 1) || n_omega < 1 || n_s < 1 || n_f < 0 ||
        (want_diag != 0 && want_diag != 1) || (n_f == 0 && !want_diag) || !V || !c || !D || !alpha || !u ||
        (n_f > 0 && (!F || !out_value || !out_var || !out_prior)) || (want_diag && (!out_diag_var || !out_diag_prior || !out_h)))
        return MXE_ERR_ARG;
    if (m > mxe::FM_MAX_M || n_s > mxe::FM_MAX_NS) return MXE_ERR_LIMIT;
    const bool cplx = is_complex != 0;
    const size_t nj = n_job, nw = n_omega, ns = n_s, nf = n_f, P = mxe::fm_P(m, cplx), d = P * ns, npw = P * nw;
    if (nw * ns > 0x7fffffffull || nj * npw > 0x7fffffffull || nj * d > 0x7fffffffull || nf * npw > 0x7fffffffull ||
        nj * nf > 0x7fffffffull || P * (P + 1) / 2 * nw > 0x7fffffffull || 16 * npw > 0x7fffffffull)
        return MXE_ERR_ARG;
    // (u is not looked at: a job whose u is not finite gets NaN from the kernel, its neighbours are not touched)
    if (!all_finite(V, nw * ns) || !all_finite(c, ns) || !all_finite(D, nw) || !all_finite(alpha, nj) || (nf && !all_finite(F, nf * npw)))
        return MXE_ERR_ARG;
    for (size_t i = 0; i < nw; ++i) if (!(D[i] > 0.0)) return MXE_ERR_ARG;
    for (size_t k = 0; k < ns; ++k) if (!(c[k] > 0.0)) return MXE_ERR_ARG;
    for (size_t a = 0; a < nj; ++a) if (!(alpha[a] > 0.0)) return MXE_ERR_ARG;
    const size_t lds = mxe::fmpv_lds_doubles((int)d) * sizeof(double);
    if (lds > 160 * 1024) return MXE_ERR_LIMIT;
    // the scratch: one slice per workgroup, as many workgroups as fit below MXE_FULLMATRIX_POSTVAR_SCRATCH_BYTES (one at least)
    const size_t scr = mxe::fmpv_scratch_doubles(m, cplx, n_omega, n_s);
    size_t n_slices = (size_t)MXE_FULLMATRIX_POSTVAR_SCRATCH_BYTES / (scr * sizeof(double));
    if (n_slices < 1) n_slices = 1;
    if (n_slices > nj) n_slices = nj;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::FullMatrixPostVarParams p;
    std::memset(&p, 0, sizeof(p));
    p.n_job = n_job; p.n_omega = n_omega; p.n_s = n_s; p.n_f = n_f; p.want_diag = want_diag;
    Block in;
    const size_t oV = in.add(nw * ns), oc = in.add(ns), oD = in.add(nw), oa = in.add(nj), ou = in.add(nj * d), oF = in.add(nf * npw);
    double* din;
    STGCHK(sg, sg.alloc(&din, in.total));
    STGCHK(sg, sg.upload(din + oV, V, nw * ns)); STGCHK(sg, sg.upload(din + oc, c, ns));
    STGCHK(sg, sg.upload(din + oD, D, nw)); STGCHK(sg, sg.upload(din + oa, alpha, nj));
    STGCHK(sg, sg.upload(din + ou, u, nj * d)); STGCHK(sg, sg.upload(din + oF, F, nf * npw));
    p.V = din + oV; p.c = din + oc; p.D = din + oD; p.alpha = din + oa; p.u = din + ou; p.F = nf ? din + oF : nullptr;
    STGCHK(sg, sg.alloc(&p.scratch, n_slices * scr));
    const size_t nd = want_diag ? nj * npw : 0;
    Block out;
    const size_t ox = out.add(nj * nf), ov = out.add(nj * nf), op = out.add(nj * nf), odv = out.add(nd), odp = out.add(nd),
                 oh = out.add(nd);
    double* dout;
    STGCHK(sg, sg.alloc(&dout, out.total));
    p.out_value = dout + ox; p.out_var = dout + ov; p.out_prior = dout + op;
    p.out_diag = dout + odv; p.out_dprior = dout + odp; p.out_h = dout + oh;
    typedef void (*kernel_t)(const mxe::FullMatrixPostVarParams);
    static const kernel_t kernels[2][4] = {
        {mxe::fullmatrix_postvar_kernel<1, false>, mxe::fullmatrix_postvar_kernel<2, false>,
         mxe::fullmatrix_postvar_kernel<3, false>, mxe::fullmatrix_postvar_kernel<4, false>},
        {mxe::fullmatrix_postvar_kernel<1, true>, mxe::fullmatrix_postvar_kernel<2, true>,
         mxe::fullmatrix_postvar_kernel<3, true>, mxe::fullmatrix_postvar_kernel<4, true>}};
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    STGCHK(sg, launch_lds(kernels[cplx ? 1 : 0][m - 1], dim3((unsigned)n_slices), dim3(mxe::FM_T), lds, sg.stream, p));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_value, p.out_value, nj * nf)); STGCHK(sg, sg.fetch(out_var, p.out_var, nj * nf));
    STGCHK(sg, sg.fetch(out_prior, p.out_prior, nj * nf));
    STGCHK(sg, sg.fetch(out_diag_var, p.out_diag, nd)); STGCHK(sg, sg.fetch(out_diag_prior, p.out_dprior, nd));
    STGCHK(sg, sg.fetch(out_h, p.out_h, nd));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL

// ---- the evidence of alpha of the whole-matrix continuation (mxe_fullmatrix_logdet.hip.h) ----
#include "mxe_fullmatrix_logdet.hip.h"

extern "C" int mxe_fullmatrix_logdet(int device, int n_job, int m, int is_complex, int n_omega, int n_s,
                                     const double* V, const double* c, const double* D, const double* alpha, const double* u,
                                     int want_ngood, double* out_logdet, double* out_ngood, float* out_ms)
try {
    if (n_job < 1 || m < 1 || (is_complex != 0 && is_complex != 1) || n_omega < 1 || n_s < 1 ||
        (want_ngood != 0 && want_ngood != 1) || !V || !c || !D || !alpha || !u || !out_logdet || (want_ngood && !out_ngood))
        return MXE_ERR_ARG;
    if (m > mxe::FM_MAX_M || n_s > mxe::FM_MAX_NS) return MXE_ERR_LIMIT;
    const bool cplx = is_complex != 0;
    const size_t nj = n_job, nw = n_omega, ns = n_s, P = mxe::fm_P(m, cplx), d = P * ns;
    // (what the kernel indexes with an int: V, u, and L, the largest of a job's arrays of n_omega)
    if (nw * ns > 0x7fffffffull || nj * d > 0x7fffffffull || P * (P + 1) / 2 * nw > 0x7fffffffull) return MXE_ERR_ARG;
    // (u is not looked at: a job whose u is not finite gets NaN from the kernel, its neighbours are not touched)
    if (!all_finite(V, nw * ns) || !all_finite(c, ns) || !all_finite(D, nw) || !all_finite(alpha, nj)) return MXE_ERR_ARG;
    for (size_t i = 0; i < nw; ++i) if (!(D[i] > 0.0)) return MXE_ERR_ARG;
    for (size_t k = 0; k < ns; ++k) if (!(c[k] > 0.0)) return MXE_ERR_ARG;
    for (size_t a = 0; a < nj; ++a) if (!(alpha[a] > 0.0)) return MXE_ERR_ARG;
    const size_t lds = mxe::fmpv_lds_doubles((int)d) * sizeof(double);
    if (lds > 160 * 1024) return MXE_ERR_LIMIT;
    // the scratch: one slice per workgroup, as for mxe_fullmatrix_posterior_var
    const size_t scr = mxe::fmld_scratch_doubles(m, cplx, n_omega, n_s);
    size_t n_slices = (size_t)MXE_FULLMATRIX_POSTVAR_SCRATCH_BYTES / (scr * sizeof(double));
    if (const char* e = getenv("MXE_FULLMATRIX_LOGDET_SLICES"))       // (tests: fewer slices than jobs)
        if (const long cap = atol(e); cap >= 1 && (size_t)cap < n_slices) n_slices = (size_t)cap;
    if (n_slices < 1) n_slices = 1;
    if (n_slices > nj) n_slices = nj;
    Stage sg;
    if (int rc = sg.open(device); rc != MXE_OK) return rc;
    mxe::FullMatrixLogdetParams p;
    std::memset(&p, 0, sizeof(p));
    p.n_job = n_job; p.n_omega = n_omega; p.n_s = n_s; p.want_ngood = want_ngood;
    Block in;
    const size_t oV = in.add(nw * ns), oc = in.add(ns), oD = in.add(nw), oa = in.add(nj), ou = in.add(nj * d);
    double* din;
    STGCHK(sg, sg.alloc(&din, in.total));
    STGCHK(sg, sg.upload(din + oV, V, nw * ns)); STGCHK(sg, sg.upload(din + oc, c, ns));
    STGCHK(sg, sg.upload(din + oD, D, nw)); STGCHK(sg, sg.upload(din + oa, alpha, nj));
    STGCHK(sg, sg.upload(din + ou, u, nj * d));
    p.V = din + oV; p.c = din + oc; p.D = din + oD; p.alpha = din + oa; p.u = din + ou;
    STGCHK(sg, sg.alloc(&p.scratch, n_slices * scr));
    const size_t ng = want_ngood ? nj : 0;
    Block out;
    const size_t ol = out.add(nj), on = out.add(ng);
    double* dout;
    STGCHK(sg, sg.alloc(&dout, out.total));
    p.out_logdet = dout + ol; p.out_ngood = dout + on;
    typedef void (*kernel_t)(const mxe::FullMatrixLogdetParams);
    static const kernel_t kernels[2][4] = {
        {mxe::fullmatrix_logdet_kernel<1, false>, mxe::fullmatrix_logdet_kernel<2, false>,
         mxe::fullmatrix_logdet_kernel<3, false>, mxe::fullmatrix_logdet_kernel<4, false>},
        {mxe::fullmatrix_logdet_kernel<1, true>, mxe::fullmatrix_logdet_kernel<2, true>,
         mxe::fullmatrix_logdet_kernel<3, true>, mxe::fullmatrix_logdet_kernel<4, true>}};
    STGCHK(sg, sg.time_begin(out_ms != nullptr));
    STGCHK(sg, launch_lds(kernels[cplx ? 1 : 0][m - 1], dim3((unsigned)n_slices), dim3(mxe::FM_T), lds, sg.stream, p));
    STGCHK(sg, sg.time_end());
    STGCHK(sg, sg.fetch(out_logdet, p.out_logdet, nj));
    STGCHK(sg, sg.fetch(out_ngood, p.out_ngood, ng));
    STGCHK(sg, sg.finish(out_ms));
    return MXE_OK;
}
MXE_CATCH_ALL
