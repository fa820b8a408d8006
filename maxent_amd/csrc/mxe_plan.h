// The launch plan of mxe_chains_upload: how the alpha scans of a batch are cut into cold-started pieces, which kernel, active
// block and layout run them, and in what order.  Plain C++17 on the host: no device call, no context, no environment, no
// I/O -- everything the decision reads is in PlanInput, everything it produces in LaunchPlan (tools/plan_dump.cpp runs it
// stand-alone).  plan_launch() runs the stages below in order; DESIGN.md section 4 lists them.
// At the end of the file, under the same rules: plan_finish(), the plan of mxe_chains_finish (FinishInput -> FinishPlan), and
// KernelBuild with its choosers: which instantiation of a chain kernel a launch runs (mxe_chains_launch, mxe_chains_finish).
// The LDS bytes of every build come from mxe_shapes.h.
#pragma once
#include "../../include/maxent_hip.h"
#include "mxe_shapes.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

namespace mxe {
constexpr double MC_COUPLING_MAX = 1e-3;     // relative coupling of the first direction the 32-row active block leaves out (choose_layout)
constexpr double MC_DEPTH_TARGET = 20.0;     // evaluations of one piece of a launch that is cut by cost (cost_cuts)
constexpr double MC_LADDER_COARSE = 2.0;     // a step between neighbouring alphas beyond this factor is not taken in one go (measured: up to a factor ~1.5 a warm step is safe, over a factor 2 single scans took 100-300 evaluations; 1.6 here cost stress case 51 -- ratio 1.66, sigma 1e-5 -- two converged flags and 3 x the time)
constexpr int MC_LADDER_MAX = 28;            // rungs per piece (the slot's alpha table holds 32 entries)
constexpr size_t LDS_CU = 160 * 1024;        // bytes of LDS of a CU
constexpr size_t LDS_MC1 = LDS_CU - 6144;    // dynamic LDS of a lock-step workgroup that has a CU to itself (the rest: the static arrays of chain_kernel_mc)
constexpr size_t LDS_MC2 = LDS_CU / 2 - 2048;      // ... of one that shares it with a second
constexpr double FIN_COARSE = 1.6;           // finishing pass: a step between neighbouring alphas beyond this factor, in either direction, is cut into rungs (plan_finish)
constexpr int FIN_RUNGS_MAX = 40;            // rungs of one such step (beyond: equal rungs of more than FinishEnv::ratio)

// the environment overrides of the plan (A/B runs and tests); read_plan_env() of maxent_hip.hip is the one place that reads them
struct PlanEnv {
    double taper = 1.0;                // MXE_TAPER: pieces of unequal length (>= 0.2; 1 = equal)
    double ladder_ratio = 1.56;        // MXE_LADDER_RATIO: ratio of the rungs (>= 1.05; just above MXE_X_WALK_RATIO: the walk lands on every rung)
    bool no_lds_basis = false, no_split_by_kind = false, no_ladder = false, no_na64 = false, no_sorted_static = false;
};
struct PlanInput {
    int n_chain = 0, n_alpha = 0, n_ds = 0, n_s = 0, NP = 64, n_omega_pad = 0, n_cu = 256;
    const int32_t* elem_of_chain = nullptr;      // [n_chain], every entry checked against the elements by the caller
    const double* alpha = nullptr;               // [n_chain][n_alpha], already divided by chi2_factor
    const int *elem_kind = nullptr, *elem_ds = nullptr;      // per element: MXE_ENTROPY_*, its data set,
    const double* elem_sumD = nullptr;                       //   the sum of its default model
    const int* ds_rows = nullptr;                // per data set: data points,
    const double* ds_c32 = nullptr;              //   the singular value c[32] (0 when n_s <= 32)
    mxe_opts opts;
    size_t lds_override[4] = {0, 0, 0, 0};       // tests only (plan_dump's `lds` key): bytes to take instead of the formulas of mxe_shapes.h for chain_kernel_lv with
                                                 //   its static arrays, chain_kernel_mc<32, 1>, <32, 2>, <64, 1>, so that "does not fit" is expressible; 0: the formula
    int wgpc_auto = 2, mc_wgpc_hint = 1;         // what the auto rule chose last: a launch with alpha_split > 0 keeps it
    PlanEnv env;
};
struct Piece {
    int elem, prob0, len, v0;      // element, first problem (scan * n_alpha + alpha index), alphas, scan (its start vector)
    int pre, walk0;                // led piece: entries it walks before its first alpha (0: none); its ladder starts at walk_alpha[walk0] (-1: it walks the scan's mesh)
};
struct LaunchPlan {
    std::vector<Piece> pieces;
    std::vector<double> walk_alpha;              // the ladders of the led pieces of a coarse mesh
    std::vector<int> excluded;                   // problems no piece covers (more than 32 coupled directions): mxe_chains_finish
    std::vector<int> queue, wg_chains;           // one data set: pieces by falling cost; several: four pieces per workgroup, -1 pads
    int layout = 1, mc_na = 0, mc_wgpc = 1, lv_mode = 0, wgpc_auto = 2, mc_wgpc_hint = 1, n_wg = 0, n_wg2 = 0, wgpc2 = 1;
    bool mc_gst = false, solo_rule = false;      // solo_rule: the launch is one the solo workgroups are for (mxe_schedule_info reports the probe then),
    int n_solo_wanted = 0;                       //   and how many it takes if the placement rule holds
    int precision = MXE_PRECISION_F64;           // after promotion
    size_t uncovered = 0, covered_twice = 0;     // check_coverage (both 0 unless plan_launch returns MXE_ERR_STATE)
};
namespace plan {
// what the stages hand on.  precision and f32_lv are STATE: a promotion is seen by every rule after it
struct State {
    int precision = MXE_PRECISION_F64, split = 0, split_pm = 0;       // split: pieces per scan; split_pm: per plus-minus scan where that differs (0: the same)
    bool lv_fits = false, f32_lv = false, ladder_ok = false;
    bool fits32 = true;                // no alpha of the job couples more than 32 directions (choose_precision)
    bool cut_by_cost = false;          // launches that do not fill the GPU: pieces of equal COST, one per slot (decided once for the launch)
};
inline bool normal_elem(const PlanInput& in, int e) { return in.elem_kind[e] == MXE_ENTROPY_NORMAL; }
// (what every lock-step build needs of the options)
inline bool lockstep_opts(const PlanInput& in) { return in.NP == 64 && in.opts.chains_per_wg != 1 && in.opts.tol_d <= 0.0 && in.opts.decouple_tol > 0.0; }
// dynamic LDS of the candidate builds at the mesh of the input: chain_kernel_lv with its static arrays, chain_kernel_mc<NA, wgpc> at four waves
inline size_t lds_lv(const PlanInput& in) { return in.lds_override[0] ? in.lds_override[0] : lv_lds_bytes(in.n_s, in.n_omega_pad) + LV_STATIC_LDS; }
inline size_t lds_mc(const PlanInput& in, int NA, int wgpc)
{
    const size_t over = in.lds_override[NA == 64 ? 3 : wgpc == 2 ? 2 : 1];
    return over ? over : mc_lds_bytes(NA, in.n_omega_pad, wgpc);
}
inline double piece_amin(const PlanInput& in, const Piece& p) { return *std::min_element(in.alpha + p.prob0, in.alpha + p.prob0 + p.len); }
// alpha x the relative coupling of the first direction a 32-row active block leaves out, for element e: c_32^2 wmax, wmax <= max(1, sum D)
inline double coupling32(const PlanInput& in, int e) { const double c = in.ds_c32[in.elem_ds[e]]; return c * c * std::max(1.0, in.elem_sumD[e]); }

// ---- stage 1: the arithmetic.  chain_kernel_lv (V^T resident in LDS as binary32) is possible where the basis fits beside the
// state of four slots; binary32 launches in that kernel are scheduled like binary64 ones: lock-step pieces, one workgroup per CU
inline void choose_precision(const PlanInput& in, State& st)
{
    const mxe_opts& o = in.opts;
    st.precision = o.precision;
    const bool lds_basis_ok = o.lds_basis != 2 && !in.env.no_lds_basis && lockstep_opts(in);
    st.lv_fits = in.n_omega_pad <= 512 && lds_basis_ok && lds_lv(in) <= LDS_CU;
    st.f32_lv = st.precision == MXE_PRECISION_F32 && st.lv_fits;
    // (the criterion of choose_layout, per scan: no alpha of the job couples more than 32 directions)
    for (int c = 0; c < in.n_chain && st.fits32 && in.n_s > 32; ++c) {
        const double* ac = in.alpha + (size_t)c * in.n_alpha;
        const double amin = *std::min_element(ac, ac + in.n_alpha);
        if (!(coupling32(in, in.elem_of_chain[c]) / amin <= MC_COUPLING_MAX)) st.fits32 = false;
    }
    if (st.f32_lv && in.n_s > 32) {
        // (chain_kernel_lv has the plain 32-row build only: a job with an alpha that couples more than 32 directions keeps the
        //  one-chain binary32 kernel AND its pieces of six alphas)
        st.f32_lv = st.fits32;
        // Binary32 is asked for as the cheaper arithmetic; for such a job the cheaper arithmetic is the binary64 lock-step
        // build with the 64-row block (and the hand-over of what it leaves): the one-chain binary32 kernel took 0.7-1.5 s
        // where that takes 4-5 ms, and stops at its rounding floor besides (STRESS_F32=1 tools/stress.py, cases 24 / 25:
        // profiles/r04_e_stress_f32.txt).  The launch is promoted; mxe_last_launch_info names the kernel that ran.
        if (!st.f32_lv) st.precision = MXE_PRECISION_F64;
    }
    // A frequency mesh whose basis does not fit the LDS as binary32 (n_omega > 512, or n_s x (n_omega_pad + 4) floats beyond what
    // the slots leave): the binary32 request would run one chain per workgroup with V streamed from the L2 by every chain --
    // 3.6-7.8 ms where the binary64 lock-step kernel takes 0.5-1.7 (8 x 8 and 16 x 16 elements x 100 alpha at n_omega = 640 ...
    // 1500), and stops at its rounding floor besides (audit 8e-4 against 1e-8).  Binary32 is asked for as the cheaper
    // arithmetic: the launch is promoted like the case above.  lds_basis = 2 or chains_per_wg = 1 keep the one-chain
    // binary32 kernel (BASELINE config 5's tolerance sweep on such a mesh asks for it that way).
    if (st.precision == MXE_PRECISION_F32 && !st.lv_fits && lds_basis_ok) st.precision = MXE_PRECISION_F64;
    st.ladder_ok = !in.env.no_ladder && lockstep_opts(in) && (st.precision == MXE_PRECISION_F64 || st.f32_lv);
}
// the logarithmic range of a scan, where its guarded tail begins (the last 6 % of it) and the smallest alpha at or above that:
// what leads the tail pieces (-1: none)
struct ScanRange { double lmax = -1e300, lmin = 1e300, lguard = 0.0; int lead = -1; };
inline ScanRange scan_range(const double* ac, int n_alpha)
{
    ScanRange r;
    for (int i = 0; i < n_alpha; ++i) { const double l = std::log(ac[i]); r.lmax = std::max(r.lmax, l); r.lmin = std::min(r.lmin, l); }
    r.lguard = r.lmax - 0.94 * (r.lmax - r.lmin);
    double best = 1e300;
    for (int i = 0; i < n_alpha; ++i) if (std::log(ac[i]) >= r.lguard && ac[i] < best) { best = ac[i]; r.lead = i; }
    return r;
}
// ---- stage 3a: cuts of one normal-entropy scan of a launch that does not fill the GPU (piece starts, + n_alpha).
// Such a launch is as long as its deepest slot, so the pieces are cut to equal COST and every slot gets one.  The cost of a
// normal-entropy piece is its cold start -- 9-10 evaluations in the upper third of the logarithmic alpha range, rising to 17-19
// just above the guarded tail (profiles/r04_b_depth_by_piece.txt; the same numbers as the cold-start profile of r02) -- plus ~3
// per further alpha: with the uniform pieces of two alphas the deepest slot of the 8-GPU shards was a piece at alpha index 88-92
// (19 + 5 evaluations), not the led tail pieces (~22 rounds with their walk).  Pieces of a normal-entropy scan therefore get as
// many alphas as fit MC_DEPTH_TARGET evaluations (4 at the top of the mesh, 1 next to the tail) and end where the guarded range
// begins; the plus-minus scans (cold start ~4.5, ~2.2 per alpha) share the slots the normal-entropy pieces leave.
// (the same cut for the normal-entropy scans of the batch that FILLS the GPU -- targets of 34 / 38 / 42 evaluations instead of 15
//  uniform pieces -- was 10-13 % slower, 0.814 -> 0.894 / 0.893 / 0.917 ms: there the queue balances, profiles/r04_experiments.txt)
inline void cost_cuts(const double* ac, int n_alpha, std::vector<int>& cuts)
{
    const ScanRange r = scan_range(ac, n_alpha);
    auto in_tail = [&](int i) { return r.lmax > r.lmin && std::log(ac[i]) < r.lguard && r.lead >= 0 && r.lead < i; };
    cuts.clear();
    for (int a0 = 0; a0 < n_alpha;) {
        cuts.push_back(a0);
        if (in_tail(a0)) break;     // (the guarded tail: one range, cut into led single alphas by emit_scan)
        const double xpos = (r.lmax > r.lmin) ? (r.lmax - std::log(ac[a0])) / (r.lmax - r.lmin) : 0.0;
        const double cold = 9.5 + 13.0 * std::max(0.0, xpos - 0.3);
        const int L = 1 + (int)std::floor(std::max(0.0, (MC_DEPTH_TARGET - cold) / 3.0));
        int a1 = std::min(n_alpha, a0 + std::max(1, std::min(L, 6)));
        for (int j = a0 + 1; j < a1; ++j) if (in_tail(j)) { a1 = j; break; }
        a0 = a1;
    }
    cuts.push_back(n_alpha);
}
// ---- stage 3b: plus-minus scans of such a launch: cold start ~4.5 evaluations, then 2 per alpha at the top of the mesh and 3 at
// its bottom -- with uniform pieces of seven alphas the deepest slot of the four-GPU shards was a plus-minus piece at the
// smallest alphas (4.6 + 7 x 3.0 = 26 rounds).  At most `pieces` pieces of equal cost: the smallest cost per piece that needs no
// more (bisection)
inline void pm_cuts(const double* ac, int n_alpha, int pieces, std::vector<int>& cuts)
{
    const ScanRange r = scan_range(ac, n_alpha);
    auto w = [&](int a) { return 2.0 + ((r.lmax > r.lmin) ? (r.lmax - std::log(ac[a])) / (r.lmax - r.lmin) : 0.0); };
    auto cut = [&](double T, std::vector<int>* out) {
        int n = 0, a0 = 0;
        while (a0 < n_alpha) {
            if (out) out->push_back(a0);
            double cost = 4.5 + w(a0);
            int a1 = a0 + 1;
            while (a1 < n_alpha && cost + w(a1) <= T) { cost += w(a1); ++a1; }
            a0 = a1; ++n;
        }
        return n;
    };
    double lo = 6.0, hi = 4.5 + 3.0 * n_alpha + 1.0;
    for (int it = 0; it < 40 && hi - lo > 0.05; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (cut(mid, nullptr) <= pieces) hi = mid; else lo = mid;
    }
    cuts.clear(); cut(hi, &cuts); cuts.push_back(n_alpha);
}
// ---- stage 2: pieces per scan.  An alpha scan may be cut into pieces that are cold-started from the same v0 (the minimiser of
// each alpha does not depend on the path)
inline void pieces_per_scan(const PlanInput& in, State& st, LaunchPlan& lp)
{
    const mxe_opts& o = in.opts;
    const int n_chain = in.n_chain, n_alpha = in.n_alpha, n_cu = in.n_cu;
    st.split = o.alpha_split;
    lp.wgpc_auto = in.wgpc_auto; lp.mc_wgpc_hint = in.mc_wgpc_hint;
    if (st.split <= 0) {
        // about two pieces per chain slot of the GPU (CUs x workgroups per CU x 4 slots): the persistent grid then balances (pieces have
        // unequal costs and are handed out most expensive first), and a batch that is small for the GPU -- one rank's shard of a job that is
        // spread over several -- is cut into many short cold-started pieces rather than left on a fraction of the CUs.  None shorter than two
        // alphas (a cold start costs 4-10 iterations, a warm alpha 2-3).  Measured, kernel time of 256 / 128 / 64 / 32 scans of 100 alphas
        // (profiles/r02_d_shard_sweep.txt): 16 pieces per scan 1.28 / 1.09 / 0.93 / 1.54 ms, 34: 2.95 / 0.84 / 0.73 / 0.62, 50: 3.27 / 0.87 /
        // 0.67 / 0.57.  A piece of a normal-entropy scan costs about twice one of a plus-minus scan of the same length (10-18 against 5
        // evaluations for the cold start, 3 against 2 per alpha): it counts twice, so that a slot gets two plus-minus pieces or one normal
        // piece, not three (cfg4: 15 pieces per scan instead of 16 -- of 4096 pieces 14 % of the slots took a third --, 1.228 -> 1.171 ms; 14: 1.34 ms)
        long long scans = 0; for (int c = 0; c < n_chain; ++c) scans += normal_elem(in, in.elem_of_chain[c]) ? 2 : 1;
        if (st.f32_lv && o.wg_per_cu == 0 && in.n_omega_pad <= 512) {
            // A binary32 launch runs in chain_kernel_lv at ONE workgroup per CU.  A batch that fills the GPU at two per CU (the test
            // of the loop below) is faster in the binary64 kernel that runs that way: the 25 600-problem batch 0.81 ms against
            // 1.24 ms -- binary32 is asked for as the cheaper arithmetic, and there it is not.  Such a launch is promoted like the
            // one that couples more than 32 directions; wg_per_cu = 1 keeps it in chain_kernel_lv.
            const int want2 = (int)std::max(1LL, (2LL * 8 * n_cu) / std::max(1LL, scans));
            if (std::max(1, std::min(want2, n_alpha / 2)) >= want2) { st.f32_lv = false; st.precision = MXE_PRECISION_F64; }
        }
        // (two workgroups per CU where the lock-step kernel has a build for it: n_omega_pad <= 512)
        int wgpc = (o.wg_per_cu != 1 && in.n_omega_pad <= 512 && in.NP == 64 && o.chains_per_wg != 1 && !st.f32_lv) ? 2 : 1;
        // (mxe_opts.in_flight = n: the caller keeps n such batches in flight -- each fills 1 / n of the slots, with 1 / n of the cold starts:
        //  25 600 alpha-solves in 4 x 256 pieces of 25 alphas cost 0.65 ms side by side with three other batches, in 15 x 256 pieces 0.83 ms
        //  alone and 0.74 ms next to one other; profiles/r04_experiments.txt 10.)
        const long long nfl = std::max(1, o.in_flight), weight = scans * nfl;
        for (;;) {
            const int n_slots = 4 * wgpc * n_cu;
            // (rounded UP when batches share the GPU: 4 pieces per scan x 4 batches 0.647 ms per batch, 3 x 4: 0.690)
            const int want = (int)std::max(1LL, (2LL * n_slots + (nfl > 1 ? std::max(1LL, weight) - 1 : 0)) / std::max(1LL, weight));
            st.split = std::max(1, std::min(want, n_alpha / 2));
            // The loss rule.  A batch with more scans than that rule has pieces for (two pieces per slot would be fewer than six per scan:
            // 32 x 32 elements and beyond) was left with one to four long pieces per scan, 1.1-2.3 per slot -- and a slot that takes one
            // piece more than its neighbours then runs half a launch longer: 48 x 48 x 100 alphas 9.6 ms, 23 M alpha-solves/s, where six
            // pieces per scan take 5.6 ms, 40.8 M (tools/batch_size_sweep.sh, profiles/r05_experiments.txt 11.).  There the count
            // is chosen by what it costs: the cold start of a piece, 4 evaluations against 2 per alpha of its length, and the
            // imbalance of a queue of pieces of one size, half a piece per slot.  (Batches in flight fill each other's gaps: fewest
            // pieces, as above.)
            if (nfl == 1 && want < 6 && n_alpha >= 16) {
                double best = 1e300;
                for (int sp = std::max(1, want); sp <= std::min(16, n_alpha / 4); ++sp) {
                    const double len = (double)n_alpha / sp, per_slot = (double)sp * (double)weight / n_slots;
                    const double loss = 4.0 / (4.0 + 2.0 * len) + 0.5 / per_slot;
                    if (loss < best) { best = loss; st.split = sp; }
                }
            }
            // (the binary32 streaming variant stops an alpha at its rounding floor, which a cold start reaches
            //  from further away: it keeps pieces of at least six alphas, at most 16 per scan)
            if (st.precision == MXE_PRECISION_F32 && !st.f32_lv) st.split = std::max(1, std::min(std::min(want, 16), n_alpha / 6));
            // two workgroups per CU pay when there is work for two rounds of them; a batch that cannot be cut into that many pieces runs
            // at one per CU, where a round of a workgroup takes 45 k instead of 73 k cycles (the 3 200-problem shard of cfg4 / 8: 0.48 against 0.59 ms)
            if (wgpc == 2 && o.wg_per_cu == 0 && st.split < want) { wgpc = 1; continue; }
            break;
        }
        lp.wgpc_auto = lp.mc_wgpc_hint = wgpc;
        // A launch that does not fill the GPU (one workgroup per CU: pieces at the cap of two alphas) is as long as its deepest slot,
        // and a slot that takes a second piece pays a second cold start.  Where the uniform cut gives more pieces than slots, the
        // plus-minus scans -- cold start 5 rounds against 12-16, 2 rounds per alpha against 2.75: a piece of twice the alphas costs
        // what a normal-entropy piece does -- are cut into fewer, longer pieces, so that every slot gets ONE piece (the 3 200-problem
        // shard of cfg4 / 8: 1 600 pieces on 1 024 slots -> 1 012; profiles/r04_experiments.txt).  MXE_NO_SPLIT_BY_KIND: the old cut
        // (one workgroup per CU only.  At two per CU -- the two-GPU shard of cfg4, whose plus-minus pieces would stay short enough --
        //  the cut by cost LOST: 0.565 -> 0.617 ms; two workgroups per CU are the throughput regime, profiles/r04_experiments.txt)
        st.cut_by_cost = wgpc == 1 && o.wg_per_cu == 0 && !in.env.no_split_by_kind && n_alpha >= 4;
        // a small batch that cannot fill the lock-step layout (>= 768 pieces) with pieces of six alphas, but can with shorter ones, takes
        // those: the lock-step kernel serves four pieces with the loads and the time the one-chain kernel spends on one (cfg3, 16 scans:
        // 1.9 ms with 256 pieces in the one-chain layout, 0.7 ms with 768 pieces of two alphas in the lock-step layout)
        if ((long long)n_chain * st.split < 768 && n_alpha >= 4 && (long long)n_chain * (n_alpha / 2) >= 768 &&
            lockstep_opts(in) && (st.precision == MXE_PRECISION_F64 || st.f32_lv))
            st.split = (768 + n_chain - 1) / n_chain;
    }
    if (st.split > n_alpha) st.split = n_alpha;
    if (st.cut_by_cost) {
        long long n_normal = 0, pieces_normal = 0, slots = 4LL * n_cu;      // (one workgroup per CU)
        std::vector<int> cuts;
        for (int c = 0; c < n_chain; ++c)
            if (normal_elem(in, in.elem_of_chain[c])) {
                ++n_normal;
                cost_cuts(in.alpha + (size_t)c * n_alpha, n_alpha, cuts);
                pieces_normal += (long long)cuts.size() - 2 + (n_alpha - cuts[cuts.size() - 2]);      // (the last range: one piece per alpha if it is the guarded tail -- an upper bound otherwise)
            }
        const long long n_pm = n_chain - n_normal;
        // (one workgroup per CU is not always a launch that does not fill the GPU -- a binary32 launch runs that way whatever its
        //  size --: the cut is only taken when the plus-minus pieces it leaves are short.  A plus-minus piece of eight or nine
        //  alphas costs ~4.5 + 8 x 2.5 = 24 evaluations: the depth of the led tail pieces.  The four-GPU shard of cfg4 -- 14 pieces
        //  per scan -- stays that short, cfg4 itself does not.  Without that test the 25 600-problem batch in binary32 got ONE piece
        //  per plus-minus scan: 1.24 -> 3.18 ms)
        const long long min_pm = (n_alpha + 8) / 9;       // (at most nine alphas per plus-minus piece)
        if (pieces_normal + n_pm * min_pm <= slots) {
            if (n_pm > 0) st.split_pm = (int)std::max(1LL, std::min<long long>(n_alpha / 2, (slots - pieces_normal) / n_pm));
        } else st.cut_by_cost = false;                  // (more scans than slots can take one piece of each: the uniform cut)
    }
}
// ---- stage 3: cuts of scan c (piece starts, + n_alpha): by cost where the launch is cut that way, else uniform or tapered
inline void scan_cuts(const PlanInput& in, const State& st, int c, std::vector<int>& cuts)
{
    const int n_alpha = in.n_alpha;
    const double* ac = in.alpha + (size_t)c * n_alpha;
    const bool normal_c = normal_elem(in, in.elem_of_chain[c]);
    cuts.clear();
    if (st.cut_by_cost && normal_c && st.split > 1) return cost_cuts(ac, n_alpha, cuts);
    if (st.cut_by_cost && !normal_c && st.split_pm > 1 && st.split_pm < n_alpha / 2) return pm_cuts(ac, n_alpha, st.split_pm, cuts);      // (at the cap of two alphas there is nothing to balance)
    const int split_c = (st.split_pm > 0 && !normal_c) ? std::min(st.split_pm, n_alpha) : st.split;
    // (taper: the pieces of a scan grow from its first alpha to its last -- piece i of n has 1 + (taper - 1) i / (n - 1) parts --
    //  so that what the queue hands out LAST, the cheap short pieces at the top of the mesh, evens the workgroups out;
    //  1 = pieces of equal length)
    const double taper = in.env.taper;
    if (taper != 1.0 && split_c > 1) {
        std::vector<double> wsum(split_c + 1, 0.0);
        for (int i = 0; i < split_c; ++i) wsum[i + 1] = wsum[i] + 1.0 + (taper - 1.0) * i / (split_c - 1);
        for (int sidx = 0; sidx <= split_c; ++sidx) {
            int a = std::max((int)std::llround(n_alpha * wsum[sidx] / wsum[split_c]), sidx == 0 ? 0 : cuts.back() + 1);          // (no empty piece)
            a = sidx == split_c ? n_alpha : std::min(a, n_alpha - (split_c - sidx));
            if (cuts.empty() || a > cuts.back()) cuts.push_back(a);
        }
    } else
        for (int sidx = 0; sidx <= split_c; ++sidx) {
            const int a = (int)((long long)n_alpha * sidx / split_c);
            if (cuts.empty() || a > cuts.back()) cuts.push_back(a);
        }
}
// ---- stage 4: the pieces of scan c between its cuts.
// Normal entropy: from the default model the smallest alphas of a scan are far away.  Measured on the BASELINE
// batch (profiles/r02_f_cold_start_profile.txt), a cold start in the last 6 % of the logarithmic alpha range takes
// 20-30 evaluations on average and 50-390 for single scans (above that range: 10-18, at most 21) -- and a launch
// ends with its slowest piece.  A piece that starts there is led by the last alpha ABOVE the range: cold start
// where it is cheap and safe, then one warm step down to the piece's first alpha (lock-step kernel: chain_pre);
// in the other layouts, and where that step would be long, the piece is joined to the one before it (choose_layout).
inline void emit_scan(const PlanInput& in, const State& st, int c, const std::vector<int>& cuts, LaunchPlan& lp)
{
    const int n_alpha = in.n_alpha, e = in.elem_of_chain[c];
    const double* ac = in.alpha + (size_t)c * n_alpha;
    const double ladder_ratio = in.env.ladder_ratio;
    const double hard_below = 0.25 * in.ds_rows[in.elem_ds[e]];      // alpha~ below N_data / 4
    double pre_alpha = 0.0, lguard = 0.0;
    int pre_index = -1;                              // the smallest alpha of the scan that is still above the guarded range
    if (normal_elem(in, e) && st.split > 1) {
        const ScanRange r = scan_range(ac, n_alpha);
        lguard = r.lguard; pre_index = r.lead;
        if (r.lmax > r.lmin && r.lead >= 0) pre_alpha = ac[r.lead];
    }
    auto emit = [&](int first, int len, int pre, int walk0) { lp.pieces.push_back(Piece{e, c * n_alpha + first, len, c, pre, walk0}); };
    // A mesh too coarse to walk on (round 5).  The warm step into an alpha is safe over a factor ~1.5 in alpha; the reference's
    // own tests and defaults use 3-20 alphas over 4-6 decades (alpha_meshes.py:81, test/python/tau_maxent.py:44), and
    // where the entropy term no longer holds the solution (alpha~ below about N_data / 4) a step over a factor 2 ... 600 took
    // 250-2 300 evaluations (profiles/r05_b_coarse_mesh.txt: smoke()'s last alpha 913 of the launch's 308 rounds).  Such an
    // alpha is a piece of its own that starts cold where that is cheap -- at max(N_data / 4, its own alpha) -- and walks down a
    // LADDER of alphas of its own (ratio ladder_ratio, a few loose rounds per rung, no records) to its alpha: all hard
    // alphas of a scan side by side, each as deep as one cold start + one walk.
    auto hard = [&](int i) {
        if (!st.ladder_ok || i < 0 || i >= n_alpha) return false;
        if (!(ac[i] < hard_below) || i == 0) return false;                  // (the head of a scan starts from the default model as ever)
        const double r = ac[i - 1] / ac[i];
        return r > MC_LADDER_COARSE || r < 1.0 / MC_LADDER_COARSE;
    };
    // (chain_kernel_lv keeps LV_ACAP alphas per slot, and a piece that does not fit that table reads every entry from the scan's
    //  mesh: right for a piece the mesh leads, wrong for rungs.  Until this rule such a launch got the ladders of chain_kernel_mc
    //  -- four alphas from alpha~ = 1e2 down to 1e-4 on 100 data points: 18 and 23 rungs + 1 alpha -- and walked the mesh BEFORE
    //  the piece instead, for the first scan from in front of the alpha array.  The second line is what order_pieces asks of a
    //  two-pass launch, short of a state in device memory, which no mesh that fits this kernel needs.)
    const bool lv_table = st.f32_lv ||
                          (st.lv_fits && st.precision == MXE_PRECISION_F64 && in.opts.lds_basis == 1 && st.fits32);
    auto emit_ladder = [&](int i, int len = 1) {
        const double a = ac[i];
        const double top = std::max(hard_below, a * ladder_ratio);
        int rungs = (int)std::ceil(std::log(top / a) / std::log(ladder_ratio) - 1e-9);
        rungs = std::max(1, std::min(rungs, lv_table ? LV_ACAP - len : std::min(MC_LADDER_MAX, 30 - len)));      // (rungs + alphas of the piece: the slot's table of 32, of LV_ACAP in chain_kernel_lv)
        const double ratio = std::pow(top / a, 1.0 / rungs);          // (equal rungs; more than that would not fit the slot's table)
        const int w0 = (int)lp.walk_alpha.size();
        for (int k = 0; k < rungs; ++k) lp.walk_alpha.push_back(a * std::pow(ratio, rungs - k));
        emit(i, len, rungs, w0);
    };
    // A piece whose FIRST alpha is its hardest: the head of a scan that begins deep in the hard region, and every piece of an
    // ASCENDING scan there (each starts from the default model at its smallest alpha: on 150 alphas rising from alpha~ = 0.5 at
    // sigma = 4e-5 the head took 2 989 evaluations and did not converge, tools/stress.py case 17).  It is led down a ladder from
    // N_data / 4 to its first alpha and goes on up its own mesh from there.
    auto emit_plain = [&](int first, int len) {
        const bool deep = st.ladder_ok && len <= (lv_table ? LV_ACAP : 32) - 8 && ac[first] * (ladder_ratio * ladder_ratio) < hard_below &&
                          (first == 0 || ac[first - 1] < ac[first]);
        if (deep) emit_ladder(first, len); else emit(first, len, 0, -1);
    };
    for (size_t sidx = 0; sidx + 1 < cuts.size(); ++sidx) {
        const int a0 = cuts[sidx], a1 = cuts[sidx + 1];
        if (a1 <= a0) continue;
        const bool guarded = pre_alpha > 0.0 && sidx > 0 && std::log(ac[a0]) < lguard && pre_index < a0;
        // (lock-step kernel: the piece WALKS from the leading alpha down the mesh to its first alpha with a loose tolerance -- every step as
        //  safe as the scan itself --, so every piece of the tail stands alone and the tail of a scan is as many short chains side by side as
        //  it has pieces.  A jump over more than a factor 1.5 in alpha -- measured: at most 11 evaluations up to that; single scans took
        //  100-300 over a factor 2 -- was what joined pieces until r02_k)
        // (a led piece is cut into single alphas: each walks down from the leading alpha on its own, and the tail of the scan -- the longest
        //  chain of every launch that does not fill the GPU -- is as deep as ONE walk)
        // (a piece that starts above the range and runs into it stays whole: cutting it where it enters cost the batch that fills the GPU
        //  6 % -- cfg4 on one GPU 0.947 -> 1.01 ms)
        const int g0 = guarded ? a0 : a1;
        // the part of the piece that is not led: cut at every hard alpha
        int b = a0;
        for (int i = a0; i < g0; ++i)
            if (hard(i)) {
                if (i > b) emit_plain(b, i - b);
                emit_ladder(i);
                b = i + 1;
            }
        if (g0 > b) emit_plain(b, g0 - b);
        for (int b0 = g0; b0 < a1; ++b0) { if (hard(b0)) emit_ladder(b0); else emit(b0, 1, b0 - pre_index, -1); }
    }
}
// the one place pieces are dropped: keep(piece, the piece kept last or nullptr) may shorten the piece or grow that one
template <class F> void filter_pieces(std::vector<Piece>& ps, F keep)
{
    size_t w = 0;
    for (size_t sc = 0; sc < ps.size(); ++sc) { Piece p = ps[sc]; if (keep(p, w ? &ps[w - 1] : nullptr)) ps[w++] = p; }
    ps.resize(w);
}
// ---- stage 5: layout and active block: four chains of one data set per workgroup wherever the lock-step kernel has a build for
// the problem -- also for a handful of pieces: its round (four chains) takes no longer than an iteration of the
// one-chain kernel (one), and a single scan of 100 alphas in 50 pieces runs in 0.45 ms against 0.94 ms
// (profiles/r02_k_small_batches.txt; until r02_j: only from 768 pieces on)
inline int choose_layout(const PlanInput& in, State& st, LaunchPlan& lp)
{
    const mxe_opts& o = in.opts;
    const size_t P = (size_t)in.n_chain * in.n_alpha;
    int layout = o.chains_per_wg == 0 ? 4 : o.chains_per_wg;
    if (layout == 4 && (in.NP != 64 || o.tol_d > 0.0 || o.decouple_tol <= 0.0 || (st.precision != MXE_PRECISION_F64 && !st.f32_lv))) layout = 1;
    if (layout == 4) {
        // capacity of the active block: the kernel clamps n_act to NA, and the
        // first neglected direction couples with relative strength
        // c_NA^2 wmax / alpha (wmax <= sum w ~ max(1, sum D)); accept NA when that
        // is below MC_COUPLING_MAX for every chain (inexact Newton: the contraction is that number, and the stopping
        // estimate of the kernel does not know about it -- an alpha stops when (e^{|du|} - 1 + theta) relH < tol_h, so its
        // last correction relH may be as large as tol_h / theta = 1e-4 and what the neglected direction leaves behind is
        // coupling x relH.  With 1e-2, the value until r03, converged alphas of launches AT that limit were 1.1e-6 ... 1.6e-6
        // from their fixed points (profiles/r03_i_small_sigma.txt); 1e-3 keeps a factor ten to the 1e-6 of the audit).
        // (an active block of 48 in the lock-step kernel spilled registers in every tiling that was tried: problems
        //  that couple more than 32 directions run in the one-chain layout, whose solve lives in LDS)
        double worst32 = 0.0;
        if (in.n_s > 32) for (const Piece& p : lp.pieces) worst32 = std::max(worst32, coupling32(in, p.elem) / piece_amin(in, p));
        if (worst32 <= MC_COUPLING_MAX) lp.mc_na = 32;
        else if (st.f32_lv) layout = 1;      // (chain_kernel_lv has the plain 32-row build only: the one-chain binary32 kernel, BEFORE any piece is cut or dropped below)
        else {
            // Some alphas couple more than 32 directions (very small error bars: sigma = 1e-6 on the BASELINE grids does at
            // the 27 smallest of 100 alphas).  Until r03 the whole launch then went to the one-chain layout (7 x slower).
            // (a) Plus-minus scans: the build with a 64-row active block -- ten Gram tiles per slot (80 KB of the LDS: one
            // workgroup per CU, n_omega_pad <= 512) and the one-row-per-lane elimination (gj1_solve_rows_f32).  240
            // off-diagonal scans x 100 alphas at sigma = 4e-6 ... 5e-7: 2.2 / 3.5 / 3.8 / 4.4 ms, nothing left over, audit
            // 5e-10 (one-chain layout: 12.8 ms).  (b) Normal-entropy scans: their systems at those alphas are ill conditioned
            // beyond what the binary16 Gram products of either lock-step build resolve (the iteration crawls to its limit
            // where the one-chain kernel, binary64 throughout, takes 3-28 steps): their pieces are cut where the criterion
            // fails -- coupling grows as alpha falls, so that is the tail of a scan -- and the alphas behind the cut are left
            // open for mxe_chains_finish: one warm chain per scan from the last alpha before the cut (records of such alphas
            // are NaN / not converged / 0 iterations until then: clear_excluded_kernel).  Without the 64-row build (a larger
            // frequency mesh) the plus-minus scans are cut as well.  Measured on the BASELINE batch (16 diagonal + 240
            // off-diagonal scans) with sigma = 4e-6 / 2e-6 / 1e-6 (maxiter 100): 15.4 / 17.1 / 146 ms in the one-chain
            // layout, 8-12 / 11-16 / 55-63 ms in every variant of this -- the serial depth of the 16 finishing chains (13-30
            // alphas x 3-28 iterations x 150-190 us in the one-chain kernel with 64 coupled directions) is the floor.
            // Leaving the cut alphas to the lock-step kernel's own give-up costs accuracy in the 32-row build (exact Newton
            // correction up to 9e-7, p99 1e-7, against 4e-8 / 2e-9) and time in the 64-row build (pieces of 10 alphas x 32
            // iterations: launch 8-9 ms).  Not when more than a third of the alphas would be left to the finishing pass
            // (sigma = 5e-7 without the 64-row build: 197 against 150 ms).  profiles/r03_c_cut_pieces.txt, r03_e_na64.txt
            const bool have64 = !in.env.no_na64 && in.n_s > 32 && o.wg_per_cu != 2 && lds_mc(in, 64, 1) <= LDS_MC1;
            bool need64 = false;
            std::vector<char> bad(P, 0); size_t n_bad = 0;
            for (int c = 0; c < in.n_chain; ++c) {
                const int e = in.elem_of_chain[c];
                const double lim = MC_COUPLING_MAX / coupling32(in, e);    // alpha >= 1 / lim passes
                const bool to64 = have64 && !normal_elem(in, e);
                for (int i = 0; i < in.n_alpha; ++i)
                    if (!(in.alpha[(size_t)c * in.n_alpha + i] * lim >= 1.0)) {
                        if (to64) need64 = true;
                        else { bad[(size_t)c * in.n_alpha + i] = 1; ++n_bad; }
                    }
            }
            // (a led piece starts from an alpha above its own: larger, so it passes when the piece's does)
            if (3 * n_bad > P || std::all_of(lp.pieces.begin(), lp.pieces.end(), [&](const Piece& p) { return bad[p.prob0] != 0; })) layout = 1;
            else {
                lp.mc_na = need64 ? 64 : 32;
                filter_pieces(lp.pieces, [&](Piece& p, Piece*) {      // (the pieces come in the order of the problems: so does what they leave)
                    int len = 0;
                    while (len < p.len && !bad[(size_t)p.prob0 + len]) ++len;
                    for (int i = len; i < p.len; ++i) lp.excluded.push_back(p.prob0 + i);
                    p.len = len; return len > 0;
                });
            }
        }
    }
    if (layout == 4) {
        lp.mc_wgpc = (o.wg_per_cu != 1 && (o.wg_per_cu == 2 || lp.wgpc_auto == 2) && lp.mc_na == 32 && in.n_omega_pad <= 512 &&
                      lds_mc(in, 32, 2) <= LDS_MC2) ? 2 : 1;
        if (lds_mc(in, lp.mc_na, lp.mc_wgpc) > LDS_MC1) {
            // a frequency mesh whose state (u, H, sw of four slots: 80 B per omega) does not fit the LDS beside the
            // rest: the state goes to device memory (chain_kernel_mc<.., GSTATE>, one workgroup per CU)
            lp.mc_wgpc = 1; lp.mc_gst = true;
        }
        if (st.f32_lv) {
            // the binary32 launch: only the plain 32-row layout with nothing cut has a build in chain_kernel_lv
            // (anything else was sent to the one-chain layout above, before the pieces were touched: r04's first form of this fell back
            //  HERE, after pieces of a 64-row launch had been cut -- the alphas behind the cuts were never solved, their records garbage:
            //  STRESS_F32=1 tools/stress.py, cases 24 / 25 / 42)
            if (lp.mc_na == 32 && lp.excluded.empty() && !lp.mc_gst) { lp.lv_mode = 1; lp.mc_wgpc = 1; }
            else return MXE_ERR_STATE;
        }
    } else {
        // the other layouts have no walk: a led piece is joined to the piece before it, and nothing is left to the finishing pass
        filter_pieces(lp.pieces, [](Piece& p, Piece* last) {
            if (p.pre > 0 && last && last->v0 == p.v0) { last->len += p.len; return false; }
            p.pre = 0; p.walk0 = -1; return true;
        });
        lp.walk_alpha.clear(); lp.excluded.clear();
    }
    lp.layout = layout;
    return MXE_OK;
}
// ---- stage 6: what a piece costs, a priori: normal entropy and small alpha cost more iterations
inline double piece_cost(const PlanInput& in, const Piece& p)
{
    const bool normal = normal_elem(in, p.elem);
    return p.len * (normal ? 4.0 : 3.0) + (normal ? 16.0 : 6.0) - 1e-3 * std::log10(piece_amin(in, p)) +
           (p.walk0 >= 0 ? 2.0 : 0.7) * p.pre;     // (the walk of a led piece: on the scan's mesh a landing every ~third alpha, MXE_X_WALK_RATIO; on a ladder every rung)
}
// ---- stage 7: the order of the pieces, the grid, and the two-pass mode
inline void order_pieces(const PlanInput& in, const State& st, LaunchPlan& lp)
{
    const mxe_opts& o = in.opts;
    const int n_sub = (int)lp.pieces.size(), n_cu = in.n_cu, n_alpha = in.n_alpha;
    if (lp.layout != 4) { lp.n_wg = n_sub; return; }
    std::vector<double> cost(n_sub);
    for (int sc = 0; sc < n_sub; ++sc) cost[sc] = piece_cost(in, lp.pieces[sc]);
    auto dearer = [&](int a, int b) { return cost[a] > cost[b]; };
    auto ds_of = [&](int sc) { return in.elem_ds[lp.pieces[sc].elem]; };
    bool one_ds = true;
    for (int sc = 1; sc < n_sub && one_ds; ++sc) one_ds = ds_of(sc) == ds_of(0);
    if (!one_ds) {
        // static layout (several data sets: a workgroup streams ONE basis, its four pieces come from one data set and it takes no
        // others): group by data set, four per workgroup, -1 pads.  The four pieces of a workgroup run in lock-step until the
        // longest is through, so pieces of like cost go together (the estimate the queue of the one-data-set launch is ordered
        // by), and the workgroups with the longest pieces are dispatched first: with a data set per element the BASELINE batch
        // 2.13 -> 1.29 ms, with two data sets 1.42 -> 0.95 (tools/many_datasets.py, profiles/r05_experiments.txt 12.)
        std::vector<std::vector<int>> by_ds(in.n_ds);
        for (int sc = 0; sc < n_sub; ++sc) by_ds[ds_of(sc)].push_back(sc);
        std::vector<std::pair<double, std::array<int, 4>>> wgs;
        const bool sorted = !in.env.no_sorted_static;
        for (auto& g : by_ds) {
            if (sorted) std::stable_sort(g.begin(), g.end(), dearer);
            for (size_t i0 = 0; i0 < g.size(); i0 += 4) {
                std::array<int, 4> w4;
                for (int q = 0; q < 4; ++q) w4[q] = i0 + q < g.size() ? g[i0 + q] : -1;
                wgs.emplace_back(cost[g[i0]], w4);
            }
        }
        if (sorted) std::stable_sort(wgs.begin(), wgs.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        for (auto& w : wgs) for (int q = 0; q < 4; ++q) lp.wg_chains.push_back(w.second[q]);
        lp.n_wg = (int)lp.wg_chains.size() / 4;
        return;
    }
    // dynamic layout: a persistent grid takes pieces from a queue, most expensive first
    for (int sc = 0; sc < n_sub; ++sc) lp.queue.push_back(sc);
    std::stable_sort(lp.queue.begin(), lp.queue.end(), dearer);
    lp.n_wg = std::min((n_sub + 3) / 4, n_cu * lp.mc_wgpc);
    // The launch ends with its longest pieces: the last pieces of the normal-entropy scans (the most expensive
    // cold start, the most evaluations per alpha).  They are at the head of the queue; with two workgroups per
    // CU, the workgroups that take them get a CU to themselves -- workgroups b and b + n_wg / 2 share one
    // (tools/wg_placement.hip), the partners leave at once --, where a round takes 47 k instead of 69 k cycles
    // (cfg4, 16 such pieces in four workgroups: kernel 1.150 -> 1.123 ms; 16 workgroups 1.130, 64: 1.21).
    // The library's own schedule only, and only where workgroups b and b + n_wg / 2 do share a CU on this device: the caller probes
    lp.solo_rule = o.alpha_split == 0 && lp.mc_wgpc == 2 && lp.n_wg == 2 * n_cu;
    int n_tail = 0;
    for (const Piece& p : lp.pieces) n_tail += normal_elem(in, p.elem) && p.prob0 + p.len == (p.v0 + 1) * n_alpha;
    if (lp.solo_rule) lp.n_solo_wanted = std::min((n_tail + 3) / 4, n_cu / 32);
    // A binary64 launch that does not fill the GPU (one workgroup per CU by the rule above) is as long as its
    // deepest chain of rounds: its first pass runs in chain_kernel_lv -- binary32, V^T in LDS, a round in a
    // fraction of the time --, every alpha to LV_TOL1, and the binary64 kernel then takes every alpha as a piece
    // of its own from that v: P pieces of one alpha, start vector = the record of the first pass
    if (st.lv_fits && st.precision == MXE_PRECISION_F64 && lp.mc_na == 32 && !lp.mc_gst && lp.excluded.empty() && o.lds_basis == 1) {
        const int P2 = in.n_chain * n_alpha;
        lp.lv_mode = 2; lp.mc_wgpc = 1; lp.n_wg = std::min((n_sub + 3) / 4, n_cu);
        lp.wgpc2 = (o.wg_per_cu != 1 && (P2 + 3) / 4 >= 2 * n_cu && lds_mc(in, 32, 2) <= LDS_MC2) ? 2 : 1;
        lp.n_wg2 = std::min((P2 + 3) / 4, n_cu * lp.wgpc2);
    }
}
// ---- stage 8: every problem belongs to exactly one piece, or to the list the finishing pass takes (checked: a problem that
// nothing covers would keep whatever the result buffers held before)
inline bool check_coverage(const PlanInput& in, LaunchPlan& lp)
{
    const size_t P = (size_t)in.n_chain * in.n_alpha;
    std::vector<char> cov(P, 0);
    auto mark = [&](size_t i) { if (cov[i]) ++lp.covered_twice; cov[i] = 1; };
    for (const Piece& p : lp.pieces) for (int i = 0; i < p.len; ++i) mark((size_t)p.prob0 + i);
    for (int x : lp.excluded) mark((size_t)x);
    lp.uncovered = (size_t)std::count(cov.begin(), cov.end(), 0);
    return !lp.uncovered && !lp.covered_twice;
}

}  // namespace plan
// the launch plan of (input): MXE_OK, or MXE_ERR_STATE for a plan that cannot run (nothing of it is to be used then)
inline int plan_launch(const PlanInput& in, LaunchPlan& lp)
{
    lp = LaunchPlan();
    plan::State st;
    plan::choose_precision(in, st);
    plan::pieces_per_scan(in, st, lp);
    std::vector<int> cuts;
    // (scan by scan in ascending order: the ladders are appended as the pieces are)
    for (int c = 0; c < in.n_chain; ++c) { plan::scan_cuts(in, st, c, cuts); plan::emit_scan(in, st, c, cuts, lp); }
    if (const int rc = plan::choose_layout(in, st, lp); rc != MXE_OK) return rc;
    lp.precision = st.precision;
    plan::order_pieces(in, st, lp);
    return plan::check_coverage(in, lp) ? MXE_OK : MXE_ERR_STATE;
}

// ---- The plan of mxe_chains_finish: which alphas the one-chain kernel solves again behind a lock-step launch, as which warm
// chains, from where, over which rungs and with what budgets.  The same rules as above: numbers in, numbers out.
// the environment overrides (read_finish_env() of maxent_hip.hip is the one place that reads them)
struct FinishEnv {
    double ratio = 1.3;                // MXE_FIN_RATIO: largest ratio between two rungs (plan_finish: at least 1.05)
    int rung_iters = 10;               // MXE_FIN_RUNG_ITERS: iterations a rung gets (plan_finish: at least 1)
    bool no_ladder = false;            // MXE_NO_FINISH_LADDER: no rungs
};
struct FinishInput {
    int n_chain = 0, n_alpha = 0, maxiter = 0;   // maxiter: the caller's, over both passes
    const double* alpha = nullptr;               // [n_chain][n_alpha] as the device has them (alpha / eta)
    const int *converged = nullptr, *n_iter = nullptr, *n_evals = nullptr;      // [n_chain][n_alpha]: the records of the lock-step pass
    const int* chain_elem = nullptr;             // [n_chain]
    const int* chain_rows = nullptr;             // [n_chain]: data points of the scan's data set
    FinishEnv env;
};
// where a run starts from: row `index` of the result vectors of the launch, or -- from_v0 -- the start vector of scan `index`
struct FinishStart { bool from_v0; int index; };
struct FinishRun { int elem, entry0, len; FinishStart start; };      // one warm chain: entries [entry0, entry0 + len)
struct FinishPlan {
    std::vector<FinishRun> runs;
    std::vector<double> entry_alpha;             // per entry: an open alpha of the mesh or a rung on the way to one,
    std::vector<int> entry_out, entry_budget;    //   the problem whose record it writes (-1: a rung, no record), the iterations it may spend
    std::vector<char> open;                      // per problem: solved again (its counters are those of both passes)
    int n_open = 0, n_rungs = 0;                 // n_open == 0: nothing to do, the plan is empty
};
namespace plan {
// The rungs of ONE step of a chain from a_from to a_to, either direction: m equal steps of at most env.ratio (at most
// FIN_RUNGS_MAX + 1 of them), the last of them a_to itself, which the caller lays.  Steps first .. m - 1 are laid; step 0 is
// a_from -- a cold start, three times a rung's budget.  A rung has no record; its cost is counted with the alpha it leads to.
inline void lay_rungs(double a_from, double a_to, int first, const FinishEnv& env, FinishPlan& fp)
{
    const double r = a_from > a_to ? a_from / a_to : a_to / a_from;
    int m = (int)std::ceil(std::log(r) / std::log(env.ratio) - 1e-9);
    m = std::max(2, std::min(m, FIN_RUNGS_MAX + 1));
    const double q = std::pow(a_to / a_from, 1.0 / m);
    for (int s = first; s < m; ++s) {
        fp.entry_alpha.push_back(a_from * std::pow(q, s)); fp.entry_out.push_back(-1);
        fp.entry_budget.push_back(s == 0 ? 3 * env.rung_iters : env.rung_iters);
        ++fp.n_rungs;
    }
}
// ---- finish stage 1: what is open: not converged, and iterations of the caller's maxiter left (an alpha that used them up
// stays as it is)
inline void open_problems(const FinishInput& in, FinishPlan& fp)
{
    const size_t P = (size_t)in.n_chain * in.n_alpha;
    fp.open.assign(P, 0);
    for (size_t i = 0; i < P; ++i) if (!in.converged[i] && in.n_iter[i] < in.maxiter) { fp.open[i] = 1; ++fp.n_open; }
}
// ---- finish stage 2: the run of the open alphas [i, j) of scan c.
// The alphas to solve again, as the reference would have reached them: every run of consecutive open alphas of a scan is
// ONE warm-started chain that begins at the solution of the alpha before it (a converged neighbour: 3-5 iterations
// per alpha, where the cold-started piece the lock-step kernel gave up on was stuck far from the minimiser -- on inputs
// whose error bar lies far below their noise a cold start does not get there in thousands of evaluations, the
// reference's warm scan does: tests/golden/stress_reference.npz); a run at the head of a scan starts from the state its
// first alpha was left in.
// Its entries: the open alphas of the mesh and -- where the mesh is too coarse to step on (round 5) -- RUNGS in between.
// What is left to this pass lies deep in the region where the entropy term no longer holds the solution (or couples
// more directions than the lock-step layout takes); there a warm step over the factor 1.9 of the reference's default mesh
// (alpha_meshes.py:81: 20 alphas from 20 down to 1e-4) took 500-2 300 evaluations where ten steps of 10 % take 35 each
// (profiles/r05_b_coarse_mesh.txt, tools/stress.py case 17).  A step over more than FIN_COARSE is therefore cut into equal
// rungs of at most env.ratio; a rung gets env.rung_iters iterations.
inline void emit_run(const FinishInput& in, int c, int i, int j, FinishPlan& fp)
{
    const int na = in.n_alpha, head = c * na + i;
    const double* ac = in.alpha + (size_t)c * na;
    // (a run at the head of a scan starts from the state its first alpha was left in -- if it was ever evaluated: a led piece
    //  that gives up during its WALK leaves no record of its own alpha, and the vector in the result buffer is then whatever
    //  the block held before: the start vector of the scan instead)
    const bool from_v0 = i == 0 && in.n_iter[head] == 0 && in.n_evals[head] == 0;
    const FinishStart start = from_v0 ? FinishStart{true, c} : FinishStart{false, i > 0 ? head - 1 : head};
    const int entry0 = (int)fp.entry_alpha.size();
    if (!in.env.no_ladder && from_v0) {
        // a run that begins at the head of a scan from the default model, deep in the hard region (an ascending mesh, or a
        // mesh that lies there altogether): rungs from N_data / 4 down to its first alpha, like the led pieces of the
        // lock-step kernel (emit_scan) -- the cold start at alpha~ = 0.5 of tools/stress.py case 17 ran into maxiter
        const double a_to = ac[0], a_from = 0.25 * in.chain_rows[c];
        // (only where the mesh goes on FINE from there -- the rising mesh of case 17: 148 -> 150 of 150 converged, 61 -> 8 ms;
        //  case 5: 29 -> 4.5 ms.  With three alphas five decades apart, alpha~ = 0.06 at sigma = 1e-5 on 40 data points, the
        //  cold start with its full budget converged 129 of 192 and the rungs 99-108 at any ratio and budget tried: case 93)
        const bool fine_head = na > 1 && std::max(ac[1] / a_to, a_to / ac[1]) <= FIN_COARSE;
        if (fine_head && a_to * in.env.ratio * in.env.ratio < a_from) lay_rungs(a_from, a_to, 0, in.env, fp);
    }
    for (int k = i; k < j; ++k) {
        if (!in.env.no_ladder && k > 0 && std::max(ac[k - 1] / ac[k], ac[k] / ac[k - 1]) > FIN_COARSE) lay_rungs(ac[k - 1], ac[k], 1, in.env, fp);
        fp.entry_alpha.push_back(ac[k]); fp.entry_out.push_back(c * na + k);
        // the caller's maxiter bounds the iterations of an alpha over BOTH passes, alpha by alpha as the reference caps them
        // (levenberg_minimizer.py:155): every open alpha gets what the lock-step pass left of ITS budget -- an alpha that pass
        // never touched (the rest of an abandoned piece, an excluded alpha: n_iter = 0) the whole of it.  (Until round 5 the pass had
        // ONE budget, that of the open alpha with the most iterations behind it: ADVICE r04.)
        fp.entry_budget.push_back(std::max(1, in.maxiter - in.n_iter[c * na + k]));
    }
    fp.runs.push_back(FinishRun{in.chain_elem[c], entry0, (int)fp.entry_alpha.size() - entry0, start});
}
}  // namespace plan
// the plan of the finishing pass of (input); empty (n_open == 0) when nothing is open
inline void plan_finish(const FinishInput& input, FinishPlan& fp)
{
    FinishInput in = input;
    in.env.ratio = std::max(1.05, in.env.ratio); in.env.rung_iters = std::max(1, in.env.rung_iters);
    fp = FinishPlan();
    plan::open_problems(in, fp);
    if (fp.n_open == 0) return;
    for (int c = 0; c < in.n_chain; ++c)
        for (int i = 0; i < in.n_alpha; ) {
            const char* oc = fp.open.data() + (size_t)c * in.n_alpha;
            if (!oc[i]) { ++i; continue; }
            int j = i;
            while (j < in.n_alpha && oc[j]) ++j;
            plan::emit_run(in, c, i, j, fp);
            i = j;
        }
}

// ---- The build of a chain kernel: which instantiation a launch runs, with how much dynamic LDS.  mxe_chains_launch and
// mxe_chains_finish ask the choosers below; maxent_hip.hip instantiates exactly the builds listed here (LOCKSTEP_BUILDS,
// ONE_CHAIN_BUILDS, and chain_kernel_lv) and finds the kernel of a build in those lists, so a build that is not listed has
// no kernel and is an error, never a neighbouring one.
struct KernelBuild {
    enum Kind { ONE_CHAIN, LOCKSTEP, LV } kind = ONE_CHAIN;
    int NA = 0, WGPC = 0, NWV = 0; bool lead = false, gst = false;      // LOCKSTEP: chain_kernel_mc<NA, WGPC, lead, NWV, gst>
    int NW = 0, NAB = 0; bool f32 = false;                              // ONE_CHAIN: chain_kernel<NW, NAB, float / double, gst>
    size_t lds = 0;                                                     // dynamic LDS of the launch
    int waves() const { return kind == ONE_CHAIN ? NW : NWV; }          // wavefronts of a workgroup
};
// the environment overrides of a launch (diagnostics and A/B runs; read_launch_env() of maxent_hip.hip is the one place that reads them)
struct LaunchEnv {
    bool count_rounds = false;         // MXE_COUNT_ROUNDS: the rounds of every workgroup also where the shipped build does not count them
    bool debug_occ = false;            // MXE_DEBUG_OCC: print how many workgroups of the build a CU holds
    bool has_mc_maxevals = false; int mc_maxevals = 0;       // MXE_MC_MAXEVALS: evaluations the lock-step kernel spends on one alpha (default: 3 x its iterations)
    int stuck_skip = 1;                // MXE_STUCK_SKIP
    int poison_lds = 0;                // MXE_POISON_LDS: 1 / 2, every CU's LDS is written over before the kernel starts
};
struct LockstepKey { int NA, WGPC; bool lead; int NWV; bool gst; };
struct OneChainKey { int NW, NAB; bool f32, gst; };
// (the device-memory-state build is the LEAD build; the 64-row build and two workgroups per CU have four waves)
constexpr LockstepKey LOCKSTEP_BUILDS[] = {
    {32, 2, false, 4, false}, {32, 1, false, 8, false}, {32, 1, false, 4, false}, {64, 1, true, 4, false}, {64, 1, false, 4, false},
    {32, 1, true, 8, true}, {32, 1, true, 4, true}, {32, 2, true, 4, false}, {32, 1, true, 8, false}, {32, 1, true, 4, false}};
// (binary32 only with the 64-row Newton matrix, NAB = 2; device-memory state: four waves, one where NAB = 4 leaves no room for more)
constexpr OneChainKey ONE_CHAIN_BUILDS[] = {
    {4, 2, true, true}, {4, 2, false, true}, {1, 4, false, true}, {1, 2, true, false}, {2, 2, true, false}, {4, 2, true, false},
    {1, 2, false, false}, {1, 4, false, false}, {2, 2, false, false}, {2, 4, false, false}, {4, 2, false, false}, {4, 4, false, false}};
constexpr int N_LOCKSTEP_BUILDS = sizeof(LOCKSTEP_BUILDS) / sizeof(LOCKSTEP_BUILDS[0]), N_ONE_CHAIN_BUILDS = sizeof(ONE_CHAIN_BUILDS) / sizeof(ONE_CHAIN_BUILDS[0]);
// where build b stands in its list (chain_kernel_lv: 0), -1: there is no such kernel
inline int build_index(const KernelBuild& b)
{
    if (b.kind == KernelBuild::LV) return 0;
    if (b.kind == KernelBuild::LOCKSTEP) {
        for (int i = 0; i < N_LOCKSTEP_BUILDS; ++i) {
            const LockstepKey& k = LOCKSTEP_BUILDS[i];
            if (k.NA == b.NA && k.WGPC == b.WGPC && k.lead == b.lead && k.NWV == b.NWV && k.gst == b.gst) return i;
        }
        return -1;
    }
    for (int i = 0; i < N_ONE_CHAIN_BUILDS; ++i) {
        const OneChainKey& k = ONE_CHAIN_BUILDS[i];
        if (k.NW == b.NW && k.NAB == b.NAB && k.f32 == b.f32 && k.gst == b.gst) return i;
    }
    return -1;
}
// The lock-step build of (active block, workgroups per CU, led pieces, device-memory state).  Eight waves (four helpers for
// the streaming passes) where the launch runs one workgroup per CU, i.e. does not fill the GPU and is as long as its deepest
// chain of rounds; mxe_opts.waves_per_chain = 4 / 8 overrides (the passes of that build want n_omega_pad in units of 256).
// MXE_ERR_LIMIT: the build does not fit the LDS
inline int lockstep_build(int NA, int wgpc, bool lead, bool gst, int n_omega_pad, int waves_per_chain, KernelBuild& b)
{
    b = KernelBuild();
    b.kind = KernelBuild::LOCKSTEP; b.NA = NA; b.WGPC = wgpc; b.lead = lead; b.gst = gst;
    b.NWV = (NA == 32 && wgpc == 1 && n_omega_pad % 256 == 0 && waves_per_chain != 4 && mc_lds_bytes(NA, n_omega_pad, 1, 8, gst) <= LDS_MC1) ? 8 : 4;
    b.lds = mc_lds_bytes(NA, n_omega_pad, wgpc, b.NWV, gst);
    return b.lds <= LDS_MC1 ? MXE_OK : MXE_ERR_LIMIT;
}
// The build of the one-chain kernel: NW waves per chain, halved down to nw_min until the LDS takes the chain (the launch: 1;
// the finishing pass never halved: 4).  A frequency mesh whose omega-space state (five arrays per chain) does not fit it even
// then: the state goes to device memory (four waves per chain; one where the 128 x 128 Newton matrix leaves no room for
// more) -- b.gst, the caller provides KParams::gstate.  MXE_ERR_LIMIT: not even that fits, or binary32 with NP = 128
inline int one_chain_build(int NP, int n_omega_pad, int NW, int nw_min, bool f32, KernelBuild& b)
{
    b = KernelBuild();
    b.kind = KernelBuild::ONE_CHAIN; b.NAB = NP / 32; b.f32 = f32;
    if (f32 && NP != 64) return MXE_ERR_LIMIT;
    b.lds = lds_bytes(NP, n_omega_pad, NW, f32);
    while (b.lds > LDS_CU && NW > nw_min) { NW /= 2; b.lds = lds_bytes(NP, n_omega_pad, NW, f32); }
    b.gst = b.lds > LDS_CU;
    if (b.gst) {
        NW = (NP == 64) ? 4 : 1;
        b.lds = lds_bytes(NP, n_omega_pad, NW, f32, true);
    }
    b.NW = NW;
    return b.lds <= LDS_CU ? MXE_OK : MXE_ERR_LIMIT;
}
// waves per chain the one-chain launch asks one_chain_build for: the caller's (eight waves per chain -- two per SIMD at 256
// registers each -- spilled and are not built: four), else enough to fill the 256 CUs x 4 SIMDs: few chains -> more waves per chain
inline int first_waves(int waves_per_chain, int n_sub)
{
    if (waves_per_chain != 0) return std::min(waves_per_chain, 4);
    return (n_sub >= 2048) ? 1 : (n_sub >= 1024) ? 2 : 4;
}
// chain_kernel_lv: one build (32-row active block, led pieces, one workgroup of LV_NWV waves per CU)
inline KernelBuild lv_build(int n_s, int n_omega_pad)
{
    KernelBuild b;
    b.kind = KernelBuild::LV; b.NA = 32; b.WGPC = 1; b.NWV = LV_NWV; b.lead = true; b.lds = lv_lds_bytes(n_s, n_omega_pad);
    return b;
}
// the one place that spells the name of a kernel (mxe_last_kernel_name)
inline std::string build_name(const KernelBuild& b)
{
    switch (b.kind) {
        case KernelBuild::LV: return "mxe::chain_kernel_lv";
        case KernelBuild::LOCKSTEP:
            return "mxe::chain_kernel_mc<" + std::to_string(b.NA) + ", " + std::to_string(b.WGPC) + (b.lead ? ", lead" : "") +
                   (b.NWV == 8 ? ", 8 waves" : "") + (b.gst ? ", device-memory state>" : ">");
        default:
            return "mxe::chain_kernel<" + std::to_string(b.NW) + ", " + std::to_string(b.NAB) + (b.f32 ? ", float" : ", double") +
                   (b.gst ? ", device-memory state>" : ">");
    }
}
// ... and of a two-pass launch: chain_kernel_lv, then every alpha a piece of its own in build `second`
inline std::string two_pass_name(const KernelBuild& first, const KernelBuild& second) { return build_name(first) + " + " + build_name(second) + " per alpha"; }

}  // namespace mxe
