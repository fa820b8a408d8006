// Runs the planners of maxent_amd/csrc/mxe_plan.h stand-alone, on the host.  `plan_dump`: the launch planner of
// mxe_chains_upload -- reads one PlanInput from stdin, prints the LaunchPlan (tests/test_launch_plan_host.py).  `plan_dump finish`:
// the planner of mxe_chains_finish -- reads one FinishInput, prints the FinishPlan (tests/test_finish_plan_host.py; below).
// `plan_dump build`: the choosers of the kernel build -- answers queries with the KernelBuild and its name
// (tests/test_kernel_build_host.py; below).
// tests/plan_dump_build.py builds it:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/plan_dump.cpp -o plan_dump
//
// Input: words separated by white space, `key value...`, in any order except that the counts come before their lists:
//   n_chain N  n_alpha M  n_s K  NP K  n_omega_pad K  n_cu K  wgpc_auto K  mc_wgpc_hint K
//   lds LV MC32x1 MC32x2 MC64x1                     (optional override, bytes; 0: what the formulas of mxe_shapes.h give)
//   opt NAME VALUE                                  (alpha_split wg_per_cu in_flight chains_per_wg precision lds_basis tol_d decouple_tol)
//   env NAME VALUE                                  (taper ladder_ratio no_lds_basis no_split_by_kind no_ladder no_na64 no_sorted_static)
//   elems E  then E x (kind data_set sumD)          ds D  then D x (n_rows c32)
//   elem_of_chain  then n_chain integers            alpha  then n_chain x n_alpha numbers (already divided by chi2_factor)
// Output: `rc`, the scalars of the plan, then pieces (with the a-priori cost of each), walk_alpha, excluded, queue, wg_chains.
#include "../maxent_amd/csrc/mxe_plan.h"
#include <cstdio>
#include <iostream>
#include <cstring>
#include <string>

static int fail(const std::string& what) { std::fprintf(stderr, "plan_dump: %s\n", what.c_str()); return 2; }

// `plan_dump finish`.  Input, `key value...` as above, the counts before their lists:
//   n_chain N  n_alpha M  maxiter K
//   env NAME VALUE                                  (ratio rung_iters no_ladder)
//   rows  then n_chain integers (data points of the scan's data set)       chain_elem  then n_chain integers
//   alpha  then n_chain x n_alpha numbers           converged, n_iter, n_evals  then n_chain x n_alpha integers each
// Output: n_open, n_rungs, runs (elem entry0 len from_v0 index), entries (alpha out budget), open (one flag per problem).
static int finish_main()
{
    mxe::FinishInput in;
    std::vector<double> alpha;
    std::vector<int> rows, chain_elem, converged, n_iter, n_evals;
    std::string key, name;
    auto per_chain = [&](std::vector<int>& v) { if (in.n_chain < 1 || in.n_chain > (1 << 24)) return false; v.resize(in.n_chain); for (int& x : v) std::cin >> x; return true; };
    auto per_problem = [&](auto& v) {
        if (in.n_chain < 1 || in.n_alpha < 1 || (long long)in.n_chain * in.n_alpha > (1 << 26)) return false;
        v.resize((size_t)in.n_chain * in.n_alpha); for (auto& x : v) std::cin >> x; return true;
    };
    while (std::cin >> key) {
        bool counts_first = true;
        if (key == "n_chain") std::cin >> in.n_chain;
        else if (key == "n_alpha") std::cin >> in.n_alpha;
        else if (key == "maxiter") std::cin >> in.maxiter;
        else if (key == "env") {
            double v; std::cin >> name >> v;
            if (name == "ratio") in.env.ratio = v; else if (name == "rung_iters") in.env.rung_iters = (int)v;
            else if (name == "no_ladder") in.env.no_ladder = v != 0;
            else return fail("unknown override " + name);
        } else if (key == "rows") counts_first = per_chain(rows);
        else if (key == "chain_elem") counts_first = per_chain(chain_elem);
        else if (key == "alpha") counts_first = per_problem(alpha);
        else if (key == "converged") counts_first = per_problem(converged);
        else if (key == "n_iter") counts_first = per_problem(n_iter);
        else if (key == "n_evals") counts_first = per_problem(n_evals);
        else return fail("unknown key " + key);
        if (!counts_first) return fail("n_chain and n_alpha come before " + key);
        if (!std::cin) return fail("bad value for " + key);
    }
    const size_t P = (size_t)in.n_chain * in.n_alpha;
    if (in.n_chain < 1 || in.n_alpha < 1 || in.maxiter < 1) return fail("n_chain, n_alpha or maxiter missing");
    if (rows.size() != (size_t)in.n_chain || chain_elem.size() != rows.size()) return fail("rows or chain_elem missing");
    if (alpha.size() != P || converged.size() != P || n_iter.size() != P || n_evals.size() != P) return fail("a list per problem is missing");
    for (double a : alpha) if (!(a > 0.0) || !std::isfinite(a)) return fail("alpha not positive");
    for (int r : rows) if (r < 1) return fail("rows not positive");
    in.alpha = alpha.data(); in.converged = converged.data(); in.n_iter = n_iter.data(); in.n_evals = n_evals.data();
    in.chain_elem = chain_elem.data(); in.chain_rows = rows.data();

    mxe::FinishPlan fp;
    mxe::plan_finish(in, fp);
    std::printf("n_open %d\nn_rungs %d\nruns %zu\n", fp.n_open, fp.n_rungs, fp.runs.size());
    for (const mxe::FinishRun& r : fp.runs) std::printf("%d %d %d %d %d\n", r.elem, r.entry0, r.len, (int)r.start.from_v0, r.start.index);
    std::printf("entries %zu\n", fp.entry_alpha.size());
    for (size_t i = 0; i < fp.entry_alpha.size(); ++i) std::printf("%.17g %d %d\n", fp.entry_alpha[i], fp.entry_out[i], fp.entry_budget[i]);
    std::printf("open %zu\n", fp.open.size());
    for (char o : fp.open) std::printf("%d\n", (int)o);
    return 0;
}

// `plan_dump build`.  The choosers of the kernel build (KernelBuild).  Input: any number of queries, each answered by one line:
//   lockstep NA WGPC LEAD GST N_OMEGA_PAD WAVES_PER_CHAIN        one_chain NP N_OMEGA_PAD NW NW_MIN F32
//   lv N_S N_OMEGA_PAD                                           two_pass N_S N_OMEGA_PAD WGPC2   (lv, then lockstep 32 WGPC2 0 0 .. 0)
//     -> rc kind NA WGPC NWV lead gst NW NAB f32 lds listed | name      (listed: the build has a kernel, build_index >= 0;
//        two_pass: the second build and the name of both)
//   first_waves WAVES_PER_CHAIN N_SUB  -> the waves
static int build_main()
{
    auto print = [](int rc, const mxe::KernelBuild& b, const std::string& name) {
        std::printf("%d %d %d %d %d %d %d %d %d %d %zu %d | %s\n", rc, (int)b.kind, b.NA, b.WGPC, b.NWV, (int)b.lead, (int)b.gst, b.NW, b.NAB,
                    (int)b.f32, b.lds, (int)(mxe::build_index(b) >= 0), name.c_str());
    };
    std::string q;
    while (std::cin >> q) {
        int a[6] = {0, 0, 0, 0, 0, 0};
        const int n = q == "lockstep" ? 6 : q == "one_chain" ? 5 : q == "two_pass" ? 3 : (q == "lv" || q == "first_waves") ? 2 : -1;
        if (n < 0) return fail("unknown query " + q);
        for (int i = 0; i < n; ++i) std::cin >> a[i];
        if (!std::cin) return fail("bad value for " + q);
        mxe::KernelBuild b;
        if (q == "first_waves") { std::printf("%d\n", mxe::first_waves(a[0], a[1])); continue; }
        if (q != "one_chain" && (a[q == "lockstep" ? 4 : 1] < 0 || a[q == "lockstep" ? 4 : 1] > (1 << 24))) return fail("n_omega_pad out of range");
        if (q == "lockstep") { const int rc = mxe::lockstep_build(a[0], a[1], a[2] != 0, a[3] != 0, a[4], a[5], b); print(rc, b, mxe::build_name(b)); }
        else if (q == "one_chain") {
            if ((a[0] != 64 && a[0] != 128) || a[1] < 0 || a[1] > (1 << 24) || a[2] < 1 || a[2] > 4 || a[3] < 1) return fail("one_chain: NP 64 or 128, NW 1 .. 4, NW_MIN >= 1");
            const int rc = mxe::one_chain_build(a[0], a[1], a[2], a[3], a[4] != 0, b); print(rc, b, mxe::build_name(b));
        } else if (q == "lv") { b = mxe::lv_build(a[0], a[1]); print(0, b, mxe::build_name(b)); }
        else { const int rc = mxe::lockstep_build(32, a[2], false, false, a[1], 0, b); print(rc, b, mxe::two_pass_name(mxe::lv_build(a[0], a[1]), b)); }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return std::strcmp(argv[1], "finish") == 0 ? finish_main() : std::strcmp(argv[1], "build") == 0 ? build_main() : fail(std::string("unknown mode ") + argv[1]);
    mxe::PlanInput in;
    in.opts = mxe_opts();
    in.opts.decouple_tol = 1e-5;
    std::vector<int32_t> elem_of_chain;
    std::vector<double> alpha, sumD, c32;
    std::vector<int> kind, eds, rows;
    std::string key, name;
    while (std::cin >> key) {
        if (key == "n_chain") std::cin >> in.n_chain;
        else if (key == "n_alpha") std::cin >> in.n_alpha;
        else if (key == "n_s") std::cin >> in.n_s;
        else if (key == "NP") std::cin >> in.NP;
        else if (key == "n_omega_pad") std::cin >> in.n_omega_pad;
        else if (key == "n_cu") std::cin >> in.n_cu;
        else if (key == "wgpc_auto") std::cin >> in.wgpc_auto;
        else if (key == "mc_wgpc_hint") std::cin >> in.mc_wgpc_hint;
        else if (key == "lds") std::cin >> in.lds_override[0] >> in.lds_override[1] >> in.lds_override[2] >> in.lds_override[3];
        else if (key == "opt") {
            double v; std::cin >> name >> v;
            mxe_opts& o = in.opts;
            if (name == "alpha_split") o.alpha_split = (int)v; else if (name == "wg_per_cu") o.wg_per_cu = (int)v;
            else if (name == "in_flight") o.in_flight = (int)v; else if (name == "chains_per_wg") o.chains_per_wg = (int)v;
            else if (name == "precision") o.precision = (int)v; else if (name == "lds_basis") o.lds_basis = (int)v;
            else if (name == "tol_d") o.tol_d = v; else if (name == "decouple_tol") o.decouple_tol = v;
            else return fail("unknown option " + name);
        } else if (key == "env") {
            double v; std::cin >> name >> v;
            mxe::PlanEnv& e = in.env;
            if (name == "taper") e.taper = v; else if (name == "ladder_ratio") e.ladder_ratio = v;
            else if (name == "no_lds_basis") e.no_lds_basis = v != 0; else if (name == "no_split_by_kind") e.no_split_by_kind = v != 0;
            else if (name == "no_ladder") e.no_ladder = v != 0; else if (name == "no_na64") e.no_na64 = v != 0;
            else if (name == "no_sorted_static") e.no_sorted_static = v != 0;
            else return fail("unknown override " + name);
        } else if (key == "elems") {
            size_t n; std::cin >> n;
            if (!std::cin || n > (1u << 24)) return fail("bad element count");
            kind.resize(n); eds.resize(n); sumD.resize(n);
            for (size_t i = 0; i < n; ++i) std::cin >> kind[i] >> eds[i] >> sumD[i];
        } else if (key == "ds") {
            size_t n; std::cin >> n;
            if (!std::cin || n > (1u << 24)) return fail("bad data set count");
            rows.resize(n); c32.resize(n);
            for (size_t i = 0; i < n; ++i) std::cin >> rows[i] >> c32[i];
        } else if (key == "elem_of_chain") {
            if (in.n_chain < 1 || in.n_chain > (1 << 24)) return fail("n_chain comes before elem_of_chain");
            elem_of_chain.resize(in.n_chain);
            for (auto& e : elem_of_chain) std::cin >> e;
        } else if (key == "alpha") {
            if (in.n_chain < 1 || in.n_alpha < 1 || (long long)in.n_chain * in.n_alpha > (1 << 26)) return fail("n_chain and n_alpha come before alpha");
            alpha.resize((size_t)in.n_chain * in.n_alpha);
            for (auto& a : alpha) std::cin >> a;
        } else return fail("unknown key " + key);
        if (!std::cin) return fail("bad value for " + key);
    }
    // what mxe_chains_upload checks before it plans
    if (elem_of_chain.size() != (size_t)in.n_chain || in.n_chain < 1 || alpha.size() != (size_t)in.n_chain * in.n_alpha) return fail("elem_of_chain or alpha missing");
    for (int e : elem_of_chain) if (e < 0 || (size_t)e >= kind.size()) return fail("element out of range");
    for (int d : eds) if (d < 0 || (size_t)d >= rows.size()) return fail("data set out of range");
    for (double a : alpha) if (!(a > 0.0) || !std::isfinite(a)) return fail("alpha not positive");
    if (in.n_cu < 1 || in.opts.alpha_split < 0 || in.opts.in_flight < 0) return fail("bad n_cu or option");
    in.elem_of_chain = elem_of_chain.data(); in.alpha = alpha.data();
    in.elem_kind = kind.data(); in.elem_ds = eds.data(); in.elem_sumD = sumD.data();
    in.n_ds = (int)rows.size(); in.ds_rows = rows.data(); in.ds_c32 = c32.data();

    mxe::LaunchPlan lp;
    const int rc = mxe::plan_launch(in, lp);
    std::printf("rc %d\nprecision %d\nlayout %d\nmc_na %d\nmc_wgpc %d\nmc_gst %d\nlv_mode %d\nwgpc_auto %d\nmc_wgpc_hint %d\n", rc, lp.precision,
                lp.layout, lp.mc_na, lp.mc_wgpc, (int)lp.mc_gst, lp.lv_mode, lp.wgpc_auto, lp.mc_wgpc_hint);
    std::printf("n_wg %d\nn_wg2 %d\nwgpc2 %d\nsolo_rule %d\nn_solo_wanted %d\nuncovered %zu\ncovered_twice %zu\n", lp.n_wg, lp.n_wg2, lp.wgpc2,
                (int)lp.solo_rule, lp.n_solo_wanted, lp.uncovered, lp.covered_twice);
    std::printf("pieces %zu\n", lp.pieces.size());
    for (const mxe::Piece& p : lp.pieces)
        std::printf("%d %d %d %d %d %d %.17g\n", p.elem, p.prob0, p.len, p.v0, p.pre, p.walk0, mxe::plan::piece_cost(in, p));
    std::printf("walk_alpha %zu\n", lp.walk_alpha.size());
    for (double a : lp.walk_alpha) std::printf("%.17g\n", a);
    auto ints = [](const char* what, const std::vector<int>& v) {
        std::printf("%s %zu\n", what, v.size());
        for (int x : v) std::printf("%d\n", x);
    };
    ints("excluded", lp.excluded); ints("queue", lp.queue); ints("wg_chains", lp.wg_chains);
    return 0;
}
