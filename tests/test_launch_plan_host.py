"""The launch planner of mxe_chains_upload (maxent_amd/csrc/mxe_plan.h) on the host: tools/plan_dump.cpp, a stand-alone program
built with the system compiler (with the address and undefined-behaviour sanitizers where the compiler links them), is fed
synthetic PlanInputs -- n_cu = 256 as data -- and its LaunchPlan is checked: the invariants of every plan, and the decisions
DESIGN.md section 4 states, derived by hand from the rules."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_dump_build import plan_dump_binary, run_plan_dump as run_text

NORMAL, PM = 0, 1
N_CU = 256
LADDER_RATIO = 1.56
LV_ACAP = 16             # alphas of a slot's piece that chain_kernel_lv keeps in LDS (mxe_shapes.h)
# dynamic LDS of chain_kernel_lv with its static arrays and of chain_kernel_mc<32, 1>, <32, 2>, <64, 1>: 0 = what the planner's own
# formulas give (mxe_shapes.h; at n_omega_pad = 512, n_s = 56: 161 536, 98 304, 77 824, 155 648 -- all of them fit 160 KB, 160 KB - 6 KB,
# 80 KB - 2 KB, 160 KB - 6 KB; tests/test_kernel_build_host.py derives them).  A case overrides one with TOO_BIG to say "does not fit"
LDS = dict(lv=0, mc32x1=0, mc32x2=0, mc64x1=0)
TOO_BIG = 200000


@pytest.fixture(scope='session')
def plan_dump(tmp_path_factory):
    return plan_dump_binary(tmp_path_factory)


def mesh(n_alpha, hi=1e4, lo=1e-2, n_tau=200):
    """alpha~ of a logarithmic mesh from hi down to lo (the BASELINE mesh: synthetic.alpha_mesh), times the data points"""
    return n_tau * hi * (lo / hi) ** (np.arange(n_alpha) / max(1, n_alpha - 1))


def case(kinds, alphas, ds_of_elem=None, rows=(200,), c32=None, sumD=1.0, n_s=56, NP=64, n_omega_pad=512, lds=None, opts=None, env=None,
         wgpc_auto=2):
    """one element per scan; alphas [n_alpha] (shared) or [n_chain][n_alpha]"""
    kinds = list(kinds)
    a = np.asarray(alphas, dtype=float)
    if a.ndim == 1:
        a = np.tile(a, (len(kinds), 1))
    return dict(kinds=kinds, alpha=a, ds=list(ds_of_elem) if ds_of_elem is not None else [0] * len(kinds), rows=list(rows),
                c32=list(c32) if c32 is not None else [0.0] * len(rows), sumD=sumD, n_s=n_s, NP=NP, n_omega_pad=n_omega_pad,
                lds=dict(LDS, **(lds or {})), opts=dict(opts or {}), env=dict(env or {}), wgpc_auto=wgpc_auto)


def text_of(c):
    n_chain, n_alpha = c['alpha'].shape
    w = ['n_chain %d n_alpha %d n_s %d NP %d n_omega_pad %d n_cu %d wgpc_auto %d' % (n_chain, n_alpha, c['n_s'], c['NP'], c['n_omega_pad'], N_CU, c['wgpc_auto']),
         'lds %d %d %d %d' % (c['lds']['lv'], c['lds']['mc32x1'], c['lds']['mc32x2'], c['lds']['mc64x1'])]
    w += ['opt %s %r' % kv for kv in sorted(c['opts'].items())] + ['env %s %r' % kv for kv in sorted(c['env'].items())]
    w.append('elems %d ' % n_chain + ' '.join('%d %d %r' % (k, d, float(c['sumD'])) for k, d in zip(c['kinds'], c['ds'])))
    w.append('ds %d ' % len(c['rows']) + ' '.join('%d %r' % (r, float(x)) for r, x in zip(c['rows'], c['c32'])))
    w.append('elem_of_chain ' + ' '.join(str(i) for i in range(n_chain)))
    w.append('alpha ' + ' '.join(repr(float(x)) for x in c['alpha'].ravel()))
    return '\n'.join(w) + '\n'


def parse(out):
    lines = out.split('\n')
    p, i = {}, 0
    while i < len(lines) and lines[i]:
        key, val = lines[i].split()
        i += 1
        if key in ('pieces', 'walk_alpha', 'excluded', 'queue', 'wg_chains'):
            rows = lines[i:i + int(val)]
            i += int(val)
            if key == 'pieces':
                p['pieces'] = [dict(zip(('elem', 'prob0', 'len', 'v0', 'pre', 'walk0'), map(int, r.split()[:6])), cost=float(r.split()[6])) for r in rows]
            elif key == 'walk_alpha':
                p[key] = [float(r) for r in rows]
            else:
                p[key] = [int(r) for r in rows]
        else:
            p[key] = int(val)
    return p


def check_invariants(c, p):
    n_chain, n_alpha = c['alpha'].shape
    P = n_chain * n_alpha
    alpha = c['alpha'].ravel()
    pieces = p['pieces']
    if p['rc'] != 0:
        return
    assert p['uncovered'] == 0 and p['covered_twice'] == 0
    # each problem lies in exactly one piece or in excluded
    count = np.zeros(P, dtype=int)
    for q in pieces:
        assert q['len'] >= 1 and q['prob0'] // n_alpha == q['v0'] == (q['prob0'] + q['len'] - 1) // n_alpha and q['elem'] == q['v0']
        count[q['prob0']:q['prob0'] + q['len']] += 1
    excluded = set(p['excluded'])
    assert len(excluded) == len(p['excluded'])
    for x in excluded:
        count[x] += 1
    assert (count == 1).all()
    # the pieces of a scan are contiguous and ascending (what lies between two of them is excluded)
    for a, b in zip(pieces, pieces[1:]):
        assert b['v0'] >= a['v0']
        if a['v0'] == b['v0']:
            assert b['prob0'] >= a['prob0'] + a['len']
            assert all(x in excluded for x in range(a['prob0'] + a['len'], b['prob0']))
    # led and laddered pieces fit the slot's table of 32 alphas; the ladders
    in_lv = p['lv_mode'] in (1, 2)
    for q in pieces:
        assert q['pre'] >= 0 and (q['pre'] > 0 or q['walk0'] == -1)
        if q['pre'] > 0:
            assert q['pre'] + q['len'] <= 32
        if q['walk0'] >= 0:
            assert 1 <= q['pre'] <= 28
            # chain_kernel_lv walks rungs from its table of LV_ACAP alphas only (alpha_at: a piece beyond the table reads the scan's mesh)
            if in_lv:
                assert q['pre'] + q['len'] <= LV_ACAP, (q, p['lv_mode'])
            rungs = p['walk_alpha'][q['walk0']:q['walk0'] + q['pre']]
            assert len(rungs) == q['pre']
            a = alpha[q['prob0']]
            assert all(x > y for x, y in zip(rungs, rungs[1:])) and rungs[-1] > a
            # equal rungs from max(N_data / 4, a x LADDER_RATIO) down to a: of at most LADDER_RATIO unless the table cuts their number
            top = max(0.25 * c['rows'][c['ds'][q['elem']]], a * LADDER_RATIO)
            np.testing.assert_allclose(rungs, a * (top / a) ** (np.arange(q['pre'], 0, -1) / q['pre']), rtol=1e-12)
            if q['pre'] + q['len'] < LV_ACAP if in_lv else (q['pre'] < 28 and q['pre'] + q['len'] < 30):
                assert rungs[-1] / a <= LADDER_RATIO * (1 + 1e-12)
        elif q['pre'] > 0:
            assert q['prob0'] - q['pre'] >= q['v0'] * n_alpha          # led by an alpha of its own scan
    layout, n = p['layout'], len(pieces)
    if layout != 4:
        assert p['n_wg'] == n and not p['queue'] and not p['wg_chains'] and not excluded and not p['walk_alpha']
        assert all(q['pre'] == 0 and q['walk0'] == -1 for q in pieces)
    elif p['wg_chains']:
        # static layout: the four entries of a workgroup share one data set
        assert not p['queue'] and len(p['wg_chains']) == 4 * p['n_wg']
        assert sorted(x for x in p['wg_chains'] if x >= 0) == list(range(n))
        for g in range(p['n_wg']):
            four = p['wg_chains'][4 * g:4 * g + 4]
            assert four[0] >= 0 and len({c['ds'][pieces[x]['elem']] for x in four if x >= 0}) == 1
    else:
        # the queue is a permutation whose costs do not increase
        assert sorted(p['queue']) == list(range(n))
        costs = [pieces[x]['cost'] for x in p['queue']]
        assert all(x >= y for x, y in zip(costs, costs[1:]))
        if p['lv_mode'] == 2:
            assert p['mc_wgpc'] == 1 and p['n_wg'] == min((n + 3) // 4, N_CU)
            assert p['wgpc2'] in (1, 2) and p['n_wg2'] == min((P + 3) // 4, N_CU * p['wgpc2'])
        else:
            assert p['n_wg'] == min((n + 3) // 4, N_CU * p['mc_wgpc'])
    if layout == 4:
        assert p['mc_na'] in (32, 64) and p['mc_wgpc'] in (1, 2) and (p['mc_wgpc'] == 1 or p['mc_na'] == 32)
    if p['lv_mode'] == 1:
        assert p['mc_na'] == 32 and not excluded and p['mc_wgpc'] == 1
    if p['n_solo_wanted'] > 0:
        assert p['solo_rule'] and p['mc_wgpc'] == 2 and p['n_wg'] == 2 * N_CU


def plan(binary, c):
    p = parse(run_text(binary, text_of(c)))
    check_invariants(c, p)
    return p


def starts(p, scan, n_alpha):
    return [q['prob0'] - scan * n_alpha for q in p['pieces'] if q['v0'] == scan]


def baseline_mix(n_normal=16, n_pm=240, **kw):
    """the BASELINE batch: normal entropy on the diagonal of a matrix, plus-minus off it; 100 alphas, 200 data points"""
    kinds = [NORMAL if i < n_normal else PM for i in range(n_normal + n_pm)]
    return case(kinds, mesh(100), **kw)


def test_baseline_batch_fills_the_gpu_at_two_workgroups_per_cu(plan_dump):
    """DESIGN section 4 (auto rule): 256 scans x 15 pieces on 512 workgroups; a normal-entropy piece counts twice -- 2 x 2048 slots /
    (2 x 16 + 240) = 15 --, cut at 100 s / 15; the last pieces of the 16 normal-entropy scans in min((16 + 3) / 4, 256 / 32) = 4 solo
    workgroups"""
    p = plan(plan_dump, baseline_mix())
    uniform = sorted({100 * s // 15 for s in range(15)})
    for scan in (0, 15, 16, 100, 255):
        assert starts(p, scan, 100) == uniform
    # (the last piece starts at alpha 93 of 100, above the last 6 % of the logarithmic range: it runs into the guarded tail whole)
    assert all(q['pre'] == 0 for q in p['pieces'])
    assert (p['layout'], p['mc_na'], p['mc_wgpc'], p['wgpc_auto'], p['n_wg'], p['lv_mode'], p['precision']) == (4, 32, 2, 2, 512, 0, 0)
    assert p['solo_rule'] == 1 and p['n_solo_wanted'] == min((16 + 3) // 4, 256 // 32) == 4
    assert not p['excluded'] and not p['walk_alpha']


def test_batches_in_flight_take_fewer_pieces(plan_dump):
    """mxe_opts.in_flight = 4: 2 x 2048 / (272 x 4), rounded up: 4 pieces per scan"""
    p = plan(plan_dump, baseline_mix(opts=dict(in_flight=4)))
    assert starts(p, 100, 100) == [0, 25, 50, 75]
    assert set(starts(p, 0, 100)) >= {0, 25, 50, 75}


def test_a_shard_that_does_not_fill_the_gpu_is_cut_by_cost(plan_dump):
    """the 32-scan shard of the BASELINE batch on eight GPUs (2 normal + 30 plus-minus scans): one workgroup per CU, pieces of equal
    cost and no more of them than the 4 x n_cu slots (launches that do not fill the GPU: four alphas at the top of
    the mesh, one next to the tail)"""
    p = plan(plan_dump, baseline_mix(2, 30))
    assert (p['layout'], p['mc_wgpc'], p['wgpc_auto']) == (4, 1, 1)
    assert len(p['pieces']) <= 4 * N_CU
    normal = [q for q in p['pieces'] if q['v0'] == 0]
    assert normal[0]['len'] == 4 and max(q['len'] for q in normal) <= 6
    plain = [q['len'] for q in normal if q['pre'] == 0]
    assert plain[-1] == 1 and all(x >= y for x, y in zip(plain, plain[1:]))
    pm = [q['len'] for q in p['pieces'] if q['v0'] == 31]
    assert len(set(pm)) > 1 and pm[0] >= pm[-1] and max(pm) <= 9       # cheaper alphas at the top: longer pieces there; at most nine
    # MXE_NO_SPLIT_BY_KIND: the uniform cut, pieces of two alphas
    q = plan(plan_dump, baseline_mix(2, 30, env=dict(no_split_by_kind=1)))
    assert starts(q, 31, 100) == list(range(0, 100, 2)) and len(q['pieces']) > 4 * N_CU


def test_many_scans_take_the_count_of_least_loss(plan_dump):
    """48 x 48 elements: two pieces per slot would be fewer than six per scan, so the count minimises
    4 / (4 + 2 len) + 0.5 / (pieces per slot): the cold start of a piece against the imbalance of the queue"""
    n_normal, n_pm, n_alpha = 48, 2256, 100
    weight, n_slots = 2 * n_normal + n_pm, 4 * 2 * N_CU
    want = max(1, 2 * n_slots // weight)
    assert want < 6
    best, expected = 1e300, None
    for sp in range(max(1, want), min(16, n_alpha // 4) + 1):
        loss = 4.0 / (4.0 + 2.0 * (n_alpha / sp)) + 0.5 / (sp * weight / n_slots)
        if loss < best:
            best, expected = loss, sp
    p = plan(plan_dump, baseline_mix(n_normal, n_pm))
    assert starts(p, 2000, 100) == sorted({100 * s // expected for s in range(expected)})
    assert (p['mc_wgpc'], p['n_wg']) == (2, 512)


def test_a_coarse_mesh_gets_ladders(plan_dump):
    """five alphas over five decades on 200 data points: every alpha below N_data / 4 that is more than a factor 2 from its
    neighbour is a laddered piece of its own; the head of the scan is not (a mesh too coarse to walk on)"""
    a = mesh(5, hi=1e1, lo=1e-4)
    p = plan(plan_dump, case([NORMAL, PM], a))
    for scan in (0, 1):
        qs = [q for q in p['pieces'] if q['v0'] == scan]
        for i in range(1, 5):
            if a[i] < 200 / 4:
                (q,) = [q for q in qs if q['prob0'] == scan * 5 + i]
                assert q['len'] == 1 and q['walk0'] >= 0 and q['pre'] == max(1, math.ceil(math.log(max(50.0, a[i] * LADDER_RATIO) / a[i]) / math.log(LADDER_RATIO) - 1e-9))
        assert sum(a < 50) == 3
        head = qs[0]
        assert head['prob0'] == scan * 5 and head['pre'] == 0 and head['walk0'] == -1
    off = plan(plan_dump, case([NORMAL, PM], a, env=dict(no_ladder=1)))
    assert not off['walk_alpha']


def rungs_wanted(a, n_data):
    return max(1, math.ceil(math.log(max(0.25 * n_data, a * LADDER_RATIO) / a) / math.log(LADDER_RATIO) - 1e-9))


@pytest.mark.parametrize('n_tau', [30, 100, 200])
@pytest.mark.parametrize('n_alpha,lo', [(4, 1e-4), (8, 1e-5)])
@pytest.mark.parametrize('opts,lv_mode', [(dict(precision=1), 1), (dict(lds_basis=1), 2)])
def test_ladders_of_a_launch_in_chain_kernel_lv_fit_its_table_of_16(plan_dump, opts, lv_mode, n_alpha, lo, n_tau):
    """A coarse mesh (alpha~ from 1e2 down to 1e-4 on 4 points, to 1e-5 on 8) in chain_kernel_lv, as the launch (precision = F32)
    and as the first pass (lds_basis = 1).  chain_kernel_mc holds 32 alphas per slot and gets up to 28 rungs; chain_kernel_lv holds
    LV_ACAP = 16, and alpha_at sends a piece with more entries to the scan's mesh, where no rung is: rungs + alphas of a laddered
    piece are at most 16 there (check_invariants), and exactly 16 where a ratio of 1.56 would want more.  The same mesh without
    the option keeps the long ladders.  (Until the planner knew the table the lv plans held the pieces of the other kernel: n_tau
    = 100, four alphas: 18 and 23 rungs + 1.)"""
    a = mesh(n_alpha, hi=1e2, lo=lo, n_tau=n_tau)
    p = plan(plan_dump, case([NORMAL, PM], a, rows=(n_tau,), opts=opts))
    assert (p['rc'], p['lv_mode'], p['layout'], p['mc_na']) == (0, lv_mode, 4, 32)
    mc = plan(plan_dump, case([NORMAL, PM], a, rows=(n_tau,)))
    assert mc['lv_mode'] == 0 and len(mc['pieces']) == len(p['pieces'])
    laddered, longest = 0, 0
    for q, q_mc in zip(p['pieces'], mc['pieces']):
        assert (q['prob0'], q['len'], q['walk0'] >= 0) == (q_mc['prob0'], q_mc['len'], q_mc['walk0'] >= 0)
        if q['walk0'] >= 0:
            want = rungs_wanted(a[q['prob0'] % n_alpha], n_tau)
            assert q['pre'] == min(want, LV_ACAP - q['len']) and q_mc['pre'] == min(want, 28, 30 - q_mc['len'])
            laddered += 1
            longest = max(longest, want + q['len'])
    # every alpha below N_data / 4 but the head of a scan is such a piece, and some of them wanted more than the table holds
    assert laddered == 2 * int(np.sum(a[1:] < 0.25 * n_tau)) and longest > LV_ACAP


def test_a_long_piece_deep_in_the_hard_region_is_laddered_in_chain_kernel_lv_only_where_the_table_takes_it(plan_dump):
    """an ascending scan in the hard region: every piece is led down a ladder to its first alpha -- in chain_kernel_lv pieces of up
    to LV_ACAP - 8 alphas (the other kernels: 32 - 8), so that at least eight rungs fit; a longer piece starts cold"""
    a = 0.5 * 1.09 ** np.arange(40)
    for split, laddered in ((5, True), (4, False)):            # pieces of 8 and of 10 alphas
        p = plan(plan_dump, case([NORMAL, PM], a, opts=dict(precision=1, alpha_split=split)))
        assert p['lv_mode'] == 1 and all(q['len'] == 40 // split for q in p['pieces'])
        assert all((q['walk0'] >= 0) == laddered for q in p['pieces'])
        assert all(q['pre'] == (min(rungs_wanted(a[q['prob0'] % 40], 200), LV_ACAP - q['len']) if laddered else 0) for q in p['pieces'])
    p = plan(plan_dump, case([NORMAL, PM], a, opts=dict(alpha_split=4)))
    assert p['lv_mode'] == 0 and all(q['walk0'] >= 0 and q['len'] == 10 for q in p['pieces'])


def test_an_ascending_scan_in_the_hard_region_starts_every_piece_with_a_ladder(plan_dump):
    a = 0.5 * 1.09 ** np.arange(40)
    assert a[-1] * LADDER_RATIO ** 2 < 50
    p = plan(plan_dump, case([NORMAL, PM], a))
    assert all(q['walk0'] >= 0 and q['pre'] >= 1 for q in p['pieces'])


def coupled(k, n_normal=16, n_pm=240, **kw):
    """the BASELINE batch with a c[32] that fails the coupling bound c32^2 max(1, sum D) / alpha <= 1e-3 at the k smallest alphas"""
    a = mesh(100)
    thr = math.sqrt(a[100 - k] * a[100 - k - 1])
    return baseline_mix(n_normal, n_pm, c32=[math.sqrt(1e-3 * thr)], **kw)


def test_more_than_32_coupled_directions(plan_dump):
    tail = lambda scans, k: sorted(s * 100 + i for s in scans for i in range(100 - k, 100))
    # the 64-row build fits: plus-minus scans whole, normal-entropy scans end at the cut
    p = plan(plan_dump, coupled(27))
    assert (p['layout'], p['mc_na'], p['mc_wgpc']) == (4, 64, 1)
    assert p['excluded'] == tail(range(16), 27)
    assert starts(p, 100, 100) == sorted({100 * s // 15 for s in range(15)})
    # it does not (or MXE_NO_NA64): every scan is cut
    for kw in (dict(lds=dict(mc64x1=TOO_BIG)), dict(env=dict(no_na64=1))):
        p = plan(plan_dump, coupled(27, **kw))
        assert (p['layout'], p['mc_na']) == (4, 32) and p['excluded'] == tail(range(256), 27)
    # more than a third of the alphas would be left to the finishing pass: the one-chain layout
    p = plan(plan_dump, coupled(40, lds=dict(mc64x1=TOO_BIG)))
    assert p['layout'] == 1 and p['mc_na'] == 0 and not p['excluded']
    # a binary32 request in that state is promoted to the binary64 lock-step build
    p = plan(plan_dump, coupled(27, opts=dict(precision=1, wg_per_cu=1)))
    assert (p['precision'], p['layout'], p['mc_na'], p['lv_mode']) == (0, 4, 64, 0)


def test_binary32_requests(plan_dump):
    # a small batch: chain_kernel_lv is the launch
    p = plan(plan_dump, baseline_mix(4, 12, opts=dict(precision=1)))
    assert (p['precision'], p['lv_mode'], p['mc_na'], p['mc_wgpc'], p['layout']) == (1, 1, 32, 1, 4)
    # a batch that fills the GPU at two workgroups per CU is promoted; wg_per_cu = 1 keeps chain_kernel_lv
    p = plan(plan_dump, baseline_mix(opts=dict(precision=1)))
    assert (p['precision'], p['lv_mode'], p['mc_wgpc']) == (0, 0, 2)
    p = plan(plan_dump, baseline_mix(opts=dict(precision=1, wg_per_cu=1)))
    assert (p['precision'], p['lv_mode'], p['mc_wgpc']) == (1, 1, 1)
    # a basis that does not fit the LDS as binary32: promoted; lds_basis = 2 keeps the one-chain binary32 kernel
    big = dict(n_omega_pad=640, lds=dict(lv=TOO_BIG))
    p = plan(plan_dump, baseline_mix(opts=dict(precision=1), **big))
    assert (p['precision'], p['layout']) == (0, 4)
    p = plan(plan_dump, baseline_mix(opts=dict(precision=1, lds_basis=2), **big))
    assert (p['precision'], p['layout']) == (1, 1)
    assert max(q['len'] for q in p['pieces']) >= 6 and len(starts(p, 100, 100)) <= 16
    # lds_basis = 1 on a binary64 launch: the two-pass mode
    p = plan(plan_dump, baseline_mix(4, 12, opts=dict(lds_basis=1)))
    assert (p['precision'], p['lv_mode'], p['mc_wgpc']) == (0, 2, 1)


@pytest.mark.parametrize('opts', [dict(chains_per_wg=1), dict(tol_d=1e-4)])
def test_the_one_chain_layout_has_no_led_pieces(plan_dump, opts):
    """layout 1: no pre, no walk0 (check_invariants), and the led tail of a normal-entropy scan is joined to the piece before it"""
    p = plan(plan_dump, baseline_mix(opts=opts))
    assert p['layout'] == 1 and p['n_wg'] == len(p['pieces'])
    n = 7 if 'chains_per_wg' in opts else 15          # (chains_per_wg = 1 is planned for one workgroup per CU: 2 x 1024 slots / 272)
    uniform = sorted({100 * s // n for s in range(n)})
    assert starts(p, 0, 100) == uniform and starts(p, 100, 100) == uniform
    # pieces of two alphas: the single led alphas 94 .. 99 of the lock-step layout (test_explicit_split_...) are joined to the piece at 92
    p = plan(plan_dump, baseline_mix(opts=dict(opts, alpha_split=50)))
    assert starts(p, 0, 100) == list(range(0, 94, 2)) and starts(p, 100, 100) == list(range(0, 100, 2))
    assert [q['len'] for q in p['pieces'] if q['v0'] == 0][-1] == 8
    # ... also where the pieces were laddered
    a = mesh(5, hi=1e1, lo=1e-4)
    p = plan(plan_dump, case([NORMAL, PM], a, opts=opts))
    assert p['layout'] == 1 and not p['walk_alpha']


def test_two_data_sets_take_the_static_layout(plan_dump):
    c = baseline_mix(ds_of_elem=[e % 2 for e in range(256)], rows=(200, 200))
    p = plan(plan_dump, c)
    assert p['layout'] == 4 and p['wg_chains'] and not p['queue'] and p['solo_rule'] == 0
    first = [p['pieces'][p['wg_chains'][4 * g]]['cost'] for g in range(p['n_wg'])]
    assert all(x >= y for x, y in zip(first, first[1:]))          # workgroups by the cost of their first piece


def test_explicit_split_keeps_the_last_auto_choice(plan_dump):
    """alpha_split > 0 skips the auto rule: workgroups per CU as that rule chose last (wgpc_auto of the input)"""
    for last in (1, 2):
        p = plan(plan_dump, baseline_mix(opts=dict(alpha_split=7), wgpc_auto=last))
        assert p['wgpc_auto'] == last and p['mc_wgpc'] == last and p['solo_rule'] == 0
        assert starts(p, 100, 100) == sorted({100 * s // 7 for s in range(7)})
    p = plan(plan_dump, baseline_mix(opts=dict(alpha_split=1)))
    assert len(p['pieces']) == 256 and p['n_wg'] == 64
    # pieces of two alphas: those of a normal-entropy scan that START in the last 6 % of its logarithmic range (alpha 94 of 100 on)
    # are single alphas led by the last alpha above it, 93
    p = plan(plan_dump, baseline_mix(opts=dict(alpha_split=50)))
    assert starts(p, 0, 100) == list(range(0, 94, 2)) + list(range(94, 100)) and starts(p, 100, 100) == list(range(0, 100, 2))
    assert [q['pre'] for q in p['pieces'] if q['v0'] == 0 and q['prob0'] >= 94] == [1, 2, 3, 4, 5, 6]


def test_the_plan_is_deterministic(plan_dump):
    for c in (baseline_mix(), coupled(27), baseline_mix(2, 30), case([NORMAL, PM], mesh(5, hi=1e1, lo=1e-4))):
        t = text_of(c)
        assert run_text(plan_dump, t) == run_text(plan_dump, t)
