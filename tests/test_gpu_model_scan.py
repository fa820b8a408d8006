"""Default-model scans on the device: ``mxe_evidence_reduce`` against its longdouble restatement
(tests/model_scan_ref.py) with the bounds derived there, its bitwise promises and refusals, and ``default_model_scan`` end
to end against a loop of ``TauMaxEnt(probability='normal')`` objects, one per default model.

Measured on the MI355X (the tests print their own figures): worst error / bound of the kernel test 0.47 (a weight over
alpha); largest rel L2 of ``A_models`` to the loop 1.5e-16, audit 3.1e-10; largest |log_evidence - the same sum formed on
the host from the loop's probabilities| 0: a scan's bits do not depend on the launch it is in, and the device's exp and
log agreed with numpy's on these terms.  Ten times that is 0, so the gate is what remains when another libm rounds the
last bit the other way: the rounding of the sum itself, (n_alpha + 8) eps |log Z| (3e-13 here), and never above 1e-4."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, model_scan
from model_scan_ref import evidence_reduce_ref, scan_problem, EPS

pytestmark = pytest.mark.gpu

GATE = 1e-6                 # the project's parity gate, relative L2
MEASURED_EVIDENCE_GAP = 0.0


def evidence_gate(log_evidence, n_alpha):
    """ten times the largest difference measured (see above) plus the rounding of the sum itself, never above 1e-4"""
    return min(10 * MEASURED_EVIDENCE_GAP + (n_alpha + 8) * EPS * float(np.max(np.abs(log_evidence))), 1e-4)


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def rel_l2(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b), axis=-1) / np.linalg.norm(np.asarray(b), axis=-1)


def _ctx(n_omega):
    n_s = min(n_omega, 4)
    rng = np.random.RandomState(n_omega)
    return device.DeviceContext(rng.randn(6, n_s), np.linspace(1.0, 0.1, n_s), np.linalg.qr(rng.randn(n_omega, n_s))[0])


# ---- the kernel against the reference, H from the host ------------------------------------------------------------------------
SIZES = [0, 1, 2, 7]                        # scans per group: 10 scans


def _case(n_omega, n_alpha, seed=0):
    """10 scans in groups of 0, 1, 2 and 7.  logp over 8000 nats (every other scan: over 5, so that several alphas carry
    weight); where the alphas allow it single NaN, +inf and -inf entries, a scan whose every alpha is NaN, a scan whose row
    at the LARGEST finite logp is NaN (the maximum has to be taken again); a log_prior with one -inf"""
    rng = np.random.RandomState(1000 * n_omega + n_alpha + seed)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    ns = int(off[-1])
    H = np.ascontiguousarray(0.5 + rng.rand(ns, n_alpha, n_omega) * np.linspace(1.0, 1e-3, n_omega)[None, None, :])
    logp = -60.0 - rng.rand(ns, n_alpha) * np.where(np.arange(ns) % 2 == 0, 8000.0, 5.0)[:, None]
    if n_alpha >= 2:
        logp[3, rng.randint(n_alpha)] = np.nan
        logp[4, rng.randint(n_alpha)] = np.inf
        logp[5, rng.randint(n_alpha)] = -np.inf
        H[7, int(np.argmax(logp[7])), n_omega // 2] = np.nan
    logp[6] = np.nan
    alpha = np.logspace(3, -2, n_alpha) if n_alpha > 1 else np.array([2.0])
    log_quad = model_scan.log_measure(alpha)
    log_prior = np.log(rng.rand(ns) + 0.1)
    log_prior[8] = -np.inf
    pick = rng.randint(0, n_alpha, size=ns).astype(np.int32)
    pick[9] = -1
    return off, H, logp, log_quad, log_prior, pick


def _ratio(got, ref, name, worst):
    """error / bound of one output; where the bound is 0 the values must be equal; NaN exactly where the reference has it"""
    g, r, b = np.asarray(got[name], dtype=float), ref[name], ref[name + '_bound']
    rn = np.isnan(np.asarray(r, dtype=float))
    assert np.array_equal(np.isnan(g), rn), name
    inf = np.isinf(np.asarray(r, dtype=float))
    assert np.array_equal(g[inf], np.asarray(r, dtype=float)[inf]), name
    ok = ~(rn | inf)
    err = np.abs(np.asarray(g[ok] - r[ok], dtype=float))
    bb = b[ok]
    assert np.all(err[bb == 0] == 0), name
    q = float(np.max(err[bb > 0] / bb[bb > 0])) if np.any(bb > 0) else 0.0
    worst[name] = max(worst.get(name, 0.0), q)
    assert q <= 1.0, (name, q)


@pytest.mark.parametrize('n_alpha', [1, 2, 17, 64, 65])
@pytest.mark.parametrize('n_omega', [1, 63, 64, 65, 500])
def test_kernel_against_longdouble(n_omega, n_alpha):
    off, H, logp, log_quad, log_prior, pick = _case(n_omega, n_alpha)
    rng = np.random.RandomState(n_omega + n_alpha)
    ctx = _ctx(n_omega)
    worst = {}
    try:
        for mode in (0, 1, 2):
            for n_f in (0, 1, 5, 17):
                F = rng.randn(n_f, n_omega) if n_f else None
                log_mix = log_quad if (mode == 0 and n_f == 5) else None              # (average_by_integration)
                kw = dict(log_mix=log_mix, log_prior=log_prior, row_mode=mode, pick=pick if mode == 2 else None, F=F)
                got = ctx.evidence_reduce(off, logp, log_quad, H=H, **kw)
                ref = evidence_reduce_ref(H, off, logp, log_quad, **kw)
                assert np.array_equal(got['kmax'], ref['kmax']) and np.array_equal(got['ngood'], ref['ngood'])
                assert np.array_equal(got['used'], ref['used'])
                for name in ('logZ', 'walpha', 'row', 'fval', 'wmodel', 'mean', 'between', 'fmean', 'fcov'):
                    _ratio(got, ref, name, worst)
                # zeros and NaNs exactly where they belong
                unusable = ~ref['usable']
                assert unusable[6] and (mode != 2 or unusable[9])
                assert np.all(got['logZ'][unusable] == -np.inf) and np.all(got['wmodel'][unusable] == 0)
                assert np.all(np.isnan(got['row'][unusable])) and np.all(np.isnan(got['fval'][unusable]))
                assert np.all(got['walpha'][~np.isfinite(logp)] == 0) and np.all(got['walpha'][6] == 0)
                assert got['wmodel'][8] == 0 and got['ngood'][6] == 0 and got['kmax'][6] == -1
                assert np.all(np.isnan(got['mean'][0])) and np.all(np.isnan(got['between'][0])) and got['used'][0] == 0
                assert np.all(np.isnan(got['fmean'][0])) and np.all(np.isnan(got['fcov'][0]))
                if n_alpha >= 2 and mode == 0:
                    k7 = int(np.argmax(logp[7]))
                    assert got['walpha'][7, k7] == 0 and got['ngood'][7] == n_alpha - 1 and got['kmax'][7] != k7
                    assert np.all(np.isfinite(got['row'][7])) and got['wmodel'][7] > 0
                for gi in (1, 2, 3):
                    s = slice(off[gi], off[gi + 1])
                    if ref['used'][gi] and np.all(np.isfinite(got['wmodel'][s])):
                        assert abs(got['wmodel'][s].sum() - 1.0) <= SIZES[gi] * EPS
                    assert np.array_equal(got['fcov'][gi], got['fcov'][gi].T)
                assert np.all(got['between'][1:] >= 0)
    finally:
        ctx.close()
    print('n_omega %d n_alpha %d: worst error / bound %s' % (n_omega, n_alpha, {k: round(v, 3) for k, v in worst.items()}))


def test_kernel_bits():
    n_omega, n_alpha = 65, 17
    off, H, logp, log_quad, log_prior, pick = _case(n_omega, n_alpha)
    F = np.random.RandomState(3).randn(5, n_omega)
    names = ('logZ', 'kmax', 'ngood', 'walpha', 'row', 'fval', 'wmodel', 'mean', 'between', 'fmean', 'fcov', 'used')
    ctx = _ctx(n_omega)
    try:
        for mode in (0, 1, 2):
            kw = dict(row_mode=mode, F=F)
            pk = pick if mode == 2 else None
            got = ctx.evidence_reduce(off, logp, log_quad, H=H, log_prior=log_prior, pick=pk, **kw)
            again = ctx.evidence_reduce(off, logp, log_quad, H=H, log_prior=log_prior, pick=pk, **kw)
            for k in names:
                assert got[k].tobytes() == again[k].tobytes(), k                          # two calls: the same bits
            # a group alone: the bits it has in the batch
            for gi in (2, 3):
                s = slice(off[gi], off[gi + 1])
                sub = ctx.evidence_reduce([0, SIZES[gi]], logp[s], log_quad, H=H[s], log_prior=log_prior[s],
                                          pick=None if pk is None else pk[s], **kw)
                for k in ('logZ', 'kmax', 'ngood', 'walpha', 'row', 'fval', 'wmodel'):
                    assert sub[k].tobytes() == got[k][s].tobytes(), (k, gi)
                for k in ('mean', 'between', 'fmean', 'fcov', 'used'):
                    assert sub[k][0].tobytes() == got[k][gi].tobytes(), (k, gi)
            # a scan moved to another group keeps its stage-one bits: scan 3 (of the last group) joins group 1
            order = np.array([0, 3, 1, 2, 4, 5, 6, 7, 8, 9])
            moved = ctx.evidence_reduce([0, 0, 2, 4, 10], logp[order], log_quad, H=H[order], log_prior=log_prior[order],
                                        pick=None if pk is None else pk[order], **kw)
            for k in ('logZ', 'kmax', 'ngood', 'walpha', 'row', 'fval'):
                assert moved[k].tobytes() == got[k][order].tobytes(), k
        # identical scans in a group get identical weights
        same = np.array([5, 9, 5, 9, 5])
        tw = ctx.evidence_reduce([0, 5], logp[same], log_quad, H=H[same])
        assert tw['wmodel'][0] == tw['wmodel'][2] == tw['wmodel'][4] and tw['wmodel'][1] == tw['wmodel'][3]
        assert abs(tw['wmodel'].sum() - 1.0) <= 5 * EPS
        # only what is asked for comes back
        part = ctx.evidence_reduce(off, logp, log_quad, H=H, want=('mean',))
        assert sorted(part) == ['kmax', 'logZ', 'mean', 'ngood', 'used', 'wmodel']
    finally:
        ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _raw(ctx, off, na, H, ci, logp, lq, lm, pr, mode, pick, nf, F, outs):
    def p(a):
        if a is None:
            return None
        return a.ctypes.data_as(DP if a.dtype == np.float64 else IP)
    o = outs
    return ctx._lib.mxe_evidence_reduce(ctx._h, len(off) - 1, p(off), na, p(H), p(ci), p(logp), p(lq), p(lm), p(pr), mode, p(pick),
                                        nf, p(F), p(o['logZ']), p(o['kmax']), p(o['ngood']), p(o['walpha']), p(o['row']),
                                        p(o['fval']), p(o['wmodel']), p(o['mean']), p(o['between']), p(o['fmean']), p(o['fcov']),
                                        p(o['used']), None)


ERR_ARG, ERR_STATE = -1, -4                 # (MXE_ERR_ARG, MXE_ERR_STATE of include/maxent_hip.h)


def _prefilled(ns, na, n_omega, ng, nf):
    shapes = dict(logZ=ns, walpha=ns * na, row=ns * n_omega, fval=ns * nf, wmodel=ns, mean=ng * n_omega, between=ng * n_omega,
                  fmean=ng * nf, fcov=ng * nf * nf)
    o = {k: np.full(n, 123.456) for k, n in shapes.items()}
    o.update(kmax=np.full(ns, 77, dtype=np.int32), ngood=np.full(ns, 77, dtype=np.int32), used=np.full(ng, 77, dtype=np.int32))
    return o


def _untouched(o):
    return all(np.all(v == (77 if v.dtype == np.int32 else 123.456)) for v in o.values())


def _with(a, i, v):
    c = a.copy()
    c[i] = v
    return c


def test_refusals_touch_nothing():
    n_omega, na, ns, ng, nf = 9, 4, 3, 2, 2
    rng = np.random.RandomState(0)
    off = np.array([0, 1, 3], dtype=np.int32)
    H, logp = 0.5 + rng.rand(ns, na, n_omega), -rng.rand(ns, na)
    lq, lm, pr = np.zeros(na), np.zeros(na), np.zeros(ns)
    pick = np.zeros(ns, dtype=np.int32)
    F = rng.randn(nf, n_omega)
    fresh, untouched, bad = (lambda: _prefilled(ns, na, n_omega, ng, nf)), _untouched, _with
    ctx = _ctx(n_omega)
    try:
        # H == NULL and nothing was launched (a fresh context): MXE_ERR_STATE
        o = fresh()
        assert _raw(ctx, off, na, None, None, logp, lq, lm, pr, 0, None, nf, F, o) == ERR_STATE and untouched(o)
        with pytest.raises(device.MaxEntDeviceError, match='call order'):
            ctx.evidence_reduce(off, logp, lq)
        big = np.array([0, 70000], dtype=np.int32)
        cases = dict(
            no_group=dict(off=np.array([0], dtype=np.int32)),
            no_alpha=dict(na=0),
            offsets_start=dict(off=np.array([1, 1, 3], dtype=np.int32)),
            offsets_decrease=dict(off=np.array([0, 3, 1], dtype=np.int32)),
            mode_low=dict(mode=-1), mode_high=dict(mode=3),
            mode2_without_pick=dict(mode=2, pick=None),
            pick_too_large=dict(mode=2, pick=np.array([0, na, 0], dtype=np.int32)),
            quad_nan=dict(lq=bad(lq, 1, np.nan)), quad_inf=dict(lq=bad(lq, 0, -np.inf)),
            mix_inf=dict(lm=bad(lm, 3, np.inf)), F_nan=dict(F=bad(F, (1, 2), np.nan)),
            prior_nan=dict(pr=bad(pr, 1, np.nan)), prior_plus_inf=dict(pr=bad(pr, 2, np.inf)),
            too_large=dict(off=big, na=70000))
        for name, ch in cases.items():
            a = dict(off=off, na=na, H=H, ci=None, logp=logp, lq=lq, lm=lm, pr=pr, mode=0, pick=pick, nf=nf, F=F)
            a.update(ch)
            o = fresh()
            rc = _raw(ctx, a['off'], a['na'], a['H'], a['ci'], a['logp'], a['lq'], a['lm'], a['pr'], a['mode'], a['pick'],
                      a['nf'], a['F'], o)
            assert rc == ERR_ARG, (name, rc)
            assert untouched(o), name
        # NaN and infinities in logp are data, a log_prior of -inf is allowed
        o = fresh()
        lp = logp.copy()
        lp[0, 0], lp[1, 1], lp[2, 2] = np.nan, np.inf, -np.inf
        assert _raw(ctx, off, na, H, None, lp, lq, lm, bad(pr, 1, -np.inf), 0, pick, nf, F, o) == 0 and not untouched(o)
        # the wrapper turns the refusal into a ValueError
        with pytest.raises(ValueError, match='refused'):
            ctx.evidence_reduce(off, logp, lq, H=H, row_mode=2)
        with pytest.raises(ValueError):
            ctx.evidence_reduce([0, 2, 1], logp, lq, H=H)
    finally:
        ctx.close()


def test_rows_of_the_last_launch_are_read_where_they_lie():
    """H == NULL: the chains of the last launch, in any order and more than once, give the bits of the same rows handed in"""
    tm, models = _tm()
    K = tm.K
    loop = tm.maxent_loop
    template = loop.make_spec()
    specs = [loop.spec_with_model(template, np.asarray(m.D)) for m in models[:3]]
    from maxent_amd.batch_solver import BatchSolver, directions_to_keep
    from maxent_amd.maxent_loop import solve_elements
    sols, info = solve_elements(K, specs, loop.minimizer, want_logdet=True, want_H=True, select=None)
    solver = BatchSolver.for_kernel(K, (0,), keep=directions_to_keep(K, specs, None))
    ctx = solver.ctxs[0]
    Hs = np.stack([np.asarray(s['H']) for s in sols])
    logp = np.stack([mx.NormalLogProbability().from_logdet(s['logdet'], s['alpha'], s['Q'], 60) for s in sols])
    lq = model_scan.log_measure(specs[0]['alpha'])
    order = np.array([2, 0, 1, 2], dtype=np.int32)
    F = np.ones((1, 60))
    for mode in (0, 1):
        there = ctx.evidence_reduce([0, 1, 4], logp[order], lq, chain_index=order, row_mode=mode, F=F)
        here = ctx.evidence_reduce([0, 1, 4], logp[order], lq, H=Hs[order], row_mode=mode, F=F)
        for k in there:
            assert there[k].tobytes() == here[k].tobytes(), k
    # refusals that need a launch: a chain outside it, an n_alpha that is not its own (3 chains of 12 alphas here)
    off = np.array([0, 1, 3], dtype=np.int32)
    lm, pr = np.zeros(12), np.zeros(3)
    for name, ci, na in (('chain outside', [0, 1, 3], 12), ('chain negative', [0, -1, 1], 12), ('other n_alpha', [0, 1, 2], 11)):
        o = _prefilled(3, 12, 60, 2, 1)
        rc = _raw(ctx, off, na, None, np.array(ci, dtype=np.int32), logp, lq, lm, pr, 0, None, 1, F, o)
        assert rc == ERR_ARG and _untouched(o), (name, rc)
    o = _prefilled(5, 12, 60, 1, 1)                 # (chain_index NULL: scans 0 .. 4, the launch has three chains)
    assert _raw(ctx, np.array([0, 5], dtype=np.int32), 12, None, None, np.zeros((5, 12)), lq, lm, np.zeros(5), 0, None, 1, F, o) == ERR_ARG
    assert _untouched(o)
    with pytest.raises(ValueError, match='refused'):
        ctx.evidence_reduce([0, 1], logp[:1], lq, chain_index=[3])
    plain = ctx.evidence_reduce([0, 3], logp, lq)
    assert plain['row'].tobytes() == ctx.evidence_reduce([0, 3], logp, lq, H=Hs)['row'].tobytes()


# ---- end to end, TauMaxEnt -------------------------------------------------------------------------------------------------------
NAMES = ['flat', 'g0.5', 'g1', 'g2', 'g4', 'g8', 'truth']


def _tm(preblur=None, **kw):
    tau, omega, A, G, Ds = scan_problem()
    tm = mx.TauMaxEnt(**kw)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e3, n_points=12)
    tm.set_G_tau_data(tau, G)
    tm.set_error(1e-3)
    if preblur is not None:
        tm.A_of_H = mx.PreblurA_of_H(b=preblur, omega=tm.omega)
        tm.K = mx.PreblurKernel(K=tm.K, b=preblur)
    delta = np.asarray(tm.omega.delta)
    assert np.array_equal(np.asarray(tm.omega), omega)
    models = [mx.DataDefaultModel(D / delta, tm.omega) for D in Ds]
    return tm, models


@pytest.fixture(scope='module')
def loop_of_runs():
    """the reference: one object per default model, ``D`` set, ``run()``"""
    out = []
    for m in _tm()[1]:
        tm, _ = _tm(probability='normal')
        tm.D = m
        res = tm.run()
        assert np.all(res.converged)
        out.append(res)
    return out


def _host_log_evidence(res):
    x = np.asarray(res.probability, dtype=float) + model_scan.log_measure(res.alpha)
    return float(x.max() + np.log(np.sum(np.exp(x - x.max()))))


@pytest.mark.parametrize('alpha,analyzer', [('bryan', 'BryanAnalyzer'), ('classic', 'ClassicAnalyzer'),
                                            ('LineFitAnalyzer', 'LineFitAnalyzer')])
def test_scan_equals_a_loop_of_runs(loop_of_runs, alpha, analyzer):
    tm, models = _tm()
    D_before = tm.D
    out = tm.default_model_scan(dict(zip(NAMES, models)), alpha=alpha, windows=[(-3.0, 0.0), (0.0, 3.0)],
                                functionals=np.asarray(tm.omega)[None, :])
    assert tm.D is D_before and out['names'] == NAMES
    assert out['info']['launches'] == 1 and out['info']['audit_max'] <= GATE and out['info']['reduce_ms'] > 0
    A_loop = np.stack([np.asarray(r.analyzer_results[analyzer]['A_out']) for r in loop_of_runs])
    dist = rel_l2(out['A_models'], A_loop)
    want_idx = [int(r.analyzer_results['ClassicAnalyzer' if alpha == 'bryan' else analyzer]['alpha_index']) for r in loop_of_runs]
    host = np.array([_host_log_evidence(r) for r in loop_of_runs])
    gap = float(np.max(np.abs(out['log_evidence'] - host)))
    print('%s: largest rel L2 to the loop %.2e, largest |log evidence - host sum| %.2e, audit %.2e; log evidence %s'
          % (alpha, dist.max(), gap, out['info']['audit_max'], np.round(out['log_evidence'], 2)))
    assert np.all(dist < GATE)
    assert out['alpha_index'].tolist() == want_idx
    assert gap <= evidence_gate(host, 12)
    # what the data prefer
    le = out['log_evidence']
    assert out['best'] == 6 and out['log_bayes_factor'][6] == 0 and out['log_bayes_factor'][0] < -10.0
    assert np.argmax(le[1:6]) == 2 and le[3] - le[2] > 1.0 and le[3] - le[4] > 1.0
    assert out['alpha_at_edge'][6] and out['n_good'].tolist() == [12] * 7
    assert abs(out['weight'].sum() - 1.0) <= 7 * EPS and abs(out['n_eff'] - 1.0 / np.sum(out['weight'] ** 2)) < 1e-12
    # the averages are those of the rows that came back
    w = out['weight']
    assert np.all(rel_l2(out['A'], np.dot(w, out['A_models'])) < 1e-12)
    delta = np.asarray(tm.omega.delta)
    for n, (lo, hi) in enumerate([(-3.0, 0.0), (0.0, 3.0)]):
        inside = (np.asarray(tm.omega) >= lo) & (np.asarray(tm.omega) <= hi)
        np.testing.assert_allclose(out['window_models'][:, n], np.sum(out['A_models'][:, inside] * delta[inside], axis=1), rtol=1e-12)
    np.testing.assert_allclose(out['window_weight'], np.dot(w, out['window_models']), rtol=1e-12)
    np.testing.assert_allclose(out['functional_value'], np.dot(w, out['functional_models']), rtol=1e-12, atol=1e-15)
    assert out['functional_cov'].shape == (1, 1) and np.all(out['window_err'] >= 0)


def test_narrow_family_shares_the_weight():
    tm, _ = _tm()
    widths = [1.6, 1.8, 2.0, 2.2, 2.4]
    models = [mx.GaussianDefaultModel(tm.omega, 0.0, w) for w in widths]
    out = tm.default_model_scan(models, prior=np.ones(5))
    w = out['weight']
    print('narrow family: log evidence %s, weights %s' % (np.round(out['log_evidence'], 2), np.round(w, 3)))
    assert np.all(np.diff(w) < 0) and w[0] < 0.6 and out['best'] == 0
    assert np.all(rel_l2(out['A'], np.dot(w, out['A_models'])) < 1e-12)
    second = np.dot(w, (out['A_models'] - out['A'][None, :]) ** 2)
    assert np.linalg.norm(out['A_model_err'] ** 2 - second) <= 1e-9 * np.linalg.norm(second)
    assert 1.0 < out['n_eff'] < 5.0 and out['info']['audit_max'] <= GATE
    # a model that is switched off gets no weight, the others share it in the same proportions
    off = tm.default_model_scan(models, prior=[1, 0, 1, 1, 1], pointwise=False, windows=[(-1.0, 1.0)])
    assert off['weight'][1] == 0 and 'A' not in off and 'A_models' not in off
    np.testing.assert_allclose(off['log_evidence'], out['log_evidence'], rtol=0, atol=evidence_gate(out['log_evidence'], 12))
    # (the weights are ratios of exp(log Z): a difference of the gate in log Z is that relative difference of a weight)
    np.testing.assert_allclose(off['weight'][[0, 2, 3, 4]], w[[0, 2, 3, 4]] / (1 - w[1]), rtol=4 * evidence_gate(out['log_evidence'], 12))
    lean = tm.default_model_scan(models, keep_models=False)
    assert 'A_models' not in lean and np.array_equal(lean['A'], out['A'])


def test_preblur_refers_to_A():
    b = 0.1
    tm, all_models = _tm(preblur=b)
    models = [all_models[0], all_models[3], all_models[6]]
    out = tm.default_model_scan(models, windows=[(-2.0, 2.0)])
    A_loop = []
    for m in models:
        one, _ = _tm(preblur=b, probability='normal')
        one.D = m
        res = one.run()
        A_loop.append(np.asarray(res.analyzer_results['BryanAnalyzer']['A_out']))
    dist = rel_l2(out['A_models'], np.stack(A_loop))
    print('preblur: largest rel L2 to the loop %.2e, audit %.2e' % (dist.max(), out['info']['audit_max']))
    assert np.all(dist < GATE) and out['info']['audit_max'] <= GATE
    w, delta = out['weight'], np.asarray(tm.omega.delta)
    assert np.all(rel_l2(out['A'], np.dot(w, out['A_models'])) < 1e-12)
    inside = (np.asarray(tm.omega) >= -2.0) & (np.asarray(tm.omega) <= 2.0)
    np.testing.assert_allclose(out['window_models'][:, 0], np.sum(out['A_models'][:, inside] * delta[inside], axis=1), rtol=1e-10)
    second = np.dot(w, (out['A_models'] - out['A'][None, :]) ** 2)
    assert np.linalg.norm(out['A_model_err'] ** 2 - second) <= 1e-9 * np.linalg.norm(second)


# ---- element-wise ------------------------------------------------------------------------------------------------------------
def _matrix_job(cls, **kw):
    g = np.load(os.path.join(GOLD, 'elementwise.npz'))
    ew = cls(**kw)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(g['tau'][::5], g['G_tau_noise'][:, :, ::5])
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    ew.set_error(float(g['noise']))
    return ew, g


def test_elementwise_equals_the_single_scans():
    ew, g = _matrix_job(mx.ElementwiseMaxEnt, use_hermiticity=True)
    omega = ew.omega
    models = [mx.FlatDefaultModel(omega), mx.GaussianDefaultModel(omega, 0.0, 2.0), mx.LorentzianDefaultModel(omega, 0.0, 1.0)]
    D_before, Doff_before, res_before = ew.maxent_diagonal.D, ew.maxent_offdiagonal.D, ew.maxent_result
    out = ew.default_model_scan(models, windows=[(-2.0, 2.0)])
    assert ew.maxent_diagonal.D is D_before and ew.maxent_offdiagonal.D is Doff_before and ew.maxent_result is res_before
    assert out['A_models'].shape == (2, 2, 3, 60) and out['log_evidence'].shape == (2, 2, 3) and out['best'].shape == (2, 2)
    assert out['info']['audit_max'] <= GATE and out['info']['n_elements'] == [2, 1]
    for name in ('A', 'A_models', 'A_model_err', 'log_evidence', 'weight', 'window_weight', 'alpha_index', 'alpha_at_edge'):
        assert np.array_equal(out[name][1, 0], out[name][0, 1]), name                  # the hermitian partner is filled
        assert np.all(np.isfinite(out[name])), name
    worst, gap = 0.0, 0.0
    for (i, j) in ((0, 0), (0, 1), (1, 1)):
        tm = mx.TauMaxEnt() if i == j else mx.TauMaxEnt(cost_function='plusminus')
        tm.set_verbosity(mx.VerbosityFlags.Quiet)
        tm.omega, tm.alpha_mesh = omega, mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
        tm.set_G_tau_data(g['tau'][::5], g['G_tau_noise'][i, j, ::5])
        tm.set_error(float(g['noise']))
        one = tm.default_model_scan(models, windows=[(-2.0, 2.0)])
        worst = max(worst, float(np.max(rel_l2(out['A_models'][i, j], one['A_models']))), float(rel_l2(out['A'][i, j], one['A'])))
        gap = max(gap, float(np.max(np.abs(out['log_evidence'][i, j] - one['log_evidence']))))
        assert out['alpha_index'][i, j].tolist() == one['alpha_index'].tolist() and out['best'][i, j] == one['best']
    print('element-wise: largest rel L2 to the single scans %.2e, largest log evidence gap %.2e' % (worst, gap))
    assert worst < GATE and gap <= evidence_gate(out['log_evidence'], 8)
    with pytest.raises(NotImplementedError):
        _matrix_job(mx.PoormanMaxEnt)[0].default_model_scan(models)
    dg, _ = _matrix_job(mx.DiagonalMaxEnt)
    od = dg.default_model_scan(models, alpha='classic', pointwise=False, windows=[(-2.0, 2.0)])
    assert np.all(np.isnan(od['log_evidence'][0, 1])) and np.all(od['alpha_index'][1, 0] == -1) and np.all(np.isfinite(od['weight'][1, 1]))
    np.testing.assert_allclose(od['log_evidence'][0, 0], out['log_evidence'][0, 0], rtol=0,
                               atol=evidence_gate(out['log_evidence'][0, 0], 8))
