"""Posterior error bars on the device (mxe_posterior_var) against the extended-precision truth of
test_posterior_errors_host.py.

Gate: with r = var_truth / prior (the share of the prior variance the data leave) the Woodbury difference the kernel
evaluates loses 1/r; a numpy binary64 prototype of the same formula is off by ~4 eps / r.  So the relative error of every
variance is <= 1e-6 wherever r >= 1e-8 (4 eps / r = 9e-8 there, a factor 10 for another summation order); below that
only 0 <= var <= prior holds, and at most 5 % of the pairs of any test may fall there.  Measured worst figures of each
test are printed (``-s``) and recorded in DESIGN.md section 4m.
"""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_posterior_errors_host import truth_var                 # noqa: E402
import maxent_amd as mx                                          # noqa: E402
from maxent_amd import device, synthetic, posterior, hostprep    # noqa: E402

pytestmark = pytest.mark.gpu

GATE, R_MIN, SHARE = 1e-6, 1e-8, 0.05
AUDIT = 1e-6


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def gate(label, var, var_t, prior_t):
    """the gate of the module docstring on arrays of device variances, true variances and true priors"""
    var, var_t, prior_t = (np.asarray(x, dtype=np.longdouble).ravel() for x in (var, var_t, prior_t))
    assert np.all(np.isfinite(var.astype(float))), label
    r = var_t / prior_t
    inside = r >= R_MIN
    rel = np.abs(var - var_t) / var_t
    worst = float(rel[inside].max()) if inside.any() else 0.0
    print('%s: %d pairs, r in [%.2e, %.2e], worst |dvar|/var %.2e (at r = %.2e), %d pairs below r = %.0e'
          % (label, len(r), float(r.min()), float(r.max()), worst,
             float(r[inside][np.argmax(rel[inside])]) if inside.any() else 0.0, int((~inside).sum()), R_MIN))
    assert worst <= GATE, (label, worst)
    assert np.all(var[~inside] >= 0) and np.all(var[~inside] <= prior_t[~inside] * (1 + 1e-12)), label
    assert (~inside).mean() <= SHARE, (label, float((~inside).mean()))
    assert np.all(var.astype(float) <= prior_t.astype(float) * (1 + 1e-12)), label
    return worst


def weights(H, D, kind):
    return np.asarray(H) if kind == 'normal' else np.sqrt(np.asarray(H) ** 2 + 4.0 * np.asarray(D) ** 2)


def quiet(obj):
    obj.set_verbosity(mx.VerbosityFlags.Quiet)
    return obj


def cfg2(n_alpha=24, sigma=synthetic.SIGMA, **kw):
    tau, omega, K, G = synthetic.single_G(200, 500)
    tm = quiet(mx.TauMaxEnt(**kw))
    tm.omega = omega
    tm.set_G_tau_data(tau, G)
    tm.set_error(sigma)
    tm.alpha_mesh = synthetic.alpha_mesh(n_alpha)
    return tm, omega


def solved(tm):
    res = tm.run()
    assert np.all(res.converged)
    assert tm.last_launch['audit_max'] < AUDIT, tm.last_launch['audit_max']
    return res


WINDOWS = [(-3.0, 0.0), (0.0, 2.0), (4.0, 9.0)]


def test_tau_maxent_cfg2_windows_moment_and_pointwise():
    tm, omega = cfg2()
    res = solved(tm)
    w = np.asarray(omega)
    F = np.stack([np.ones(len(w)), w])                          # norm, first moment
    rows = np.concatenate([posterior.window_rows(w, WINDOWS), F])
    Kk, err, D = np.array(tm.K.K), np.asarray(tm.err), np.asarray(tm.D.D)
    H, alpha = np.asarray(res.H), np.asarray(res.alpha)
    ia0 = int(res.analyzer_results[res.default_analyzer_name]['alpha_index'])
    t = {}
    one = tm.posterior_errors(res, windows=WINDOWS, functionals=F, pointwise=True, timing=t)
    assert t['reused_contexts'] == 1, t                   # (the solver's context still holds this element staged)
    assert int(one['alpha_index']) == ia0 and one['window_err'].shape == (3,) and one['A_err'].shape == (len(w),)
    vt, pt = truth_var(Kk, err, H[ia0], alpha[ia0], np.concatenate([rows, np.eye(len(w))]))
    got = np.concatenate([one['window_err'], one['functional_err']]) ** 2
    gate('cfg2 default alpha, integrated', got, vt[:5], pt[:5])
    gate('cfg2 default alpha, pointwise', (one['A_err'] * omega.delta) ** 2, vt[5:], pt[5:])
    np.testing.assert_allclose(one['window_weight'], rows[:3] @ H[ia0], rtol=1e-13)
    np.testing.assert_allclose(one['functional_value'], F @ H[ia0], rtol=1e-13)
    np.testing.assert_allclose(one['prior_err'] ** 2, pt[:5].astype(float), rtol=1e-12)
    np.testing.assert_allclose((one['A_prior_err'] * omega.delta) ** 2, pt[5:].astype(float), rtol=1e-12)
    picks = [0, 5, 11, 17, 23]
    many = tm.posterior_errors(res, alpha=picks, windows=WINDOWS, functionals=F, pointwise=True)
    assert many['window_err'].shape == (5, 3) and list(many['alpha_index']) == picks and many['A_err'].shape == (5, len(w))
    vs, ps = zip(*[truth_var(Kk, err, H[i], alpha[i], np.concatenate([rows, np.eye(len(w))])) for i in picks])
    vs, ps = np.array(vs), np.array(ps)
    gate('cfg2 five alphas, integrated', np.concatenate([many['window_err'], many['functional_err']], axis=1) ** 2, vs[:, :5], ps[:, :5])
    gate('cfg2 five alphas, pointwise', (many['A_err'] * omega.delta) ** 2, vs[:, 5:], ps[:, 5:])
    # (atol: in the tails H underflows at the large alphas and w / alpha is a denormal number with a few bits)
    np.testing.assert_allclose((many['A_prior_err'] * omega.delta) ** 2, ps[:, 5:].astype(float), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(many['A'], H[picks] / omega.delta, rtol=1e-14)
    # an object that has not run stages a context of its own and gives the same bits
    tm2, _ = cfg2()
    t2 = {}
    fresh = tm2.posterior_errors(pickle.loads(pickle.dumps(res.data)), alpha=picks, windows=WINDOWS, functionals=F, pointwise=True, timing=t2)
    assert t2['reused_contexts'] == 0
    for k in ('window_err', 'functional_err', 'A_err', 'prior_err'):
        assert np.array_equal(fresh[k], many[k]), k
    # a row of H that is not finite: NaN there, reported, the others untouched
    broken = pickle.loads(pickle.dumps(res.data))
    Hb = np.array(broken.H)
    Hb[11, 7] = np.nan
    broken._saved['H'] = Hb
    bad = tm.posterior_errors(broken, alpha=picks, windows=WINDOWS, functionals=F)
    assert bad['info']['nan_rows'] == [11] and np.all(np.isnan(bad['window_err'][2])) and np.all(np.isnan(bad['functional_err'][2]))
    keep = [0, 1, 3, 4]
    assert np.array_equal(bad['window_err'][keep], many['window_err'][keep])
    assert np.array_equal(bad['functional_err'][keep], many['functional_err'][keep])


def matrix_job(n=3, n_tau=120, n_omega=300, n_alpha=16):
    tau, omega, K, Gmat, _ = synthetic.matrix_G(n, n_tau, n_omega)
    ew = quiet(mx.ElementwiseMaxEnt(use_hermiticity=False))
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.alpha_mesh = synthetic.alpha_mesh(n_alpha)
    return ew, omega, n_tau


@pytest.mark.parametrize('errors', ['scalar', 'per_tau', 'cov'])
def test_elementwise_3x3_every_element_against_its_own_truth(errors):
    ew, omega, n_tau = matrix_job()
    rng = np.random.RandomState(11)
    if errors == 'scalar':
        ew.set_error(synthetic.SIGMA)
    elif errors == 'per_tau':
        ew.set_error(synthetic.SIGMA * (1.0 + rng.rand(n_tau)))
    else:
        # correlated noise: neighbouring tau points share 30 % of their variance over a correlation time of one tau unit
        tau = np.linspace(0, synthetic.BETA, n_tau)
        ew.set_cov(synthetic.SIGMA ** 2 * (np.eye(n_tau) + 0.3 * np.exp(-np.abs(tau[:, None] - tau[None, :]))))
    res = ew.run()
    assert np.all(res.converged)
    assert ew.last_launches and all(info['audit_max'] < AUDIT for info in ew.last_launches)
    w = np.asarray(omega)
    windows = [(-2.0, 0.0), (0.0, 2.5)]
    out = ew.posterior_errors(res, windows=windows, functionals=np.ones((1, len(w))))
    assert out['window_err'].shape == (3, 3, 2) and out['functional_err'].shape == (3, 3, 1)
    rows = np.concatenate([posterior.window_rows(w, windows), np.ones((1, len(w)))])
    got, vts, pts = [], [], []
    for i in range(3):
        for j in range(3):
            worker = ew.maxent_diagonal if i == j else ew.maxent_offdiagonal
            ew._load_element(worker, (i, j), True)
            ia = int(out['alpha_index'][i, j])
            assert ia == int(res.analyzer_results[i][j][res.default_analyzer_name]['alpha_index'])
            H = np.asarray(res.H[i][j][ia])
            wgt = weights(H, worker.D.D, 'normal' if i == j else 'plusminus')
            vt, pt = truth_var(np.array(worker.K.K), np.asarray(worker.err), wgt, float(np.asarray(res.alpha)[ia]), rows)
            got.append(np.concatenate([out['window_err'][i, j], out['functional_err'][i, j]]) ** 2)
            vts.append(vt)
            pts.append(pt)
            np.testing.assert_allclose(out['window_weight'][i, j], rows[:2] @ H, rtol=1e-12, atol=1e-15)
    gate('3x3 %s' % errors, np.array(got), np.array(vts), np.array(pts))


def test_preblur_windows_and_pointwise_on_A():
    tm, omega = cfg2(n_alpha=12, cost_function='plusminus')
    b = 0.1
    tm.A_of_H = mx.PreblurA_of_H(b=b, omega=tm.omega)
    tm.K = mx.PreblurKernel(K=tm.K, b=b)
    res = solved(tm)
    w, delta = np.asarray(omega), np.asarray(omega.delta)
    out = tm.posterior_errors(res, alpha=6, windows=WINDOWS[:2], pointwise=True)
    B = np.asarray(tm.A_of_H.matrix())
    rows = np.concatenate([(posterior.window_rows(w, WINDOWS[:2]) * delta) @ B, B])
    H = np.asarray(res.H[6])
    vt, pt = truth_var(np.array(tm.K.K), np.asarray(tm.err), weights(H, tm.D.D, 'plusminus'), float(res.alpha[6]), rows)
    gate('preblur', np.concatenate([out['window_err'], out['A_err']]) ** 2, vt, pt)
    np.testing.assert_allclose(out['window_weight'], (posterior.window_rows(w, WINDOWS[:2]) * delta) @ np.asarray(res.A[6]), rtol=1e-10)
    np.testing.assert_allclose(out['A'], np.asarray(res.A[6]), rtol=1e-9, atol=1e-13)


def test_matsubara_and_symmetric_bosonic_windows():
    beta = 40.0
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=200)
    w = np.asarray(omega)
    A = synthetic.two_gaussian_spectrum(w)
    wn = (2 * np.arange(40) + 1) * np.pi / beta
    rng = np.random.RandomState(2)
    G_iw = ((A * omega.delta)[None, :] / (1j * wn[:, None] - w[None, :])).sum(axis=1)
    G_iw = G_iw + 1e-4 * (rng.randn(40) + 1j * rng.randn(40))
    tm = quiet(mx.TauMaxEnt())
    tm.omega = omega
    tm.set_G_iw_data(wn, G_iw)
    tm.set_error(1e-4)
    tm.alpha_mesh = mx.LogAlphaMesh(1e-2, 1e4, 16)
    res = solved(tm)
    windows = [(-3.0, 0.0), (0.0, 2.0)]
    out = tm.posterior_errors(res, alpha=[3, 12], windows=windows)
    rows = posterior.window_rows(w, windows)
    vs, ps = zip(*[truth_var(np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H[i]), float(res.alpha[i]), rows) for i in (3, 12)])
    gate('matsubara', out['window_err'] ** 2, np.array(vs), np.array(ps))
    # bosonic, half axis
    wh = mx.DataOmegaMesh(np.linspace(0.0, 8.0, 120))
    x = np.asarray(wh)
    Ab = np.exp(-(x - 2.0) ** 2 / 0.5)
    tau = np.linspace(0.0, beta, 60)
    Kb = mx.BosonicTauKernel(tau, wh, beta=beta, symmetric=True)
    chi = np.array(Kb.K_delta) @ Ab
    tb = quiet(mx.TauMaxEnt())
    tb.omega = wh
    tb.set_chi_tau_data(tau, chi + 1e-4 * rng.randn(60), beta=beta, symmetric=True)
    tb.set_error(1e-4)
    tb.alpha_mesh = mx.LogAlphaMesh(1e-2, 1e4, 16)
    rb = solved(tb)
    windows = [(0.0, 1.5), (1.5, 3.0)]
    ob = tb.posterior_errors(rb, alpha=8, windows=windows)
    vt, pt = truth_var(np.array(tb.K.K), np.asarray(tb.err), np.asarray(rb.H[8]), float(rb.alpha[8]), posterior.window_rows(x, windows))
    gate('bosonic symmetric', ob['window_err'] ** 2, vt, pt)


def test_all_alphas_equal_single_calls_bit_for_bit_and_unpickled_rows_equal_the_last_launch():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(4, 120, 300)
    ew = quiet(mx.ElementwiseMaxEnt(use_hermiticity=False))
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.alpha_mesh = synthetic.alpha_mesh(40)
    ew.set_error(synthetic.SIGMA)
    res = ew.run()
    assert np.all(res.converged) and all(info['audit_max'] < AUDIT for info in ew.last_launches)
    windows = [(-2.0, 0.0), (0.0, 2.5)]
    every = ew.posterior_errors(res, alpha='all', windows=windows)
    again = ew.posterior_errors(res, alpha='all', windows=windows)
    assert every['window_err'].shape == (4, 4, 40, 2)
    assert np.array_equal(every['window_err'], again['window_err']) and np.array_equal(every['prior_err'], again['prior_err'])
    for ia in (0, 7, 20, 39):
        one = ew.posterior_errors(res, alpha=ia, windows=windows)
        assert np.array_equal(one['window_err'], every['window_err'][:, :, ia]), ia
    thawed = pickle.loads(pickle.dumps(res.data))
    ew2 = ew.posterior_errors(thawed, alpha='all', windows=windows)
    assert np.array_equal(ew2['window_err'], every['window_err'])
    # DeviceContext: the rows of the last launch where they lie against the same rows handed in (after a pickle)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    alphas = np.array(synthetic.alpha_mesh(10)) * 120
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(120))
    kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
    ctx.set_elements([ds] * 2, [Gmat[0, 0], Gmat[0, 1]], np.tile(D, (2, 1)), kinds)
    v0 = np.stack([hostprep.initial_v(K.V, D, omega.delta, k) for k in kinds])
    sol = ctx.solve_chains(np.arange(2), alphas, v0)
    assert sol['converged'].all() and ctx.audit()['corr'].max() < AUDIT
    F = posterior.window_rows(np.asarray(omega), windows)
    pick = np.array([13, 2, 19, 0])                               # any subset, any order
    el, al = pick // 10, alphas[pick % 10]
    there = ctx.posterior_var(el, al, problem_index=pick, F=F, want_diag=True)
    H = pickle.loads(pickle.dumps(np.asarray(sol['H']).reshape(20, -1)[pick]))
    given = ctx.posterior_var(el, al, H=H, F=F, want_diag=True)
    # Q = eta chi2 / 2 - alpha S with eta != 1: Gamma(eta, alpha) = Gamma(1, alpha / eta) / eta, against the truth's own eta
    scaled = ctx.posterior_var(el, al, H=H, F=F, chi2_factor=2.5)
    ctx.close()
    err = synthetic.SIGMA * np.ones(120)
    vs, ps = zip(*[truth_var(np.array(K.K), err, weights(H[n], D, 'normal' if el[n] == 0 else 'plusminus'), al[n], F, eta=2.5)
                   for n in range(len(pick))])
    gate('chi2_factor 2.5', scaled['var'], np.array(vs), np.array(ps))
    np.testing.assert_allclose(scaled['prior'], np.array(ps).astype(float), rtol=1e-12)
    for k in ('var', 'prior', 'diag'):
        assert np.array_equal(there[k], given[k]), k


def test_bryan_mixture_against_the_formula():
    tm, omega = cfg2(n_alpha=16, probability='normal')
    res = solved(tm)
    w = np.asarray(omega)
    windows = WINDOWS[:2]
    rows = posterior.window_rows(w, windows)
    out = tm.posterior_errors(res, alpha='bryan', windows=windows)
    logp = np.asarray(res.probability, dtype=float)
    assert np.all(np.isfinite(logp))
    p = np.exp(logp - logp.max())
    p /= p.sum()
    H, alpha = np.asarray(res.H), np.asarray(res.alpha)
    vs, ps = zip(*[truth_var(np.array(tm.K.K), np.asarray(tm.err), H[i], alpha[i], rows) for i in range(len(alpha))])
    vs = np.array(vs)
    x = (H @ rows.T).astype(np.longdouble)
    mean = (p[:, None] * x).sum(axis=0)
    var = (p[:, None] * (vs + (x - mean) ** 2)).sum(axis=0)
    np.testing.assert_allclose(out['window_weight'], mean.astype(float), rtol=1e-12)
    rel = np.abs(out['window_err'] ** 2 - var) / var
    print('bryan: worst |dvar|/var %.2e' % float(rel.max()))
    assert float(rel.max()) <= GATE
    tm2, _ = cfg2(n_alpha=6)
    with pytest.raises(ValueError, match='Probability not calculated. Cannot use BryanAnalyzer.'):
        tm2.posterior_errors(solved(tm2), alpha='bryan', windows=windows)


def test_device_context_128_row_build_and_a_nan_row(monkeypatch):
    monkeypatch.setenv('MAXENT_AMD_ALL_DIRECTIONS', '1')
    n_tau, n_omega = 1000, 300
    tau, omega, K, G = synthetic.single_G(n_tau, n_omega)
    K.reduce_singular_space(1e-14)
    assert len(K.S) > 64
    D = synthetic.flat_D(omega)
    err = synthetic.SIGMA * np.ones(n_tau)
    alphas = np.array(mx.LogAlphaMesh(1e-1, 1e3, 6)) * n_tau
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(err)
    ctx.set_elements([ds], [G], D[np.newaxis, :], [device.ENTROPY_NORMAL])
    sol = ctx.solve_chains([0], alphas, hostprep.initial_v(K.V, D, omega.delta, device.ENTROPY_NORMAL)[np.newaxis, :])
    assert sol['converged'].all() and ctx.audit()['corr'].max() < AUDIT
    w = np.asarray(omega)
    F = np.concatenate([posterior.window_rows(w, [(-3.0, 0.0), (0.0, 2.0)]), np.ones((1, n_omega)), w[None, :]])
    H = np.array(sol['H'][0])
    good = ctx.posterior_var(np.zeros(6, dtype=int), alphas, H=H, F=F, want_diag=True)
    vs, ps = zip(*[truth_var(np.array(K.K), err, H[i], alphas[i], np.concatenate([F, np.eye(n_omega)])) for i in (0, 5)])
    gate('128-row build', np.concatenate([good['var'][[0, 5]], good['diag'][[0, 5]]], axis=1), np.array(vs), np.array(ps))
    Hn = H.copy()
    Hn[2, 17] = np.nan
    mixed = ctx.posterior_var(np.zeros(6, dtype=int), alphas, H=Hn, F=F, want_diag=True)     # (returns: MXE_OK)
    ctx.close()
    keep = np.array([0, 1, 3, 4, 5])
    for k in ('var', 'prior', 'diag'):
        assert np.all(np.isnan(mixed[k][2])), k
        assert np.array_equal(mixed[k][keep], good[k][keep]), k


def test_sanity_without_a_truth():
    outs = {}
    for sigma in (synthetic.SIGMA, 0.5 * synthetic.SIGMA):
        tm, omega = cfg2(n_alpha=12, sigma=sigma)
        res = solved(tm)
        # the same alpha~ and the same H for both error bars: the data term alone changes
        H = np.asarray(outs['H']) if 'H' in outs else np.asarray(res.H)
        outs.setdefault('H', H)
        spec = tm.maxent_loop.make_spec()
        var, prior, _ = posterior.device_variances(tm.K, [spec], [H], [np.asarray(res.alpha)],
                                                   posterior.window_rows(np.asarray(omega), WINDOWS), False)
        outs[sigma] = (var[0], prior[0])
        assert np.all(var[0] <= prior[0]) and np.all(var[0] >= 0)
    assert np.all(outs[0.5 * synthetic.SIGMA][0] <= outs[synthetic.SIGMA][0])
    # sum_i Gamma_ii alpha / w_i = n_omega - sum_k lambda_k / (alpha + lambda_k), lambda the eigenvalues of c W c
    tau, om, K, G = synthetic.single_G(200, 500)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(om)
    err = synthetic.SIGMA * np.ones(200)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(err)
    ctx.set_elements([ds], [G], D[np.newaxis, :], [device.ENTROPY_NORMAL])
    H = outs['H'][[2, 9]]
    alpha = np.array([5.0, 5.0e3])
    got = ctx.posterior_var([0, 0], alpha, H=H, want_diag=True)
    ev = ctx.eval_batch([0, 0], alpha, H, input_is_H=True, want=('W',))
    ctx.close()
    C = (K.U * K.S[None, :]) / err[:, None]
    M = C.T @ C
    for n in range(2):
        # the eigenvalues of M W are those of c W c (M = Q c^2 Q^T in the whitened basis)
        lam = np.linalg.eigvalsh(_sym_product(M, ev['W'][n]))
        lhs = float(np.sum(got['diag'][n] * alpha[n] / H[n]))
        rhs = len(H[n]) - float(np.sum(lam / (alpha[n] + lam)))
        print('trace identity: %.12g vs %.12g' % (lhs, rhs))
        assert abs(lhs - rhs) <= 1e-8 * abs(rhs)


def _sym_product(M, W):
    """W^1/2 M W^1/2: symmetric, with the eigenvalues of M W"""
    lw, Qw = np.linalg.eigh(W)
    R = (Qw * np.sqrt(np.clip(lw, 0.0, None))) @ Qw.T
    return R @ M @ R


def test_bryan_by_integration_with_pointwise_errors():
    tm, omega = cfg2(n_alpha=8, probability='normal')
    tm.analyzers = [mx.LineFitAnalyzer(), mx.BryanAnalyzer(average_by_integration=True)]
    res = solved(tm)
    w = np.asarray(omega)
    rows = np.concatenate([posterior.window_rows(w, WINDOWS[:2]), np.eye(len(w))])
    out = tm.posterior_errors(res, alpha='bryan', windows=WINDOWS[:2], pointwise=True)
    logp, alpha, H = np.asarray(res.probability, dtype=float), np.asarray(res.alpha), np.asarray(res.H)
    from maxent_amd.analyzers import get_delta
    p = np.exp(logp - logp.max())
    p = p / np.trapezoid(p, alpha) * get_delta(alpha)
    np.testing.assert_allclose(out['weights'], p, rtol=1e-14)
    vs, ps = zip(*[truth_var(np.array(tm.K.K), np.asarray(tm.err), H[i], alpha[i], rows) for i in range(len(alpha))])
    x = (H @ rows.T).astype(np.longdouble)
    x[:, 2:] = (H / omega.delta).astype(np.longdouble)                 # A, not H
    vs = np.array(vs)
    vs[:, 2:] /= np.asarray(omega.delta, dtype=np.longdouble) ** 2
    mean = (p[:, None] * x).sum(axis=0)
    var = (p[:, None] * (vs + (x - mean) ** 2)).sum(axis=0)
    got = np.concatenate([out['window_err'], out['A_err']]) ** 2
    rel = np.abs(got - var) / var
    print('bryan by integration, windows + pointwise: worst |dvar|/var %.2e' % float(rel.max()))
    assert float(rel.max()) <= GATE
    np.testing.assert_allclose(out['A'], mean[2:].astype(float), rtol=1e-12)


def complex_job(cls=None, **kw):
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 120, 300)
    Gc = Gmat.astype(complex)
    Gc[0, 1] = Gmat[0, 1] + 0.5j * Gmat[0, 0]
    Gc[1, 0] = np.conj(Gc[0, 1])
    ew = quiet((cls or mx.ElementwiseMaxEnt)(**kw))
    ew.set_G_tau_data(tau, Gc)
    ew.omega = omega
    ew.alpha_mesh = synthetic.alpha_mesh(16)
    ew.set_error(synthetic.SIGMA)
    return ew, omega


def test_complex_hermitian_elements_and_their_partners():
    """the default configuration (use_hermiticity=True) with use_complex=True: real and imaginary part of G_01 have errors of
    their own, G_10 is filled from its partner (the imaginary part's values with the other sign)"""
    ew, omega = complex_job(use_complex=True)
    res = ew.run()
    assert np.all(np.asarray(res.converged)[0, 1] == 1) and all(info['audit_max'] < AUDIT for info in ew.last_launches)
    w = np.asarray(omega)
    windows = [(-2.0, 0.0), (0.0, 2.5)]
    rows = posterior.window_rows(w, windows)
    out = ew.posterior_errors(res, alpha=9, windows=windows)
    assert out['window_err'].shape == (2, 2, 2, 2)
    got, vts, pts = [], [], []
    for key, re in (((0, 0), True), ((1, 1), True), ((0, 1), True), ((0, 1), False)):
        worker = ew.maxent_diagonal if key[0] == key[1] else ew.maxent_offdiagonal
        ew._load_element(worker, key, re)
        c = 0 if re else 1
        H = np.asarray(res.H[key[0]][key[1]][c][9])
        wgt = weights(H, worker.D.D, 'normal' if key[0] == key[1] else 'plusminus')
        vt, pt = truth_var(np.array(worker.K.K), np.asarray(worker.err), wgt, float(np.asarray(res.alpha)[9]), rows)
        got.append(out['window_err'][key + (c,)] ** 2)
        vts.append(vt)
        pts.append(pt)
        np.testing.assert_allclose(out['window_weight'][key + (c,)], rows @ H, rtol=1e-12, atol=1e-15)
    gate('2x2 complex hermitian', np.array(got), np.array(vts), np.array(pts))
    assert np.array_equal(out['window_err'][1, 0], out['window_err'][0, 1])
    assert np.array_equal(out['window_weight'][1, 0, 0], out['window_weight'][0, 1, 0])
    assert np.array_equal(out['window_weight'][1, 0, 1], -out['window_weight'][0, 1, 1])
    assert np.all(np.isnan(out['window_err'][0, 0, 1])) and np.all(np.isnan(out['window_err'][1, 1, 1]))   # (no imaginary diagonal)


def test_poorman_offdiagonal_with_its_own_default_model():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 120, 300)
    pm = quiet(mx.PoormanMaxEnt())
    pm.set_G_tau_data(tau, Gmat)
    pm.omega = omega
    pm.alpha_mesh = synthetic.alpha_mesh(16)
    pm.set_error(synthetic.SIGMA)
    res = pm.run()
    assert np.all(np.asarray(res.converged)[0, 1] == 1) and all(info['audit_max'] < AUDIT for info in pm.last_launches)
    w = np.asarray(omega)
    windows = [(-2.0, 0.0), (0.0, 2.5)]
    rows = posterior.window_rows(w, windows)
    out = pm.posterior_errors(res, alpha=9, windows=windows)
    ar = res.analyzer_results
    model = mx.DataDefaultModel(np.sqrt(np.asarray(ar[0][0]['LineFitAnalyzer']['A_out']) *
                                        np.asarray(ar[1][1]['LineFitAnalyzer']['A_out'])) + 1e-6, omega)
    Dpm = np.asarray(model.D)                     # (what run_offdiagonal hands to the solver for this element)
    np.testing.assert_allclose(pm.maxent_offdiagonal.D.D, Dpm, rtol=1e-14)
    H = np.asarray(res.H[0][1][9])
    vt, pt = truth_var(np.array(pm.maxent_offdiagonal.K.K), synthetic.SIGMA * np.ones(120), weights(H, Dpm, 'plusminus'),
                       float(np.asarray(res.alpha)[9]), rows)
    gate('poorman (0, 1)', out['window_err'][0, 1] ** 2, vt, pt)
    assert np.array_equal(out['window_err'][1, 0], out['window_err'][0, 1])
    dg = quiet(mx.DiagonalMaxEnt())
    dg.set_G_tau_data(tau, Gmat)
    dg.omega = omega
    dg.alpha_mesh = synthetic.alpha_mesh(16)
    dg.set_error(synthetic.SIGMA)
    rd = dg.run()
    od = dg.posterior_errors(rd, alpha=9, windows=windows)
    assert np.all(np.isfinite(od['window_err'][[0, 1], [0, 1]])) and np.all(np.isnan(od['window_err'][0, 1]))
    Hd = np.asarray(rd.H[0][0][9])
    vt, pt = truth_var(np.array(dg.maxent_diagonal.K.K), synthetic.SIGMA * np.ones(120), Hd, float(np.asarray(rd.alpha)[9]), rows)
    gate('diagonal (0, 0)', od['window_err'][0, 0] ** 2, vt, pt)
