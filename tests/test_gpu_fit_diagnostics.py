"""Fit diagnostics on the device (mxe_fit_diagnostics) against the extended-precision truth of
test_fit_diagnostics_host.py, evaluated at the device's own H rows.

Gate, for every (problem, data point) pair and none left out (1e-6 is the project's parity gate):

    |h - h_t|  <= 1e-6 h_t + 1e-12
    |N_g - N_t| <= 1e-6 N_t + 1e-12 n_rows
    max |r - r_t| <= 1e-6 rms(r_t)

The absolute terms cover the cancellation in |U^_i|^2 - a |L^-1 U^_i|^2: a few eps of |U^_i|^2 <= 1, times the factor 10
for another summation order that the posterior gate allows.  Every test also asserts sum_i h_i = n_good to 1e-13,
chi2 = result.chi2 to 1e-10 and 0 <= h_i <= |U^_i|^2 (1 + 1e-12).  The worst figures of each test are printed (``-s``)
and recorded in DESIGN.md section 4s.
"""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fit_diagnostics_host import truth_hat                  # noqa: E402
import maxent_amd as mx                                          # noqa: E402
from maxent_amd import device, synthetic, posterior, hostprep, diagnostics    # noqa: E402

pytestmark = pytest.mark.gpu

GATE = 1e-6
AUDIT = 1e-6


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def weights(H, D, kind):
    return np.asarray(H) if kind == 'normal' else np.sqrt(np.asarray(H) ** 2 + 4.0 * np.asarray(D) ** 2)


def quiet(obj):
    obj.set_verbosity(mx.VerbosityFlags.Quiet)
    return obj


def row_norms(U, err):
    """|U^_i|^2: the diagonal of the projector on the column space of Sigma^-1/2 K = diag(1/err) U S V^T"""
    U = np.asarray(U, dtype=float)
    Q = np.linalg.qr(U / (np.asarray(err, dtype=float) * np.ones(U.shape[0]))[:, None])[0]
    return np.sum(Q * Q, axis=1)


def gate(label, got, truths, u2, chi2_solver=None):
    """the gate of the module docstring: ``got`` the device's dict with an alpha axis in front, ``truths`` one
    (h_t, N_t, r_t) per alpha, ``u2`` the squared row norms of U^; ``chi2_solver``: the solver's chi2 of these alphas"""
    h, ng, r, chi2 = (np.asarray(got[k], dtype=float) for k in ('leverage', 'n_good', 'residual', 'chi2'))
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(r)) and np.all(np.isfinite(ng)), label
    n_rows = h.shape[1]
    worst = [0.0, 0.0, 0.0]
    for n, (ht, nt, rt) in enumerate(truths):
        assert ht.shape == (n_rows,), (label, ht.shape, n_rows)
        dh = np.abs(h[n].astype(np.longdouble) - ht)
        worst[0] = max(worst[0], float(np.max(dh / ht)))
        assert np.all(dh <= GATE * ht + 1e-12), (label, n, float(np.max(dh - GATE * ht)))
        dn = abs(np.longdouble(ng[n]) - nt)
        worst[1] = max(worst[1], float(dn / nt))
        assert dn <= GATE * nt + 1e-12 * n_rows, (label, n, float(dn))
        rms = float(np.sqrt(np.mean(rt.astype(float) ** 2)))
        dr = float(np.max(np.abs(r[n].astype(np.longdouble) - rt)))
        worst[2] = max(worst[2], dr / rms)
        assert dr <= GATE * rms, (label, n, dr, rms)
        assert abs(float(np.sum(h[n])) - ng[n]) <= 1e-13 * ng[n], (label, n)
        assert abs(float(np.sum(r[n] ** 2)) - chi2[n]) <= 1e-13 * chi2[n], (label, n)
        assert np.all(h[n] >= 0) and np.all(h[n] <= u2 * (1 + 1e-12)), (label, n)
        assert ng[n] <= n_rows
    if chi2_solver is not None:
        np.testing.assert_allclose(chi2, np.asarray(chi2_solver, dtype=float), rtol=1e-10, err_msg=label)
    print('%s: %d alphas x %d rows, N_g in [%.3f, %.3f], worst |dh|/h %.2e, |dN|/N %.2e, max|dr|/rms %.2e'
          % (label, len(truths), n_rows, float(ng.min()), float(ng.max()), worst[0], worst[1], worst[2]))


def truths_of(Kk, err, H, alpha, G, D=None, kind='normal', picks=None, eta=1.0):
    picks = range(len(alpha)) if picks is None else picks
    return [truth_hat(Kk, err, weights(H[i], D, kind), alpha[i], H[i], G, eta=eta) for i in picks]


def solved(tm):
    res = tm.run()
    assert np.all(res.converged)
    assert tm.last_launch['audit_max'] < AUDIT, tm.last_launch['audit_max']
    return res


def small_job(n_alpha=10, seed=1234, **kw):
    """n_tau = 40, n_omega = 64, an error bar per tau point: n_s = 35 (a ragged 16-tile), 40 rows (a short last block of
    16 data points), a whitened basis that carries a rotation"""
    tau, omega, K, G = synthetic.single_G(40, 64, seed=seed)
    tm = quiet(mx.TauMaxEnt(**kw))
    tm.omega = omega
    tm.set_G_tau_data(tau, G)
    tm.set_error(synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(40)))
    tm.alpha_mesh = synthetic.alpha_mesh(n_alpha)
    return tm, tau, omega


def test_ragged_tile_short_block_and_rotated_basis_every_alpha():
    tm, tau, omega = small_job()
    res = solved(tm)
    n_s = len(tm.K.S)
    assert 32 < n_s < 48 and n_s % 16 != 0, n_s
    out = tm.fit_diagnostics(res)
    spec = tm.maxent_loop.make_spec()
    Kk, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H), np.asarray(res.alpha)
    assert out['residual'].shape == (10, 40) and out['leverage'].shape == (10, 40) and out['n_good'].shape == (10,)
    assert list(out['alpha_index']) == list(range(10)) and np.array_equal(out['alpha'], alpha)
    gate('40 x 64, per-tau errors', out, truths_of(Kk, err, H, alpha, spec['G']), row_norms(tm.K.U, err), res.chi2)
    assert np.all(np.diff(out['n_good']) * np.diff(alpha) < 0)        # (more good data at smaller alpha)
    np.testing.assert_allclose(out['studentized'], diagnostics.studentized(out['residual'], out['leverage']), rtol=0, atol=0)
    np.testing.assert_allclose(out['autocorr'], diagnostics.autocorr(out['residual']), rtol=0, atol=0)
    np.testing.assert_allclose(out['gcv'], 40 * out['chi2'] / (40 - out['n_good']) ** 2, rtol=1e-14)
    np.testing.assert_allclose(out['good_data_ratio'], -2 * alpha * np.asarray(res.S) / out['n_good'], rtol=1e-14)
    assert out['info']['nan_rows'] == []


def test_cfg2_shapes_index_rules_five_alphas_and_a_fresh_object():
    tau, omega, K, G = synthetic.single_G(200, 500)

    def make():
        tm = quiet(mx.TauMaxEnt())
        tm.omega = omega
        tm.set_G_tau_data(tau, G)
        tm.set_error(synthetic.SIGMA)
        tm.alpha_mesh = synthetic.alpha_mesh(16)
        return tm
    tm = make()
    res = solved(tm)
    t = {}
    out = tm.fit_diagnostics(res, alpha='all', timing=t)
    assert t['reused_contexts'] == 1, t                   # (the solver's context still holds this element staged)
    for name, shape in (('n_good', (16,)), ('chi2', (16,)), ('residual', (16, 200)), ('leverage', (16, 200)),
                        ('studentized', (16, 200)), ('autocorr', (16,)), ('gcv', (16,)), ('good_data_ratio', (16,)),
                        ('A_gcv', (500,)), ('A_classic', (500,)), ('alpha', (16,)), ('alpha_index', (16,))):
        assert np.shape(out[name]) == shape, (name, np.shape(out[name]))
    Kk, err, H, alpha = np.array(tm.K.K), synthetic.SIGMA * np.ones(200), np.asarray(res.H), np.asarray(res.alpha)
    picks = [0, 4, 8, 12, 15]
    truths = truths_of(Kk, err, H, alpha, G, picks=picks)
    five = tm.fit_diagnostics(res, alpha=picks)
    gate('cfg2, five alphas', five, truths, row_norms(tm.K.U, err), np.asarray(res.chi2)[picks])
    for k in ('n_good', 'chi2', 'residual', 'leverage'):
        assert np.array_equal(five[k], out[k][picks]), k
    # the index rules on the truth of all 16 alphas: r_t as it is, N_t = sum s^2 / (s^2 + a) from the singular values s of
    # Y (binary64: a singular value is off by eps s_max at most, and one far below sqrt a adds nothing), checked against
    # the extended-precision N_t at the five alphas above
    N_t, chi2_t = np.empty(16), np.empty(16)
    for i in range(16):
        Y = np.sqrt(H[i])[:, None] * (Kk / err[:, None]).T
        lam = np.linalg.svd(Y, compute_uv=False) ** 2
        N_t[i] = np.sum(lam / (lam + alpha[i]))
        chi2_t[i] = np.sum(((Kk @ H[i] - G) / err) ** 2)
    for n, i in enumerate(picks):
        assert abs(N_t[i] - float(truths[n][1])) <= 1e-9 * N_t[i]
    i_gcv = diagnostics.index_gcv(diagnostics.gcv(chi2_t, N_t, 200))
    i_cls = diagnostics.index_classic(diagnostics.good_data_ratio(alpha, np.asarray(res.S), N_t))
    assert out['alpha_index_gcv'] == i_gcv and out['alpha_index_classic'] == i_cls, (out['alpha_index_gcv'], i_gcv,
                                                                                       out['alpha_index_classic'], i_cls)
    print('cfg2: N_g from %.2f to %.2f, GCV minimum at index %d (chi2 = %.1f), -2 a S = N_g at index %d'
          % (out['n_good'][0], out['n_good'][-1], i_gcv, out['chi2'][i_gcv], i_cls))
    assert np.array_equal(out['A_gcv'], np.asarray(res.A)[i_gcv]) and np.array_equal(out['A_classic'], np.asarray(res.A)[i_cls])
    # an object that has not run stages a context of its own and gives the same bits
    t2 = {}
    fresh = make().fit_diagnostics(pickle.loads(pickle.dumps(res.data)), alpha='all', timing=t2)
    assert t2['reused_contexts'] == 0, t2
    for k in ('n_good', 'chi2', 'residual', 'leverage', 'gcv', 'good_data_ratio'):
        assert np.array_equal(fresh[k], out[k]), k
    assert fresh['alpha_index_gcv'] == i_gcv and fresh['alpha_index_classic'] == i_cls


def test_elementwise_one_error_bar_then_covariances_of_differing_rank():
    n_tau = 60
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, n_tau, 100)
    ew = quiet(mx.ElementwiseMaxEnt(use_hermiticity=False))
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.alpha_mesh = synthetic.alpha_mesh(8)

    def check(label, rows_of):
        res = ew.run()
        assert np.all(res.converged) and all(info['audit_max'] < AUDIT for info in ew.last_launches)
        out = ew.fit_diagnostics(res)
        longest = max(rows_of.values())
        assert out['residual'].shape == (2, 2, 8, longest) and out['n_good'].shape == (2, 2, 8)
        assert out['alpha_index_gcv'].shape == (2, 2) and out['A_classic'].shape == (2, 2, 100)
        specs = {}
        for i in range(2):
            for j in range(2):
                worker = ew.maxent_diagonal if i == j else ew.maxent_offdiagonal
                ew._load_element(worker, (i, j), True)
                spec = specs[(i, j)] = worker.maxent_loop.make_spec()
                n_rows = rows_of[(i, j)]
                assert len(spec['G']) == n_rows
                for k in ('residual', 'leverage', 'studentized'):
                    assert np.all(np.isnan(out[k][i, j][:, n_rows:])), (label, k, i, j)
                got = dict((k, out[k][i, j][:, :n_rows] if k in ('residual', 'leverage') else out[k][i, j])
                           for k in ('residual', 'leverage', 'n_good', 'chi2'))
                kind = 'normal' if i == j else 'plusminus'
                H = np.asarray(res.H[i][j])
                truths = truths_of(np.array(worker.K.K), np.asarray(worker.err), H, np.asarray(res.alpha), spec['G'],
                                   D=worker.D.D, kind=kind)
                gate('%s (%d, %d)' % (label, i, j), got, truths, row_norms(worker.K.U, worker.err), np.asarray(res.chi2[i][j]))
                assert np.all(np.isnan(out['autocorr'][i, j])) == (spec['T'] is not None)
        return res, specs
    ew.set_error(synthetic.SIGMA)
    check('2 x 2, one error bar', dict(((i, j), n_tau) for i in range(2) for j in range(2)))
    # a covariance per element whose smallest eigenvalues lie below the threshold: 0, 3, 5 and 2 directions are dropped.
    # (Given as bins: set_cov rotates every element by the hop from the previous element's rotation, which a rotation
    #  that dropped directions cannot make; set_G_tau_bins rotates each element by its own eigenbasis alone.)
    rng = np.random.RandomState(4)
    drop = {(0, 0): 0, (0, 1): 3, (1, 0): 5, (1, 1): 2}
    n_bins = 80
    bins = np.empty((n_bins, 2, 2, n_tau))
    for key, d in drop.items():
        Qm = np.linalg.qr(rng.randn(n_tau, n_tau))[0]
        s = synthetic.SIGMA * np.sqrt(n_bins) * np.sqrt(1.0 + rng.rand(n_tau))
        s[n_tau - d:] = 0.0                                    # (no noise along d directions: eigenvalues of rounding size)
        bins[(slice(None),) + key] = Gmat[key][None, :] + (rng.randn(n_bins, n_tau) * s) @ Qm.T
    ew.set_G_tau_bins(tau, bins)
    for worker in (ew.maxent_diagonal, ew.maxent_offdiagonal):
        worker.scale_alpha = float(n_tau)       # (one alpha mesh for all: 'ndata' scales by each element's own row count)
    ranks = dict((key, int(ew.bin_statistics[key]['rank'])) for key in drop)
    assert ranks == dict((key, n_tau - d) for key, d in drop.items()), ranks
    res, specs = check('2 x 2, covariances', ranks)
    # the raw call: rows behind a data set's own are written as 0
    pair = [specs[(0, 1)], specs[(1, 0)]]
    ctx = posterior._stage(ew.maxent_offdiagonal.K, pair, 0)
    try:
        H = np.stack([np.asarray(res.H[0][1][3]), np.asarray(res.H[1][0][3])])
        raw = ctx.fit_diagnostics([0, 1], np.asarray(res.alpha)[[3, 3]], H=H)
    finally:
        ctx.close()
    assert list(raw['rows']) == [57, 55] and raw['residual'].shape == (2, 57)
    assert np.all(raw['residual'][1, 55:] == 0) and np.all(raw['leverage'][1, 55:] == 0)
    assert np.all(raw['residual'][1, :55] != 0) and np.all(raw['leverage'][0] > 0)


def test_all_alphas_equal_single_calls_and_rows_of_the_last_launch_equal_rows_handed_in():
    tm, tau, omega = small_job()
    res = solved(tm)
    every = tm.fit_diagnostics(res, alpha='all')
    for ia in (0, 3, 9):
        one = tm.fit_diagnostics(res, alpha=ia)
        assert one['residual'].shape == (40,) and np.ndim(one['n_good']) == 0 and int(one['alpha_index']) == ia
        for k in ('n_good', 'chi2', 'residual', 'leverage', 'studentized', 'autocorr', 'gcv', 'good_data_ratio'):
            assert np.array_equal(one[k], every[k][ia], equal_nan=True), (k, ia)
        assert 'alpha_index_gcv' not in one
    # DeviceContext: the rows of the last launch where they lie against the same rows handed in, both entropies in one call
    _, om, K, G = synthetic.single_G(40, 64)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(om)
    alphas = np.array(synthetic.alpha_mesh(10)) * 40
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(40)))
    kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
    ctx.set_elements([ds] * 2, [G, G], np.tile(D, (2, 1)), kinds)
    v0 = np.stack([hostprep.initial_v(K.V, D, om.delta, k) for k in kinds])
    sol = ctx.solve_chains(np.arange(2), alphas, v0)
    assert sol['converged'].all() and ctx.audit()['corr'].max() < AUDIT
    pick = np.array([13, 2, 19, 0])                               # any subset, any order
    el, al = pick // 10, alphas[pick % 10]
    there = ctx.fit_diagnostics(el, al, problem_index=pick)
    H = pickle.loads(pickle.dumps(np.asarray(sol['H']).reshape(20, -1)[pick]))
    given = ctx.fit_diagnostics(el, al, H=H)
    ctx.close()
    for k in ('n_good', 'chi2', 'residual', 'leverage'):
        assert np.all(np.isfinite(there[k])) and np.array_equal(there[k], given[k]), k
    np.testing.assert_allclose(given['chi2'], np.asarray(sol['chi2']).reshape(20)[pick], rtol=1e-10)


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
    H = np.array(sol['H'][0])
    good = ctx.fit_diagnostics(np.zeros(6, dtype=int), alphas, H=H)
    assert good['residual'].shape == (6, n_tau)
    two = dict((k, good[k][[0, 5]]) for k in ('n_good', 'chi2', 'residual', 'leverage'))
    gate('128-row build', two, truths_of(np.array(K.K), err, H, alphas, G, picks=(0, 5)), row_norms(K.U, err),
         np.asarray(sol['chi2'])[0][[0, 5]])
    Hn = H.copy()
    Hn[2, 17] = np.nan
    mixed = ctx.fit_diagnostics(np.zeros(6, dtype=int), alphas, H=Hn)     # (returns: MXE_OK)
    ctx.close()
    keep = np.array([0, 1, 3, 4, 5])
    for k in ('n_good', 'chi2', 'residual', 'leverage'):
        assert np.all(np.isnan(mixed[k][2])), k
        assert np.array_equal(mixed[k][keep], good[k][keep]), k


def test_matsubara_rows_and_chi2_factor():
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
    out = tm.fit_diagnostics(res, alpha=[3, 12])
    assert out['residual'].shape == (2, 80)                   # (the 2 n_iw stacked real rows)
    spec = tm.maxent_loop.make_spec()
    Kk, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H), np.asarray(res.alpha)
    gate('matsubara', out, truths_of(Kk, err, H, alpha, spec['G'], picks=(3, 12)), row_norms(tm.K.U, err),
         np.asarray(res.chi2)[[3, 12]])
    # Q = eta chi2 / 2 - alpha S with eta != 1: exactly the outputs of the problem at alpha / eta
    ctx = posterior._stage(tm.K, [spec], 0)
    try:
        scaled = ctx.fit_diagnostics([0, 0], alpha[[3, 12]], H=H[[3, 12]], chi2_factor=2.5)
        plain = ctx.fit_diagnostics([0, 0], alpha[[3, 12]] / 2.5, H=H[[3, 12]])
    finally:
        ctx.close()
    for k in ('n_good', 'chi2', 'residual', 'leverage'):
        assert np.all(np.isfinite(scaled[k])) and np.array_equal(scaled[k], plain[k]), k
    gate('matsubara, chi2_factor 2.5', scaled, truths_of(Kk, err, H, alpha, spec['G'], picks=(3, 12), eta=2.5),
         row_norms(tm.K.U, err))


@pytest.mark.parametrize('host_projection', [False, True])
def test_new_data_on_the_same_object_are_followed(monkeypatch, host_projection):
    """set_G_tau_data again goes through mxe_elements_update_data: the part of the data outside the singular space must
    follow, on the device's and on the host's projection path"""
    if host_projection:
        monkeypatch.setenv('MXE_HOST_PROJECTION', '1')
    tm, tau, omega = small_job(n_alpha=6)
    res1 = solved(tm)
    t = {}
    first = tm.fit_diagnostics(res1, timing=t)                # (the diagnostics' state is on the device before the update)
    assert t['reused_contexts'] == 1
    _, _, _, G2 = synthetic.single_G(40, 64, seed=77)
    tm.set_G_tau_data(tau, G2)
    res2 = solved(tm)
    t = {}
    second = tm.fit_diagnostics(res2, timing=t)
    assert t['reused_contexts'] == 1, t
    spec = tm.maxent_loop.make_spec()
    assert np.array_equal(spec['G'], G2)
    Kk, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res2.H), np.asarray(res2.alpha)
    gate('new data, %s projection' % ('host' if host_projection else 'device'), second,
         truths_of(Kk, err, H, alpha, G2), row_norms(tm.K.U, err), res2.chi2)
    assert np.max(np.abs(second['residual'] - first['residual'])) > 0.1
    # a fresh object on the new data: the same bits
    tm2, _, _ = small_job(n_alpha=6, seed=77)
    fresh = tm2.fit_diagnostics(pickle.loads(pickle.dumps(res2.data)))
    for k in ('n_good', 'chi2', 'residual', 'leverage'):
        assert np.array_equal(fresh[k], second[k]), k


def test_fewer_bins_than_data_points():
    n_tau, n_bins = 40, 30
    tau, omega, K, G = synthetic.single_G(n_tau, 64)
    rng = np.random.RandomState(8)
    bins = G[None, :] + synthetic.SIGMA * np.sqrt(n_bins) * rng.randn(n_bins, n_tau)
    tm = quiet(mx.TauMaxEnt())
    tm.omega = omega
    tm.set_G_tau_bins(tau, bins)
    tm.alpha_mesh = synthetic.alpha_mesh(8)
    res = solved(tm)
    spec = tm.maxent_loop.make_spec()
    n_rows = len(spec['G'])
    assert n_rows == n_bins - 1 and n_rows < len(tm.K.S)
    out = tm.fit_diagnostics(res)
    assert out['residual'].shape == (8, n_rows) and np.all(np.isfinite(out['n_good'])) and np.all(out['n_good'] <= n_rows)
    assert np.all(np.isnan(out['autocorr']))                   # (eigen-directions of the covariance have no order)
    Kk, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H), np.asarray(res.alpha)
    gate('29 eigen-directions of 30 bins', out, truths_of(Kk, err, H, alpha, spec['G']), row_norms(tm.K.U, err), res.chi2)


def test_argument_errors_of_the_raw_call():
    tau, omega, K, G = synthetic.single_G(40, 64)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(40))
    ctx.set_elements([ds], [G], D[np.newaxis, :], [device.ENTROPY_NORMAL])
    H = np.ascontiguousarray(np.tile(D, (2, 1)))
    el = np.zeros(2, dtype=np.int32)

    def raw(P, alpha, Hrows, ld):
        al = np.ascontiguousarray(alpha, dtype=float)
        out = np.empty((2, 64))
        return ctx._lib.mxe_fit_diagnostics(ctx._h, P, device._p(el), device._p(al), device._p(Hrows), None, 1.0, ld,
                                            None, None, device._p(out), None, None)
    try:
        assert raw(2, [1.0, 2.0], H, 40) == 0                  # (every output but one NULL)
        assert raw(2, [1.0, 2.0], H, 39) == -1                 # MXE_ERR_ARG: ld below the rows of the data set
        assert raw(0, [1.0, 2.0], H, 40) == -1
        assert raw(2, [1.0, 0.0], H, 40) == -1
        assert raw(2, [1.0, -3.0], H, 40) == -1
        assert raw(2, [1.0, 2.0], None, 40) == -4              # MXE_ERR_STATE: nothing was launched
        with pytest.raises(ValueError):
            ctx.fit_diagnostics([0, 0], [1.0, 0.0], H=H)
        with pytest.raises(device.MaxEntDeviceError):
            ctx.fit_diagnostics([0, 0], [1.0, 2.0], H=H, ld=39)
        with pytest.raises(device.MaxEntDeviceError):
            ctx.fit_diagnostics([0, 0], [1.0, 2.0])
    finally:
        ctx.close()
