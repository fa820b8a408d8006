"""Whole-matrix continuation with one error bar per matrix element, the part that needs no GPU: the host functions
(``component_errors``, ``whiten_components``), the numpy truth (tests/fullmatrix_metric_ref.py) checked itself, every
refusal before the device or the library is touched, and every condition tests/test_gpu_fullmatrix_metric.py rests on --
that under the seeded error pattern the truth accepts (rejects, halves) the steps the device is expected to accept
(reject, halve) by a clear margin, and that the gate on the backward error sees the errors the new code could make."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, full_matrix
from maxent_amd.full_matrix import FullMatrixMaxEnt, component_errors, full_matrix_continue, whiten_components
import fullmatrix_ref as R
import fullmatrix_cases as C
import fullmatrix_metric_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
MARGIN = 1e-3                       # a clear change of Q, relative to |Q| (tests/test_fullmatrix_steps_host.py)
SMALL = (2, False, 16, 20, 24, False)


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    return dict((k, z[k]) for k in z.files)


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(device, 'load_library', refuse)
    monkeypatch.setattr(device, 'device_count', refuse)


# ---- the host functions --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M,cx', [(1, False), (2, False), (3, True), (4, True)])
def test_component_errors_follow_the_basis(M, cx):
    """component p carries the error of the element(s) E_p is made of, both components of a pair the same one"""
    n = 7
    sigma = MR.pattern(M, n)
    errp = component_errors(sigma, M, cx)
    E = full_matrix.hermitian_basis(M, cx)
    assert errp.shape == (len(E), n)
    for p in range(len(E)):
        a, b = (int(x) for x in np.argwhere(E[p] != 0)[0])
        assert np.array_equal(errp[p], sigma[a, b]) and np.array_equal(errp[p], sigma[b, a])
    if M > 1 and cx:
        no = M * (M - 1) // 2
        assert np.array_equal(errp[M:M + no], errp[M + no:])
    assert np.array_equal(errp, MR.component_sigma(sigma, M, cx))
    # (M, M): one value per element, broadcast over the points when their number is given
    assert component_errors(sigma[:, :, 0], M, cx).shape == (len(E), 1)
    assert np.array_equal(component_errors(sigma[:, :, 0], M, cx, n), np.repeat(errp[:, :1], n, axis=1))


def test_component_errors_refuse():
    ok = MR.pattern(2, 5)
    for bad in (ok[0], ok[:, :1], np.ones((3, 3, 5)), np.ones(5), 1e-3, ok.astype(complex), np.ones((2, 2, 0))):
        with pytest.raises(ValueError, match='shape'):
            component_errors(bad, 2, False)
    with pytest.raises(ValueError, match='shape'):
        component_errors(ok, 2, False, n=6)
    for v in (0.0, -1.0, np.nan, np.inf):
        bad = ok.copy()
        bad[1, 1, 2] = v
        with pytest.raises(ValueError, match='positive and finite'):
            component_errors(bad, 2, False)
    bad = ok.copy()
    bad[0, 1, 3] *= 1.0 + 1e-15
    with pytest.raises(ValueError, match='symmetric'):
        component_errors(bad, 2, False)


@pytest.mark.parametrize('case', [SMALL, (3, True, 17, 21, 24, False)], ids=C.case_id)
def test_whiten_components(case):
    p, a = MR.problem(case)
    U, S, V, G, sigma = a['U'], a['S'], a['V'], a['G'], a['sigma']
    M, cx = case[0], case[1]
    errp = component_errors(sigma, M, cx)
    Rm, Am, Qh = whiten_components(U, S, errp)
    n_s = len(S)
    assert Rm.shape == Am.shape == (p.P, n_s, n_s) and Qh.shape == (p.P, case[4], n_s)
    for k in range(p.P):
        want = np.dot((U * S).T / errp[k] ** 2, U * S)                      # S U^T diag(sigma_p^-2) U S
        assert np.max(np.abs(np.dot(Rm[k].T, Rm[k]) - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.max(np.abs(Am[k] - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.allclose(np.dot(Qh[k].T, Qh[k]), np.eye(n_s), atol=1e-13)
        assert np.array_equal(Rm[k], np.triu(Rm[k]))
    # chi2 of the whitened form = the direct Frobenius sum over elements and points, at a random u
    u = 0.3 * np.random.RandomState(2).randn(p.P, n_s)
    st = p.state(u)
    H = np.moveaxis(st['Hm'], 0, -1)                                        # (M, M, n_omega)
    K = np.dot(U * S, V.T)
    direct = float(np.sum(np.abs(G - np.einsum('tw,abw->abt', K, H)) ** 2 / sigma ** 2))
    Gw = R.coords(G, full_matrix.hermitian_basis(M, cx)) / errp
    ghat = np.einsum('pts,pt->ps', Qh, Gw)
    cperp = max(float(np.sum(Gw ** 2) - np.sum(ghat ** 2)), 0.0)
    rho = np.einsum('pks,ps->pk', Rm, np.dot(st['Hc'], V)) - ghat
    print('chi2: whitened %.15g, direct %.15g, the truth %.15g' % (np.sum(rho ** 2) + cperp, direct, st['chi2']))
    assert np.isclose(np.sum(rho ** 2) + cperp, direct, rtol=1e-10, atol=0)
    assert np.isclose(st['chi2'], direct, rtol=1e-10, atol=0)
    # equal errors: one factorisation for all components, R = diag(S / sigma) up to signs
    R1, A1, _ = whiten_components(U, S, np.full((p.P, 1), 2e-3))
    assert all(np.array_equal(R1[k], R1[0]) for k in range(p.P))
    assert np.allclose(np.abs(R1[0]), np.diag(S / 2e-3), rtol=0, atol=1e-12 * S[0] / 2e-3)
    with pytest.raises(ValueError):
        whiten_components(U, S, np.ones((p.P, 3)))


# ---- the truth -----------------------------------------------------------------------------------------------------------

def test_equal_errors_reproduce_the_one_error_truth():
    p1, a = C.problem(SMALL)
    pm = MR.MetricProblem(a['U'], a['S'], a['V'], a['G'], np.full(a['G'].shape, a['err']), a['D'], a['use_complex'])
    alphas = np.array(C.case_alphas(SMALL))
    one, met = R.alpha_scan(p1, alphas), MR.alpha_scan(pm, alphas)
    assert one['converged'].all() and met['converged'].all()
    e = np.max(np.abs(met['H'] - one['H'])) / np.max(np.abs(one['H']))
    print('equal errors: max |H_metric - H| / max |H| %.2e' % e)
    assert e <= 1e-12
    assert np.allclose(met['chi2'], one['chi2'], rtol=1e-10) and np.allclose(met['S'], one['S'], rtol=1e-10)


@pytest.mark.parametrize('case', [(2, True, 5, 9, 12, False), (3, False, 4, 9, 10, False)], ids=C.case_id)
def test_F_and_J_of_the_metric_truth_agree_with_finite_differences(case):
    """dQ/du = W F (central differences of Q) and J = dF/du (central differences of F) at a random u"""
    M, cx, n_s, n_w, n_t, _ = case
    _, a = C.synthetic_problem(M, cx, n_s, n_w, n_t, seed=7, sigma=0.05)
    p = MR.MetricProblem(a['U'], a['S'], a['V'], a['G'], 50.0 * MR.pattern(M, n_t), a['D'], cx)
    u = 0.3 * np.random.RandomState(1).randn(p.P, n_s)
    alpha, h = 0.7, 1e-6
    g, J = p.grad_Q(alpha, u), p.J(alpha, u)
    gn, Jn = np.zeros(u.size), np.zeros_like(J)
    for k in range(u.size):
        e = np.zeros(u.size)
        e[k] = h
        e = e.reshape(u.shape)
        gn[k] = (p.Q(alpha, u + e) - p.Q(alpha, u - e)) / (2 * h)
        Jn[:, k] = ((p.F(alpha, u + e) - p.F(alpha, u - e)) / (2 * h)).ravel()
    # central differences with h = 1e-6: truncation h^2 and rounding eps / h, both ~1e-10 of the values
    assert np.max(np.abs(g.ravel() - gn)) <= 1e-6 * np.max(np.abs(g))
    assert np.max(np.abs(J - Jn)) <= 1e-6 * np.max(np.abs(J))
    assert np.max(np.abs(J - J.T)) > 1e-3 * np.max(np.abs(J))               # (not symmetric: the LU must not assume it)


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'mxe_fullmatrix_solve_metric' in names and 'int  mxe_fullmatrix_solve_metric(' in header
    assert 'extern "C" int mxe_fullmatrix_solve_metric(' in source
    assert hasattr(device.load_library(), 'mxe_fullmatrix_solve_metric')


def _cabi_args(**change):
    n_w, n_s, n_a, P = 6, 3, 2, 3
    a = dict(device=0, n_prob=1, m=2, is_complex=0, n_omega=n_w, n_s=n_s, n_alpha=n_a, V=np.ones((n_w, n_s)),
             R=np.ones((P, n_s, n_s)), A=np.ones((P, n_s, n_s)), D=np.ones(n_w), alpha=np.ones(n_a), ghat=np.ones((1, P, n_s)),
             cperp=np.zeros(1), u0=None, maxiter=5, tol_h=1e-9, out_u=np.zeros((1, n_a, P, n_s)),
             out_H=np.zeros((1, n_a, 1, 2, 2, n_w)), out_chi2=np.zeros(n_a), out_S=np.zeros(n_a), out_Q=np.zeros(n_a),
             out_niter=np.zeros(n_a, dtype=np.int32), out_conv=np.zeros(n_a, dtype=np.int32))
    a.update(change)
    order = ('device', 'n_prob', 'm', 'is_complex', 'n_omega', 'n_s', 'n_alpha', 'V', 'R', 'A', 'D', 'alpha', 'ghat', 'cperp',
             'u0', 'maxiter', 'tol_h', 'out_u', 'out_H', 'out_chi2', 'out_S', 'out_Q', 'out_niter', 'out_conv')
    return [device._p(a[k]) if isinstance(a[k], np.ndarray) else a[k] for k in order] + [None]


def _with(value):
    x = np.ones((3, 3, 3))
    x[2, 1, 0] = value
    return x


@pytest.mark.parametrize('change,code', [
    (dict(n_prob=0), -1), (dict(m=0), -1), (dict(is_complex=2), -1), (dict(n_omega=0), -1), (dict(n_s=0), -1),
    (dict(n_alpha=0), -1), (dict(maxiter=-1), -1), (dict(tol_h=0.0), -1), (dict(tol_h=float('nan')), -1),
    (dict(V=None), -1), (dict(ghat=None), -1), (dict(out_H=None), -1), (dict(out_conv=None), -1),
    (dict(D=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])), -1),
    (dict(alpha=np.array([1.0, np.nan])), -1), (dict(cperp=np.array([np.inf])), -1),
    (dict(m=5), -5), (dict(n_s=65), -5),
    (dict(R=None), -1), (dict(A=None), -1), (dict(R=_with(np.nan)), -1), (dict(A=_with(np.nan)), -1),
    (dict(R=_with(np.inf)), -1), (dict(A=_with(-np.inf)), -1),
])
def test_the_c_interface_refuses_before_the_device(change, code):
    """MXE_ERR_ARG (-1) and MXE_ERR_LIMIT (-5) come before a device is looked for: this runs without one.  (The c of the
    one-error entry has no counterpart: R and A need not be positive.)"""
    lib = device.load_library()
    if change.get('n_s') == 65:
        change = dict(change, V=np.ones((6, 65)), R=np.ones((3, 65, 65)), A=np.ones((3, 65, 65)), ghat=np.ones((1, 3, 65)))
    assert lib.mxe_fullmatrix_solve_metric(*_cabi_args(**change)) == code


def test_fullmatrix_solve_metric_refuses_before_the_library(no_library):
    ok = dict(V=np.ones((6, 3)), R=np.ones((3, 3, 3)), A=np.ones((3, 3, 3)), D=np.ones(6), alpha=np.ones(2),
              ghat=np.ones((1, 3, 3)), cperp=np.zeros(1), m=2, use_complex=False)
    for change in (dict(m=5), dict(m=0), dict(V=np.ones(6)), dict(R=np.ones((3, 3))), dict(A=np.ones((3, 3, 4))),
                   dict(R=np.ones((4, 3, 3))), dict(D=np.ones(5)), dict(alpha=np.ones((2, 1))), dict(ghat=np.ones((1, 4, 3))),
                   dict(cperp=np.zeros(2)), dict(u0=np.zeros((1, 3, 2))), dict(D=np.array([1.0, 1, 1, 1, 1, np.nan])),
                   dict(R=_with(np.nan)), dict(A=_with(np.inf)), dict(alpha=np.array([1.0, 0.0])), dict(maxiter=-1),
                   dict(tol_h=0.0), dict(use_complex=True)):
        with pytest.raises(ValueError):
            device.fullmatrix_solve_metric(**dict(ok, **change))
    with pytest.raises(ValueError, match='reduce_singular_space'):
        device.fullmatrix_solve_metric(**dict(ok, V=np.ones((6, 65)), R=np.ones((3, 65, 65)), A=np.ones((3, 65, 65)),
                                              ghat=np.ones((1, 3, 65))))


def test_element_errors_refuse_before_the_library(fixture, no_library):
    z = fixture
    n = len(z['tau'])
    good = np.full((2, 2, n), 1e-3)
    G = z['G_tau_noise'][None]
    args = (z['U'], z['S'], z['V'], z['D'], z['ew_alpha'])

    def cont(**kw):
        return full_matrix_continue(G, *args, **kw)
    asym = good.copy()
    asym[0, 1] *= 2.0
    nonpos = good.copy()
    nonpos[1, 1, 5] = 0.0
    with pytest.raises(ValueError, match='symmetric'):
        cont(element_err=asym)
    with pytest.raises(ValueError, match='positive and finite'):
        cont(element_err=nonpos)
    for bad in (good[:, :, :-1], good[0], np.full((3, 3), 1e-3), 1e-3):
        with pytest.raises(ValueError, match='shape'):
            cont(element_err=bad)
    with pytest.raises(ValueError, match='not both'):
        cont(err=1e-3, element_err=good)
    with pytest.raises(ValueError, match='not both'):
        full_matrix_continue(G, *args + (1e-3,), element_err=good)
    with pytest.raises(ValueError, match='no error'):
        cont()
    # the Hermiticity check looks at the error of the element: the same asymmetry passes under a large sigma_01 (the
    # library is reached: the AssertionError of the fixture) and is refused under a small one
    Ga = z['G_tau_noise'].copy()
    Ga[0, 1] += 1e-2
    big = good.copy()
    big[0, 1] = big[1, 0] = 1e-2
    with pytest.raises(ValueError, match='not Hermitian within its error'):
        full_matrix_continue(Ga[None], *args, element_err=good)
    with pytest.raises(AssertionError, match='the library was touched'):
        full_matrix_continue(Ga[None], *args, element_err=big)
    # the class
    with pytest.raises(ValueError, match='set the data first'):
        FullMatrixMaxEnt().set_element_errors(good)
    fm = FullMatrixMaxEnt()
    fm.omega = mx.DataOmegaMesh(z['omega'])
    fm.set_G_tau_data(z['tau'], z['G_tau_noise'])
    for bad, what in ((asym, 'symmetric'), (nonpos, 'positive and finite'), (good[:, :, :-1], 'shape'), (good[0], 'shape'),
                      (1e-3, 'shape')):
        with pytest.raises(ValueError, match=what):
            fm.set_element_errors(bad)
    assert fm.element_err is None
    with pytest.raises(ValueError, match='no error'):
        fm.run()
    # one replaces the other; the worker holds the error of element (0, 0)
    sigma = MR.pattern(2, n)
    fm.set_element_errors(sigma)
    assert np.array_equal(fm.element_err, sigma) and np.array_equal(fm.maxent.maxent_loop.err, sigma[0, 0])
    job = fm._job()
    assert job['err'] is None and np.array_equal(job['element_err'], sigma)
    assert job['alpha'][0] == fm.alpha_mesh[0] * n                          # alpha scaled by n_tau as before
    fm.set_error(2e-3)
    assert fm.element_err is None
    job = fm._job()
    assert job['element_err'] is None and np.all(job['err'] == 2e-3)
    fm.set_element_errors(sigma[:, :, 0])                                   # (M, M): one value per element
    assert fm.element_err.shape == (2, 2, n) and np.array_equal(fm.element_err[:, :, 7], sigma[:, :, 0])
    with pytest.raises(ValueError, match='per-element'):                    # the old names keep refusing, and say where to go
        fm.set_error(sigma)
    with pytest.raises(ValueError, match='set_element_errors'):
        fm.set_error(sigma)
    with pytest.raises(ValueError, match='element_err'):
        full_matrix_continue(G, *args, err=sigma)


# ---- the conditions of the GPU tests -------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', C.ACCEPT_CASES, ids=C.case_id)
def test_the_truth_accepts_the_full_step_under_the_pattern(case):
    """the truth converges from zero at a0 and warm at a1 in 2 to 7 steps; the undamped step at a1 from u(a0) lowers Q by more
    than MARGIN |Q|; cond(J) <= 270; the gate of the device test is printed"""
    ref = MR.reference_scan(case)
    s = MR.accepted_step(case)
    cond = np.linalg.cond(s['J'])
    print(C.gate_row(C.case_id(case), s), ' dQ / |Q| at the full step %.2e,  cond(J) %.0f,  truth n_iter %s'
          % (s['dQ'][0], cond, ref['n_iter']))
    assert ref['converged'].all() and np.all(ref['n_iter'] >= 2) and np.all(ref['n_iter'] <= 7)
    assert s['dQ'][0] < -MARGIN
    assert cond <= 270.0
    assert 0.0 < s['eta_ref'] <= 16 * C.EPS                    # LAPACK's own: a small multiple of eps
    assert s['eta_pert'] > 0.0 and s['gate'] == C.GATE_FACTOR * max(s['eta_ref'], s['eta_pert'])
    assert s['gate'] < 1e-8                                    # far below any structural error (the mutations below)


@pytest.mark.parametrize('index', range(len(C.REJECT_CASES)))
def test_the_truth_rejects_the_full_step_and_accepts_the_half_under_the_pattern(index):
    s = MR.rejected_step(index)
    print(C.gate_row(C.case_id(s['case']), s), ' dQ / |Q| at 1, 1/2, 1/4: %.3g %.3g %.3g' % tuple(s['dQ']))
    assert s['dQ'][0] > MARGIN and s['dQ'][1] < -MARGIN
    assert s['dQ'][0] > 10.0 and s['dQ'][1] < -0.5             # (+14.7, +39.4 and -0.90, -0.80 when this was written)
    assert s['gate'] < 1e-8


def test_the_helpers_of_the_step_tests_work_on_the_subclass():
    p, _ = MR.problem(SMALL)
    s = MR.accepted_step(SMALL)
    assert isinstance(p, R.Problem) and p.c is None
    assert np.array_equal(s['J'], p.J(s['alpha'], s['u0'])) and np.array_equal(s['F'], p.F(s['alpha'], s['u0']).ravel())
    assert np.allclose(np.dot(s['J'], s['delta']), s['F'], rtol=0, atol=1e-12 * np.max(np.abs(s['F'])))
    assert C.backward_error(s['J'], s['F'], s['delta']) == s['eta_ref']
    # the pattern matters: the step differs from that of the one-error problem at the same u0
    p1, _ = C.problem(SMALL)
    d1 = C.newton_step(p1, s['alpha'], s['u0'])['delta']
    assert np.max(np.abs(d1 - s['delta'])) > 1e-2 * np.max(np.abs(s['delta']))


def mutations(case):
    """the step of the case solved with the three places of the metric wrong, one at a time, in the ways the device could be"""
    p, _ = MR.problem(case)
    s = MR.accepted_step(case)
    J, F, alpha, u0, st = s['J'], s['F'], s['alpha'], s['u0'], s['st']
    d, n_s = F.size, case[2]
    W = p.gram(st)                                                          # (P, n_s, P, n_s)
    out = {}
    # one 16 x 16 tile of the block (0, 1) of blockdiag(A) W not written (alpha I is added elsewhere: it stays)
    Jm = J.copy()
    t = min(16, n_s)
    Jm[0:t, n_s:n_s + t] = 0.0
    out['a tile of A_p W zero'] = np.linalg.solve(Jm, F)
    # A_1 applied to block row 0
    Am = p.A.copy()
    Am[0] = p.A[1]
    Jm = alpha * np.eye(d) + np.einsum('pks,psqt->pkqt', Am, W).reshape(d, d)
    out['A_p of the wrong component'] = np.linalg.solve(Jm, F)
    # R_p in the place of R_p^T in F (a 1 x 1 R is its own transpose: no error to see)
    if n_s > 1:
        Fm = (alpha * u0 + np.einsum('pks,ps->pk', p.R, st['rho'])).ravel()
        out['R for R^T in F'] = np.linalg.solve(J, Fm)
    return s, out


# the smallest case (n_s = 1: the first two mutations exist, R is 1 x 1), the smallest with n_s > 1, and the largest.  (The
# M = 1 case has one component: neither a block (0, 1) nor a wrong component.)
@pytest.mark.parametrize('case', [(3, False, 1, 5, 6, False), SMALL, C.ACCEPT_CASES[0]], ids=C.case_id)
def test_the_gate_sees_a_wrong_metric(case):
    s, out = mutations(case)
    assert len(out) == (3 if case[2] > 1 else 2)
    for name, delta in out.items():
        eta = C.backward_error(s['J'], s['F'], delta)
        print('%s, %s: eta %.2e, gate %.2e' % (C.case_id(case), name, eta, s['gate']))
        assert not eta <= s['gate'], name
