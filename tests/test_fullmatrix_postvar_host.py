"""Posterior variances of the whole-matrix continuation, the parts that need no GPU: the numpy truth
tests/fullmatrix_postvar_ref.py against itself (the order-d form the device uses against the dense form), against the scalar
formula of DESIGN 4m, the host glue of ``full_matrix_posterior_errors`` and every refusal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, full_matrix
from maxent_amd.full_matrix import FullMatrixMaxEnt
import fullmatrix_ref as R
import fullmatrix_postvar_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    return dict((k, z[k]) for k in z.files)


# ---- the truth itself ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M,cx,n_w,n_s', [(1, False, 24, 5), (2, True, 30, 8), (3, False, 28, 7), (4, True, 20, 6)])
def test_the_order_d_form_is_the_dense_form(M, cx, n_w, n_s):
    """(a), Woodbury of order d = P n_s in extended precision, against (b), the covariance of order n_omega P in binary64.
    The two agree to 1e-11 of the prior (measured: 1e-13; (b) solves with a matrix of condition ~1e3)."""
    p = PR.make_problem(M, cx, n_w, n_s, seed=11 + M, err=0.02)
    u, alpha = PR.random_u(p, 5 + M), 0.4
    F = PR.random_functionals(p, 5, 3)
    a = PR.variances(p, u, alpha, F, diag=True)
    Gam, L, kappa = PR.dense_covariance(p, u, alpha)
    f = np.moveaxis(F, 1, 2).reshape(len(F), -1)                     # (n_f, (i, p))
    var_b = np.einsum('ni,ij,nj->n', f, Gam, f)
    diag_b = np.diag(Gam).reshape(n_w, p.P).T
    bound = 1e-11
    e_f = float(np.max(np.abs(a['var'] - var_b) / a['prior']))
    e_d = float(np.max(np.abs(a['diag_var'] - diag_b) / a['diag_prior']))
    print('M %d complex %d: functionals %.2e, diagonal %.2e of the prior (bound %.2e, condition %.1f); smallest var / prior %.3g'
          % (M, cx, e_f, e_d, bound, kappa, min(float(np.min(a['var'] / a['prior'])), float(np.min(a['diag_var'] / a['diag_prior'])))))
    assert e_f <= bound and e_d <= bound
    # the prior is f^T L f / alpha, the value f^T h
    st = p.state(u)
    assert np.allclose(np.asarray(a['prior'], dtype=float), np.einsum('npi,ipq,nqi->n', F, L, F) / alpha, rtol=1e-13)
    assert np.allclose(np.asarray(a['value'], dtype=float), np.einsum('npi,pi->n', F, st['Hc']), rtol=1e-12, atol=1e-14)
    assert np.all(a['var'] <= a['prior']) and np.all(a['diag_var'] <= a['diag_prior']) and np.all(a['diag_var'] > 0)


def test_M1_is_the_scalar_formula():
    """P = 1: L_i = H_i, and the variances are those of DESIGN 4m with w = H"""
    p = PR.make_problem(1, False, 24, 5, seed=3, err=0.02)
    u, alpha = PR.random_u(p, 4), 0.3
    F = PR.random_functionals(p, 4, 9)
    a = PR.variances(p, u, alpha, F, diag=True)
    H = p.state(u)['Hc'][0]
    assert np.allclose(H, p.D * np.exp(np.dot(p.V, u[0])), rtol=1e-13)
    s = PR.scalar_variances(H, p.V, p.c, alpha, F[:, 0], diag=True)
    for k, kk in (('var', 'var'), ('prior', 'prior'), ('diag_var', 'diag_var')):
        x, y = np.asarray(a[k], dtype=np.longdouble).ravel(), np.asarray(s[kk]).ravel()
        assert float(np.max(np.abs(x - y) / np.abs(y))) <= 1e-13, k


def test_block_diagonal_Gamma_gives_the_two_scalar_problems():
    """the off-diagonal rows of u are zero: H is diagonal, B decouples, and the variances of the diagonal components are
    those of the two scalar problems with H = D exp(V u_a)"""
    for cx in (False, True):
        p = PR.make_problem(2, cx, 26, 6, seed=8, err=0.02)
        u, alpha = PR.random_u(p, 2), 0.5
        u[2:] = 0.0
        a = PR.variances(p, u, alpha, diag=True)
        for comp in (0, 1):
            H = p.D * np.exp(np.dot(p.V, u[comp]))
            s = PR.scalar_variances(H, p.V, p.c, alpha, diag=True)
            e = float(np.max(np.abs(a['diag_var'][comp] - s['diag_var']) / s['diag_var']))
            assert e <= 1e-12, (cx, comp, e)
            assert np.allclose(np.asarray(a['h'][comp], dtype=float), H, rtol=1e-13)


# ---- the host glue --------------------------------------------------------------------------------------------------------

def test_functionals_must_be_hermitian():
    n_w = 7
    rng = np.random.RandomState(0)
    X = rng.randn(3, 2, 2, n_w) + 1j * rng.randn(3, 2, 2, n_w)
    Fh = X + np.conj(np.swapaxes(X, 1, 2))
    f = full_matrix.functional_coordinates(Fh, 2, True, n_w)
    assert f.shape == (3, 4, n_w) and f.dtype == float
    E = full_matrix.hermitian_basis(2, True)
    assert np.allclose(np.einsum('npi,pab->nabi', f, E), Fh, atol=1e-14)           # F = sum_p f_p E_p
    # x = sum_i Tr(F_i H_i) = sum_p,i f_p,i h_p,i
    Y = rng.randn(2, 2, n_w) + 1j * rng.randn(2, 2, n_w)
    H = Y + np.conj(np.swapaxes(Y, 0, 1))
    h = R.coords(H, E)
    assert np.allclose(np.einsum('nabi,bai->n', Fh, H).real, np.einsum('npi,pi->n', f, h))
    assert full_matrix.functional_coordinates(Fh[0].real, 2, False, n_w).shape == (1, 3, n_w)
    with pytest.raises(ValueError, match='not Hermitian'):
        full_matrix.functional_coordinates(X, 2, True, n_w)
    with pytest.raises(ValueError, match='use_complex'):
        full_matrix.functional_coordinates(Fh, 2, False, n_w)
    with pytest.raises(ValueError, match='shape'):
        full_matrix.functional_coordinates(Fh[:, :, :, :-1], 2, True, n_w)
    with pytest.raises(ValueError, match='shape'):
        full_matrix.functional_coordinates(np.zeros((3, 3, n_w)), 2, False, n_w)
    bad = Fh.copy()
    bad[1, 0, 0, 2] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        full_matrix.functional_coordinates(bad, 2, True, n_w)
    with pytest.raises(ValueError, match='numbers'):
        full_matrix.functional_coordinates(np.full((2, 2, n_w), 'x'), 2, False, n_w)


def test_window_rows():
    omega = np.linspace(-2.0, 2.0, 9)
    f = full_matrix.window_coordinates(omega, [(-2, 0), (0.4, 1.6)], 2, False)
    assert f.shape == (2 * 4, 3, 9)
    inside = [(omega >= -2) & (omega <= 0), (omega >= 0.4) & (omega <= 1.6)]
    for w in range(2):
        for p in range(3):
            want = np.zeros((3, 9))
            want[p] = inside[w]
            assert np.array_equal(f[4 * w + p], want)
        want = np.zeros((3, 9))
        want[:2] = inside[w]                                          # the trace: the diagonal units
        assert np.array_equal(f[4 * w + 3], want)
    with pytest.raises(ValueError, match='outside'):
        full_matrix.window_coordinates(omega, [(-3, 0)], 2, False)


@pytest.mark.parametrize('M,cx', [(1, False), (2, False), (3, True), (4, True)])
def test_coordinates_and_matrix_elements(M, cx):
    E = full_matrix.hermitian_basis(M, cx)
    P = len(E)
    rng = np.random.RandomState(M)
    x = rng.randn(5, P)
    re, im = full_matrix.elements_of_coordinates(x, M, cx)
    X = np.einsum('np,pab->nab', x, E)
    assert np.allclose(re, X.real, atol=1e-15) and np.allclose(im, X.imag, atol=1e-15)
    # independent coordinates with variances v: Re X_ab = x_p / sqrt 2 has the variance v_p / 2, Im X_ab v_p' / 2
    v = rng.rand(5, P)
    ere, eim = full_matrix.element_errors_of_coordinates(v, M, cx)
    want_re = np.sqrt(np.einsum('np,pab->nab', v, E.real ** 2))
    want_im = np.sqrt(np.einsum('np,pab->nab', v, E.imag ** 2))
    assert np.allclose(ere, want_re, atol=1e-15) and np.allclose(eim, want_im, atol=1e-15)
    assert np.all(eim[:, np.arange(M), np.arange(M)] == 0) and np.array_equal(eim, np.swapaxes(eim, 1, 2))
    if not cx:
        assert np.all(eim == 0)


# ---- the entry point and the refusals ---------------------------------------------------------------------------------------

def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert 'mxe_fullmatrix_posterior_var' in names and 'int  mxe_fullmatrix_posterior_var(' in header
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_fullmatrix_posterior_var(' in source and '#include "mxe_fullmatrix_postvar.hip.h"' in source
    hdr = [line for line in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')) if line.startswith('HDR')]
    assert len(hdr) == 1 and 'mxe_fullmatrix_postvar.hip.h' in hdr[0].split()
    assert hasattr(device.load_library(), 'mxe_fullmatrix_posterior_var')
    assert mx.full_matrix_posterior_errors is full_matrix.full_matrix_posterior_errors


def _cabi_args(**change):
    n_w, n_s, n_j, n_f, P = 6, 3, 2, 2, 3
    a = dict(device=0, n_job=n_j, m=2, is_complex=0, n_omega=n_w, n_s=n_s, n_f=n_f, V=np.ones((n_w, n_s)), c=np.ones(n_s),
             D=np.ones(n_w), alpha=np.ones(n_j), u=np.zeros((n_j, P, n_s)), F=np.ones((n_f, P, n_w)), want_diag=1,
             out_value=np.zeros((n_j, n_f)), out_var=np.zeros((n_j, n_f)), out_prior=np.zeros((n_j, n_f)),
             out_dv=np.zeros((n_j, P, n_w)), out_dp=np.zeros((n_j, P, n_w)), out_h=np.zeros((n_j, P, n_w)))
    a.update(change)
    order = ('device', 'n_job', 'm', 'is_complex', 'n_omega', 'n_s', 'n_f', 'V', 'c', 'D', 'alpha', 'u', 'F', 'want_diag',
             'out_value', 'out_var', 'out_prior', 'out_dv', 'out_dp', 'out_h')
    return [device._p(a[k]) if isinstance(a[k], np.ndarray) else a[k] for k in order] + [None]


@pytest.mark.parametrize('change,code', [
    (dict(n_job=0), -1), (dict(m=0), -1), (dict(is_complex=2), -1), (dict(n_omega=0), -1), (dict(n_s=0), -1), (dict(n_f=-1), -1),
    (dict(want_diag=2), -1), (dict(n_f=0, want_diag=0), -1), (dict(V=None), -1), (dict(u=None), -1), (dict(F=None), -1),
    (dict(out_var=None), -1), (dict(out_h=None), -1),
    (dict(D=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])), -1), (dict(c=np.array([1.0, -1.0, 1.0])), -1),
    (dict(alpha=np.array([1.0, np.nan])), -1), (dict(alpha=np.array([1.0, 0.0])), -1),
    (dict(F=np.full((2, 3, 6), np.inf)), -1),
    (dict(m=5), -5), (dict(n_s=65), -5),
])
def test_the_c_interface_refuses_before_the_device(change, code):
    """MXE_ERR_ARG (-1) and MXE_ERR_LIMIT (-5) come before a device is looked for: this runs without one"""
    lib = device.load_library()
    if change.get('n_s') == 65:
        change = dict(change, V=np.ones((6, 65)), c=np.ones(65), u=np.zeros((2, 3, 65)))
    assert lib.mxe_fullmatrix_posterior_var(*_cabi_args(**change)) == code


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(device, 'load_library', refuse)
    monkeypatch.setattr(device, 'device_count', refuse)


def test_fullmatrix_posterior_var_refuses_before_the_library(no_library):
    ok = dict(V=np.ones((6, 3)), c=np.ones(3), D=np.ones(6), alpha=np.ones(2), u=np.zeros((2, 3, 3)), m=2, use_complex=False,
              F=np.ones((2, 3, 6)))
    for change in (dict(m=5), dict(m=0), dict(V=np.ones(6)), dict(c=np.ones(4)), dict(D=np.ones(5)), dict(alpha=np.ones((2, 1))),
                   dict(u=np.zeros((1, 3, 3))), dict(u=np.zeros((2, 4, 3))), dict(F=np.ones((2, 3, 5))), dict(F=np.ones((3, 6))),
                   dict(D=np.array([1.0, 1, 1, 1, 1, np.nan])), dict(alpha=np.array([1.0, 0.0])), dict(c=np.array([1.0, 0.0, 1.0])),
                   dict(F=np.full((2, 3, 6), np.nan)), dict(F=None), dict(F=np.ones((0, 3, 6))), dict(use_complex=True)):
        with pytest.raises(ValueError):
            device.fullmatrix_posterior_var(**dict(ok, **change))
    with pytest.raises(ValueError, match='reduce_singular_space'):
        device.fullmatrix_posterior_var(**dict(ok, V=np.ones((6, 65)), c=np.ones(65), u=np.zeros((2, 3, 65))))
    # a u that is not finite is no refusal: the library is reached (here: the stand-in that refuses)
    with pytest.raises(AssertionError, match='the library was touched'):
        device.fullmatrix_posterior_var(**dict(ok, u=np.full((2, 3, 3), np.nan)))


def loaded(fixture, **kw):
    fm = FullMatrixMaxEnt(**kw)
    fm.omega = mx.DataOmegaMesh(fixture['omega'])
    fm.set_G_tau_data(fixture['tau'], fixture['G_tau_noise'])
    fm.set_error(float(fixture['noise']))
    return fm


NEWLY_REFUSED = ('posterior_samples', 'fit_diagnostics', 'resolution', 'default_model_response', 'resample_errors',
                 'parametric_bootstrap', 'default_model_scan', 'check_bins')


def test_the_result_taking_methods_of_the_worker_are_refused(fixture, no_library):
    fm = loaded(fixture)
    for name in NEWLY_REFUSED:
        assert hasattr(fm.maxent, name), name                       # (it would be forwarded to the scalar worker)
        with pytest.raises(NotImplementedError, match=name):
            getattr(fm, name)(None)
    # posterior_errors is the class's own, not the worker's
    assert FullMatrixMaxEnt.posterior_errors is not None and 'posterior_errors' not in full_matrix._REFUSED
    assert fm.posterior_errors.__func__ is FullMatrixMaxEnt.posterior_errors


def test_posterior_errors_refuses(fixture, no_library):
    fm = loaded(fixture)
    with pytest.raises(ValueError, match='bryan'):
        fm.posterior_errors(result=object(), alpha='bryan', pointwise=True)
    fm.set_element_errors(np.full((2, 2), float(fixture['noise'])))
    with pytest.raises(NotImplementedError, match='set_element_errors'):
        fm.posterior_errors(result=object(), pointwise=True)


def test_full_matrix_posterior_errors_refuses(no_library):
    n_t, n_w, n_s = 12, 9, 4
    rng = np.random.RandomState(1)
    U, S, V = np.linalg.qr(rng.randn(n_t, n_s))[0], np.ones(n_s), np.linalg.qr(rng.randn(n_w, n_s))[0]
    D, omega = np.ones(n_w) / n_w, np.linspace(-1, 1, n_w)
    ok = dict(u=np.zeros((1, 2, 3, n_s)), U=U, S=S, V=V, D=D, alpha=np.ones(2), err=0.1, omega=omega, pointwise=True)
    call = lambda **change: full_matrix.full_matrix_posterior_errors(**dict(ok, **change))
    for change in (dict(u=np.zeros((2, 3, n_s))), dict(alpha=np.ones(3)), dict(u=np.zeros((1, 2, 2, n_s))),
                   dict(u=np.zeros((1, 2, 3, n_s + 1))), dict(err=np.ones((2, 2, n_t))), dict(err=-1.0), dict(err=np.ones(n_t - 1)),
                   dict(pointwise=False), dict(omega=None), dict(windows=[(-5, 0)]), dict(functionals=np.ones((2, 2, n_w + 1))),
                   dict(functionals=np.array([[0.0, 1.0], [0.5, 0.0]])[:, :, None] * np.ones(n_w))):
        with pytest.raises(ValueError):
            call(**change)
    with pytest.raises(NotImplementedError, match='matrix-valued'):
        call(D=np.ones((2, 2, n_w)))
    with pytest.raises(ValueError, match='use_complex'):
        call(functionals=np.array([[0.0, 1.0j], [-1.0j, 0.0]])[:, :, None] * np.ones(n_w))
    with pytest.raises(AssertionError, match='the library was touched'):
        call()
