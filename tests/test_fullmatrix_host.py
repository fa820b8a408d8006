"""Whole-matrix continuation, the part that needs no GPU: the numpy truth (tests/fullmatrix_ref.py) is checked itself --
finite differences, block-diagonal data against the scalar solver's extended-precision truth, unitary covariance --, the
entry point is declared, and every refusal comes before the device is touched."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, full_matrix
from maxent_amd.full_matrix import FullMatrixMaxEnt, full_matrix_continue
import fullmatrix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    return dict((k, z[k]) for k in z.files)


def random_problem(M, cx, seed, n_w=24, n_s=6, n_t=30):
    rng = np.random.default_rng(seed)
    K = rng.standard_normal((n_t, n_w))
    U, S, Vh = np.linalg.svd(K, full_matrices=False)
    G = rng.standard_normal((M, M, n_t)) + (1j * rng.standard_normal((M, M, n_t)) if cx else 0)
    G = G + np.conj(np.swapaxes(G, 0, 1))
    return R.Problem(U[:, :n_s], S[:n_s], Vh[:n_s].T, G, 0.1, np.ones(n_w) / n_w, cx), rng


# ---- the truth itself ----------------------------------------------------------------------------------------------------

def test_the_basis_is_orthonormal_and_the_same_on_both_sides():
    for M in (1, 2, 3, 4):
        for cx in (False, True):
            E = R.basis(M, cx)
            assert len(E) == (M * M if cx else M * (M + 1) // 2) == device.fullmatrix_P(M, cx)
            assert np.allclose(np.einsum('pab,qba->pq', E, E), np.eye(len(E)), atol=1e-15)
            assert np.array_equal(E, np.conj(np.swapaxes(E, 1, 2)))
            assert np.array_equal(E, full_matrix.hermitian_basis(M, cx))


@pytest.mark.parametrize('M,cx', [(2, True), (3, False)])
def test_F_and_J_agree_with_finite_differences(M, cx):
    """dQ/du = W F (central differences of Q) and J = dF/du (central differences of F) at a random u"""
    p, rng = random_problem(M, cx, seed=M)
    u = 0.3 * rng.standard_normal((p.P, 6))
    a, h = 0.7, 1e-6
    g, J = p.grad_Q(a, u), p.J(a, u)
    gn, Jn = np.zeros(u.size), np.zeros_like(J)
    for k in range(u.size):
        e = np.zeros(u.size)
        e[k] = h
        e = e.reshape(u.shape)
        gn[k] = (p.Q(a, u + e) - p.Q(a, u - e)) / (2 * h)
        Jn[:, k] = ((p.F(a, u + e) - p.F(a, u - e)) / (2 * h)).ravel()
    # central differences with h = 1e-6: truncation h^2 and rounding eps / h, both ~1e-10 of the values; measured 3e-8, 1e-9
    assert np.max(np.abs(g.ravel() - gn)) <= 1e-6 * np.max(np.abs(g))
    assert np.max(np.abs(J - Jn)) <= 1e-6 * np.max(np.abs(J))
    # cold start: every Gamma is zero, the fully degenerate case of phi
    u0 = np.zeros_like(u)
    J0 = p.J(a, u0)
    for k in range(u.size):
        e = np.zeros(u.size)
        e[k] = h
        e = e.reshape(u.shape)
        Jn[:, k] = ((p.F(a, u0 + e) - p.F(a, u0 - e)) / (2 * h)).ravel()
    assert np.max(np.abs(J0 - Jn)) <= 1e-6 * np.max(np.abs(J0))


def test_phi_is_continuous_across_its_series():
    a = np.array([0.3, -2.0, 5.0])
    for x in (0.0999999, 0.1, 0.1000001, 1e-9, 0.0):
        v = R.phi(a + x, a - x)
        exact = np.exp(a) * (np.sinh(x) / x if x else 1.0)
        assert np.allclose(v, exact, rtol=4e-16 * 8, atol=0)


def test_block_diagonal_data_give_the_scalar_truth(fixture):
    """off-diagonal data zero: the problem decouples into the two DiagonalMaxEnt problems at the same mesh alpha"""
    z = fixture
    G = z['G_tau_noise'].copy()
    G[0, 1] = G[1, 0] = 0.0
    p = R.Problem(z['U'], z['S'], z['V'], G, float(z['noise']), z['D'], False)
    out = R.alpha_scan(p, z['ew_alpha'])
    assert out['converged'].all()
    T = z['ew_H_truth']
    for a in range(8):
        for k in (0, 1):
            assert np.max(np.abs(out['H'][k, k, a].real - T[k, k, a])) <= 1e-9 * np.max(np.abs(T[k, k, a]))
        assert np.all(out['H'][0, 1, a] == 0.0) and np.all(out['H'][1, 0, a] == 0.0)


@pytest.mark.parametrize('cx', [False, True])
def test_unitary_covariance(fixture, cx):
    """continuing R G R^H gives R H R^H"""
    z = fixture
    n = 4                                                                # (alphas: the covariance holds at each of them)
    G = z['G_tau_noise'].astype(complex if cx else float)
    th = 0.7
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], dtype=complex if cx else float)
    if cx:
        Rm = np.dot(Rm, np.diag([np.exp(0.4j), np.exp(-1.1j)]))
        Rm = np.dot(np.diag([1.0, np.exp(0.9j)]), Rm)
    G = 0.5 * (G + np.conj(np.swapaxes(G, 0, 1)))
    Gr = np.einsum('ab,bct,dc->adt', Rm, G, Rm.conj())
    a = R.alpha_scan(R.Problem(z['U'], z['S'], z['V'], G, float(z['noise']), z['D'], cx), z['ew_alpha'][:n])
    b = R.alpha_scan(R.Problem(z['U'], z['S'], z['V'], Gr, float(z['noise']), z['D'], cx), z['ew_alpha'][:n])
    assert a['converged'].all() and b['converged'].all()
    Hr = np.einsum('ab,bcxi,dc->adxi', Rm, a['H'], Rm.conj())
    for x in range(n):
        assert np.max(np.abs(b['H'][:, :, x] - Hr[:, :, x])) <= 1e-9 * np.max(np.abs(Hr[:, :, x]))
    assert np.allclose(a['chi2'], b['chi2'], rtol=1e-9) and np.allclose(a['S'], b['S'], rtol=1e-9, atol=1e-12)


def test_the_truth_is_positive_where_the_elementwise_truth_is_not(fixture):
    z = fixture
    p = R.Problem(z['U'], z['S'], z['V'], z['G_tau_noise'], float(z['noise']), z['D'], False)
    out = R.alpha_scan(p, z['ew_alpha'])
    assert out['converged'].all()
    lam = np.linalg.eigvalsh(np.moveaxis(out['H'], (0, 1), (-2, -1)))
    assert lam.min() >= -16 * np.finfo(float).eps * np.max(np.abs(out['H']))
    assert np.linalg.eigvalsh(np.moveaxis(z['ew_H_truth'], (0, 1), (-2, -1))).min() < -3e-2
    assert np.array_equal(out['H'], np.conj(np.swapaxes(out['H'], 0, 1)))


# ---- the entry point -----------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert 'mxe_fullmatrix_solve' in names and 'int  mxe_fullmatrix_solve(' in header
    assert '#define MXE_FULLMATRIX_MAX_M   4' in header and device.FULLMATRIX_MAX_M == 4
    assert '#define MXE_FULLMATRIX_MAX_NS  64' in header and device.FULLMATRIX_MAX_NS == 64
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_fullmatrix_solve(' in source and '#include "mxe_fullmatrix.hip.h"' in source
    hdr = [line for line in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')) if line.startswith('HDR')]
    assert len(hdr) == 1 and 'mxe_fullmatrix.hip.h' in hdr[0].split()
    assert mx.FullMatrixMaxEnt is FullMatrixMaxEnt and mx.full_matrix_continue is full_matrix_continue
    assert issubclass(mx.FullMatrixResult, mx.MaxEntResult)


def _cabi_args(**change):
    n_w, n_s, n_a, P = 6, 3, 2, 3
    a = dict(device=0, n_prob=1, m=2, is_complex=0, n_omega=n_w, n_s=n_s, n_alpha=n_a, V=np.ones((n_w, n_s)), c=np.ones(n_s),
             D=np.ones(n_w), alpha=np.ones(n_a), ghat=np.ones((1, P, n_s)), cperp=np.zeros(1), u0=None, maxiter=5, tol_h=1e-9,
             out_u=np.zeros((1, n_a, P, n_s)), out_H=np.zeros((1, n_a, 1, 2, 2, n_w)), out_chi2=np.zeros(n_a),
             out_S=np.zeros(n_a), out_Q=np.zeros(n_a), out_niter=np.zeros(n_a, dtype=np.int32),
             out_conv=np.zeros(n_a, dtype=np.int32))
    a.update(change)
    order = ('device', 'n_prob', 'm', 'is_complex', 'n_omega', 'n_s', 'n_alpha', 'V', 'c', 'D', 'alpha', 'ghat', 'cperp', 'u0',
             'maxiter', 'tol_h', 'out_u', 'out_H', 'out_chi2', 'out_S', 'out_Q', 'out_niter', 'out_conv')
    return [device._p(a[k]) if isinstance(a[k], np.ndarray) else a[k] for k in order] + [None]


@pytest.mark.parametrize('change,code', [
    (dict(n_prob=0), -1), (dict(m=0), -1), (dict(is_complex=2), -1), (dict(n_omega=0), -1), (dict(n_s=0), -1),
    (dict(n_alpha=0), -1), (dict(maxiter=-1), -1), (dict(tol_h=0.0), -1), (dict(tol_h=float('nan')), -1),
    (dict(V=None), -1), (dict(ghat=None), -1), (dict(out_H=None), -1), (dict(out_conv=None), -1),
    (dict(D=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])), -1), (dict(c=np.array([1.0, -1.0, 1.0])), -1),
    (dict(alpha=np.array([1.0, np.nan])), -1), (dict(cperp=np.array([np.inf])), -1),
    (dict(m=5), -5), (dict(n_s=65), -5),
])
def test_the_c_interface_refuses_before_the_device(change, code):
    """MXE_ERR_ARG (-1) and MXE_ERR_LIMIT (-5) come before a device is looked for: this runs without one"""
    lib = device.load_library()
    if change.get('n_s') == 65:
        change = dict(change, V=np.ones((6, 65)), c=np.ones(65), ghat=np.ones((1, 3, 65)))
    assert lib.mxe_fullmatrix_solve(*_cabi_args(**change)) == code


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(device, 'load_library', refuse)
    monkeypatch.setattr(device, 'device_count', refuse)


def test_fullmatrix_solve_refuses_before_the_library(no_library):
    ok = dict(V=np.ones((6, 3)), c=np.ones(3), D=np.ones(6), alpha=np.ones(2), ghat=np.ones((1, 3, 3)), cperp=np.zeros(1), m=2,
              use_complex=False)
    for change in (dict(m=5), dict(m=0), dict(V=np.ones(6)), dict(c=np.ones(4)), dict(D=np.ones(5)), dict(alpha=np.ones((2, 1))),
                   dict(ghat=np.ones((1, 4, 3))), dict(cperp=np.zeros(2)), dict(u0=np.zeros((1, 3, 2))),
                   dict(D=np.array([1.0, 1, 1, 1, 1, np.nan])), dict(alpha=np.array([1.0, 0.0])), dict(maxiter=-1),
                   dict(tol_h=0.0), dict(use_complex=True)):
        with pytest.raises(ValueError):
            device.fullmatrix_solve(**dict(ok, **change))
    with pytest.raises(ValueError, match='reduce_singular_space'):
        device.fullmatrix_solve(**dict(ok, V=np.ones((6, 65)), c=np.ones(65), ghat=np.ones((1, 3, 65))))


# ---- the class -----------------------------------------------------------------------------------------------------------

def loaded(fixture, **kw):
    fm = FullMatrixMaxEnt(**kw)
    fm.omega = mx.DataOmegaMesh(fixture['omega'])
    fm.set_G_tau_data(fixture['tau'], fixture['G_tau_noise'])
    fm.set_error(float(fixture['noise']))
    return fm


def test_attributes_are_forwarded(fixture):
    fm = loaded(fixture)
    fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    assert fm.maxent.alpha_mesh is fm.alpha_mesh and len(fm.alpha_mesh) == 8
    fm.reduce_singular_space = 1e-9
    assert fm.maxent.maxent_loop.reduce_singular_space == 1e-9
    fm.minimizer.maxiter = 7
    assert fm.maxent.minimizer.maxiter == 7
    assert fm.G_mat.shape == (2, 2, 201) and fm.use_complex is False
    assert len(fm.maxent.G) == 201                                       # what scale_alpha='Ndata' counts: ONE element
    job = fm._job()
    assert job['maxiter'] == 7 and job['alpha'][0] == fm.alpha_mesh[0] * 201 and len(job['S']) <= 64


def test_every_refusal(fixture, no_library):
    z = fixture
    fm = loaded(z)
    for name, args in (('set_G_iw_data', (np.arange(3.0), np.zeros((2, 2, 3), dtype=complex))),
                       ('set_chi_tau_data', (z['tau'], z['G_tau_noise'])), ('set_chi_iw_data', (np.arange(3.0), np.zeros(3))),
                       ('set_cov', (np.eye(201),)), ('set_cov_file', ('x',)), ('set_G_tau_bins', (z['tau'], np.zeros((4, 201)))),
                       ('set_G_iw_bins', (np.arange(3.0), np.zeros((4, 3)))), ('set_G_l_bins', (np.zeros((4, 3)), 10.0)),
                       ('set_G_tau', (None,))):
        with pytest.raises(NotImplementedError, match=name):
            getattr(fm, name)(*args)
    with pytest.raises(ValueError, match='per-element'):
        fm.set_error(np.full((2, 2, 201), 1e-3))
    with pytest.raises(ValueError, match='use_complex'):
        fm.set_G_tau_data(z['tau'], z['G_tau_noise'] + 1e-3j)
    with pytest.raises(ValueError, match=r'\(M, M, n\)'):
        fm.set_G_tau_data(z['tau'], z['G_tau_noise'][0])
    with pytest.raises(ValueError, match='at most 4 x 4'):
        fm.set_G_tau_data(z['tau'], np.zeros((5, 5, 201)))
    with pytest.raises(ValueError, match='dimension'):
        fm.set_G_tau_data(z['tau'][:-1], z['G_tau_noise'])
    with pytest.raises(NotImplementedError, match='probability'):
        FullMatrixMaxEnt(probability='normal')
    with pytest.raises(NotImplementedError, match='cost_function'):
        FullMatrixMaxEnt(cost_function='plusminus')
    # at run(): analyzers, preblur, matrix-valued D, too many singular values, data that are not Hermitian
    fm = loaded(z)
    fm.analyzers = [mx.LineFitAnalyzer(), mx.BryanAnalyzer()]
    with pytest.raises(NotImplementedError, match='BryanAnalyzer'):
        fm.run()
    fm = loaded(z)
    fm.maxent.maxent_loop.probability = mx.NormalLogProbability()
    with pytest.raises(NotImplementedError, match='probability'):
        fm.run()
    fm = loaded(z)
    fm.maxent.K = mx.PreblurKernel(fm.maxent.K, 0.1)
    with pytest.raises(NotImplementedError, match='preblur'):
        fm.run()
    fm = loaded(z)
    G = z['G_tau_noise'].copy()
    G[0, 1] += 1.0
    fm.set_G_tau_data(z['tau'], G)
    with pytest.raises(ValueError, match='not Hermitian within its error'):
        fm.run()
    with pytest.raises(ValueError, match='no data'):
        FullMatrixMaxEnt().run()
    with pytest.raises(ValueError, match='set the data first'):
        FullMatrixMaxEnt().set_error(1e-3)


def test_too_many_singular_values_name_the_way_out(fixture, no_library, monkeypatch):
    fm = loaded(fixture)
    monkeypatch.setattr(full_matrix, 'MAX_NS', 10)                       # (the fixture keeps 38)
    with pytest.raises(ValueError, match='raise reduce_singular_space'):
        fm.run()


def test_full_matrix_continue_refuses(fixture, no_library):
    z = fixture
    args = (z['U'], z['S'], z['V'], z['D'], z['ew_alpha'], 1e-3)
    G = z['G_tau_noise'][None]
    with pytest.raises(ValueError, match='n_prob'):
        full_matrix_continue(G[0], *args)
    with pytest.raises(NotImplementedError, match='matrix-valued'):
        full_matrix_continue(G, z['U'], z['S'], z['V'], np.ones((2, 2, 80)), z['ew_alpha'], 1e-3)
    with pytest.raises(ValueError, match='per-element'):
        full_matrix_continue(G, z['U'], z['S'], z['V'], z['D'], z['ew_alpha'], np.full((2, 2, 201), 1e-3))
    with pytest.raises(ValueError, match='positive'):
        full_matrix_continue(G, z['U'], z['S'], z['V'], z['D'], z['ew_alpha'], 0.0)
    with pytest.raises(ValueError, match='reduce_singular_space'):
        full_matrix_continue(G, np.ones((201, 65)), np.ones(65), np.ones((80, 65)), z['D'], z['ew_alpha'], 1e-3)
    assert full_matrix.RESULT_KEYS == ('u', 'H', 'chi2', 'S', 'Q', 'n_iter', 'converged', 'alpha', 'ms')
