"""Whole-matrix continuation on the device (mxe_fullmatrix_solve, FullMatrixMaxEnt) against the numpy truth
tests/fullmatrix_ref.py.  The gate on H is the project's parity gate: 1e-6 relative to max |H| of that alpha."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import synthetic
from maxent_amd.full_matrix import FullMatrixMaxEnt, full_matrix_continue
from maxent_amd.kernels import TauKernel
import fullmatrix_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GATE = 1e-6
EPS = np.finfo(float).eps


def worst(H, Href, what):
    """max over alpha of max |H - Href| / max |Href| (alpha on axis 2)"""
    e = max(float(np.max(np.abs(H[:, :, a] - Href[:, :, a])) / np.max(np.abs(Href[:, :, a]))) for a in range(H.shape[2]))
    print('%s: max |H - H_ref| / max |H_ref| over %d alphas: %.3e' % (what, H.shape[2], e))
    return e


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    return dict((k, z[k]) for k in z.files)


def test_M1_is_the_scalar_job():
    """the TauMaxEnt job of kat_tau_maxent.npz as a 1 x 1 matrix: the scalar solver's H, and the fixture's truth"""
    with np.load(os.path.join(GOLD, 'kat_tau_maxent.npz'), allow_pickle=False) as d:
        g = {k: d[k] for k in d.files}

    def load(obj, G):
        obj.set_verbosity(mx.VerbosityFlags.Quiet)
        obj.set_G_tau_data(g['tau'], G)
        obj.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.08, n_points=5)
        obj.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=200)
        obj.set_error(1.e-3)
    tm = mx.TauMaxEnt()
    load(tm, g['G'])
    scalar = tm.run()
    fm = FullMatrixMaxEnt()
    load(fm, g['G'][None, None, :])
    res = fm.run()
    assert res.H.shape == (1, 1, 5, 200) and res.chi2.shape == (5,) and np.all(res.converged)
    assert worst(res.H, np.asarray(scalar.H)[None, None], 'M = 1 against TauMaxEnt') <= GATE
    assert worst(res.H, g['H_truth'][None, None], 'M = 1 against the fixture truth') <= GATE
    assert np.allclose(res.chi2, scalar.chi2, rtol=1e-6) and np.allclose(res.S, scalar.S, rtol=1e-6, atol=1e-9)
    assert np.array_equal(res.alpha, scalar.alpha)


def test_the_fixture_as_it_is(fixture):
    """M = 2 real, n_s = 38 (no multiple of 4 or 16), n_omega = 80, through the class"""
    z = fixture
    fm = FullMatrixMaxEnt()
    fm.set_verbosity(mx.VerbosityFlags.Quiet)
    fm.omega = mx.DataOmegaMesh(z['omega'])
    fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    fm.set_G_tau_data(z['tau'], z['G_tau_noise'])
    fm.set_error(float(z['noise']))
    res = fm.run()
    K = fm.maxent.K
    assert len(K.S) % 4 != 0 and np.allclose(res.alpha, z['ew_alpha'])
    ref = R.alpha_scan(R.Problem(K.U, K.S, K.V, z['G_tau_noise'], float(z['noise']), fm.D.D, False), res.alpha)
    assert ref['converged'].all() and np.all(res.converged)
    H = np.asarray(res.H)
    assert H.shape == (2, 2, 8, 80) and H.dtype == float
    assert worst(H, ref['H'].real, 'fixture') <= GATE
    assert np.allclose(res.chi2, ref['chi2'], rtol=1e-7) and np.allclose(res.S, ref['S'], rtol=1e-6)
    assert np.allclose(res.Q, 0.5 * res.chi2 - res.alpha * res.S, rtol=1e-12)
    assert np.array_equal(H, np.swapaxes(H, 0, 1))                       # exactly Hermitian
    lam = np.linalg.eigvalsh(np.moveaxis(H, (0, 1), (-2, -1)))
    print('fixture: smallest eigenvalue of H %.3e, bound %.3e' % (lam.min(), -16 * EPS * np.max(np.abs(H))))
    assert lam.min() >= -16 * EPS * np.max(np.abs(H))
    pos = fm.positivity(res, alpha='all')
    assert np.all(pos['n_negative'] == 0) and pos['alpha'] == 'all'
    assert np.linalg.eigvalsh(np.moveaxis(z['ew_H_truth'], (0, 1), (-2, -1))).min() < -3e-2     # the element-wise truth
    # one alpha for the whole matrix; A_out is a matrix
    assert res.A.shape == (2, 2, 8, 80) and np.allclose(res.A, H / z['delta'])
    assert res.v.shape == (8, 3, len(K.S))
    for name in ('LineFitAnalyzer', 'Chi2CurvatureAnalyzer', 'EntropyAnalyzer'):
        ana = res.analyzer_results[name]
        assert ana['A_out'].shape == (2, 2, 80)
        assert np.array_equal(ana['A_out'], res.A[:, :, ana['alpha_index']])
    assert res.get_A_out().shape == (2, 2, 80)
    assert fm.positivity(res)['n_negative'] == 0


def noncommuting_G(n_tau=60, n_omega=50, sigma=1e-3, seed=7):
    tau, omega = synthetic.grids(n_tau, n_omega)
    K = TauKernel(tau=tau, omega=omega, beta=synthetic.BETA)
    w = np.asarray(omega)
    a1 = np.exp(-(w - 1.0) ** 2 / (2 * 0.6 ** 2))
    a2 = np.exp(-(w + 1.2) ** 2 / (2 * 0.9 ** 2))
    a1, a2 = a1 / np.trapezoid(a1, w), a2 / np.trapezoid(a2, w)
    th, ph = 0.3 + 0.2 * w, 0.5 * w
    Rm = np.array([[np.cos(th), -np.sin(th) * np.exp(-1j * ph)], [np.sin(th) * np.exp(1j * ph), np.cos(th) + 0j * w]])
    A = np.einsum('akw,kw,bkw->abw', Rm, np.array([a1, a2]), Rm.conj())
    rng = np.random.RandomState(seed)
    noise = sigma * (rng.randn(2, 2, n_tau) + 1j * rng.randn(2, 2, n_tau)) / np.sqrt(2.0)
    noise = 0.5 * (noise + np.conj(np.swapaxes(noise, 0, 1)))
    return omega, K, np.einsum('tw,abw->abt', K.K_delta, A) + noise, A


def test_a_spectrum_whose_matrices_do_not_commute():
    omega, K, G, A = noncommuting_G()
    comm = np.einsum('abw,bcv->acwv', A, A) - np.einsum('abv,bcw->acwv', A, A)
    assert np.max(np.abs(comm)) > 1e-3                                   # A(w) A(w') != A(w') A(w)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    alpha = np.array(mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=5)) * 60
    out = full_matrix_continue(G[None], K.U, K.S, K.V, D, alpha, 1e-3, use_complex=True)
    ref = R.alpha_scan(R.Problem(K.U, K.S, K.V, G, 1e-3, D, True), alpha)
    assert ref['converged'].all() and out['converged'].all()
    H = out['H'][0]
    assert H.dtype == complex and np.max(np.abs(H.imag)) > 1e-4
    assert worst(H, ref['H'], 'non-commuting M = 2 complex') <= GATE
    assert np.array_equal(H, np.conj(np.swapaxes(H, 0, 1)))
    assert np.linalg.eigvalsh(np.moveaxis(H, (0, 1), (-2, -1))).min() >= -16 * EPS * np.max(np.abs(H))


# (M = 4 real runs end to end in tests/test_gpu_fullmatrix_steps.py, at n_s = 64)
@pytest.mark.parametrize('M,cx,n_tau,n_omega,n_alpha,cut', [(3, False, 40, 48, 4, None), (4, True, 40, 32, 2, 12),
                                                          (3, True, 40, 32, 2, 12)])
def test_other_sizes(M, cx, n_tau, n_omega, n_alpha, cut):
    tau, omega, K, G, _ = synthetic.matrix_G(M, n_tau, n_omega)
    sigma = 1e-3
    rng = np.random.RandomState(11)
    if cx:
        ph = np.exp(1j * np.linspace(0.2, 1.4, M))
        G = G * (ph[:, None, None] * ph.conj()[None, :, None])           # U G U^H with a diagonal unitary: complex Hermitian
    noise = sigma * rng.randn(M, M, n_tau)
    G = G + 0.5 * (noise + noise.transpose(1, 0, 2))
    K.reduce_singular_space(1e-14)
    if cut is not None:
        S = np.array(K.S)
        K.reduce_singular_space(float(np.sqrt(S[cut - 1] * S[cut])))
        assert len(K.S) == cut
    D = synthetic.flat_D(omega)
    alpha = np.array(mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=n_alpha)) * n_tau
    out = full_matrix_continue(G[None], K.U, K.S, K.V, D, alpha, sigma, use_complex=cx)
    ref = R.alpha_scan(R.Problem(K.U, K.S, K.V, G, sigma, D, cx), alpha)
    assert ref['converged'].all() and out['converged'].all()
    assert out['u'].shape == (1, n_alpha, M * M if cx else M * (M + 1) // 2, len(K.S))
    H = out['H'][0]
    assert worst(H, ref['H'] if cx else ref['H'].real, 'M = %d %s' % (M, 'complex' if cx else 'real')) <= GATE
    assert np.array_equal(H, np.conj(np.swapaxes(H, 0, 1)))
    assert np.linalg.eigvalsh(np.moveaxis(H, (0, 1), (-2, -1))).min() >= -16 * EPS * np.max(np.abs(H))
    assert np.allclose(out['chi2'][0], ref['chi2'], rtol=1e-6)


def test_block_diagonal_data_on_the_device(fixture):
    z = fixture
    G = z['G_tau_noise'].copy()
    G[0, 1] = G[1, 0] = 0.0
    out = full_matrix_continue(G[None], z['U'], z['S'], z['V'], z['D'], z['ew_alpha'], float(z['noise']))
    assert out['converged'].all()
    H, T = out['H'][0], z['ew_H_truth']
    for k in (0, 1):
        e = max(np.max(np.abs(H[k, k, a] - T[k, k, a])) / np.max(np.abs(T[k, k, a])) for a in range(8))
        print('block-diagonal: element (%d, %d) against ew_H_truth: %.3e' % (k, k, e))
        assert e <= GATE
    off = max(np.max(np.abs(H[0, 1, a])) / np.max(np.abs(H[:, :, a])) for a in range(8))
    print('block-diagonal: off-diagonal / max |H|: %.3e' % off)
    assert off <= 1e-12


def test_one_error_per_tau(fixture):
    """errors that differ from tau to tau (shared by all elements) go through the whitened basis; u comes back in the basis
    of V: H = D exp(sum_p (V u)_p E_p)"""
    from maxent_amd.full_matrix import whiten
    z = fixture
    err = float(z['noise']) * (1.0 + 0.5 * np.sin(np.arange(201) / 7.0) ** 2)
    alpha = z['ew_alpha'][:4]
    out = full_matrix_continue(z['G_tau_noise'][None], z['U'], z['S'], z['V'], z['D'], alpha, err)
    Uh, c, Vw, Q = whiten(z['U'], z['S'], z['V'], err)
    assert Q is not None
    ref = R.alpha_scan(R.Problem(Uh, c, Vw, z['G_tau_noise'] / err, 1.0, z['D'], False), alpha)
    assert ref['converged'].all() and out['converged'].all()
    H = out['H'][0]
    assert worst(H, ref['H'].real, 'one error per tau') <= GATE
    E = R.basis(2, False)
    for a in range(4):
        Gam = np.moveaxis(R.from_coords(np.dot(out['u'][0, a], z['V'].T), E), -1, 0)
        g, W = np.linalg.eigh(Gam)
        Hu = z['D'][:, None, None] * np.einsum('iak,ik,ibk->iab', W, np.exp(g), W.conj()).real
        e = np.max(np.abs(np.moveaxis(Hu, 0, -1) - H[:, :, a])) / np.max(np.abs(H[:, :, a]))
        print('one error per tau: H from the returned u, alpha %d: %.3e' % (a, e))
        assert e <= 1e-9                                                 # (rounding of V u and of exp: ~1e-13 expected)


def test_a_problem_does_not_see_its_batch(fixture):
    z = fixture
    G0 = z['G_tau_noise']
    G1 = G0.copy()
    G1[0, 1] = G1[1, 0] = 0.0
    G2 = G0[::-1, ::-1].copy() * 0.8
    args = (z['U'], z['S'], z['V'], z['D'], z['ew_alpha'][:4], float(z['noise']))
    batch = full_matrix_continue(np.stack([G0, G1, G2]), *args)
    for n, G in enumerate((G0, G1, G2)):
        one = full_matrix_continue(G[None], *args)
        for name in ('u', 'H', 'chi2', 'S', 'Q', 'n_iter', 'converged'):
            assert np.array_equal(batch[name][n], one[name][0]), (n, name)


def test_maxiter_ends_the_kernel(fixture):
    z = fixture
    args = (z['U'], z['S'], z['V'], z['D'], z['ew_alpha'][:3], float(z['noise']))
    p = R.Problem(z['U'], z['S'], z['V'], z['G_tau_noise'], float(z['noise']), z['D'], False)
    ref = R.alpha_scan(p, z['ew_alpha'][:3])
    assert ref['n_iter'][0] > 2                                          # the truth needs more steps from the cold start
    out = full_matrix_continue(z['G_tau_noise'][None], *args, maxiter=2)
    assert not out['converged'][0, 0] and np.all(out['n_iter'] <= 2) and out['n_iter'][0, 0] == 2
    for name in ('u', 'H', 'chi2', 'S', 'Q'):
        assert np.all(np.isfinite(out[name])), name
    full = full_matrix_continue(z['G_tau_noise'][None], *args)
    assert full['converged'].all() and np.all(full['n_iter'] >= 1)
