"""``matrix_positivity`` and ``ElementwiseMaxEnt.positivity`` on the device against the numpy mirror
(tests/positivity_ref.py), within the gates of the kernel (tests/test_gpu_hermeig.py): the reference's own outputs, a
continued real and complex 2 x 2 job, an exactly positive matrix, and chi2 in a rotated data space."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import synthetic
import positivity_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_JOBS = {}


def _fixture(name):
    return np.load(os.path.join(GOLD, name))


def _job(use_complex):
    """the fixtures' G(tau) continued once per module: (object, result, frequency weights, tau, G, error bar)"""
    if use_complex not in _JOBS:
        if use_complex:
            g = _fixture('complex_elementwise.npz')
            ew = mx.ElementwiseMaxEnt(use_hermiticity=True, use_complex=True)
            G, n_omega, n_alpha = g['G_tau'], 60, 6
        else:
            g = _fixture('elementwise.npz')
            ew = mx.ElementwiseMaxEnt(use_hermiticity=True)
            G, n_omega, n_alpha = g['G_tau_noise'], 80, 8
        ew.set_verbosity(mx.VerbosityFlags.Quiet)
        ew.set_G_tau_data(g['tau'], G)
        ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=n_omega)
        ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=n_alpha)
        ew.set_error(float(g['noise']))
        _JOBS[use_complex] = (ew, ew.run(), np.asarray(ew.omega.delta, dtype=float), g['tau'], G, float(g['noise']))
    return _JOBS[use_complex]


def test_the_reference_outputs():
    g, c = _fixture('elementwise.npz'), _fixture('complex_elementwise.npz')
    out = {}
    for name, A, kw in (('ew', g['ew_A_out'], dict(delta=g['delta'])), ('pm', g['pm_A_out'], dict(delta=g['delta'])),
                        ('herm1', c['herm1_A_out'], dict(omega=c['omega']))):
        got = mx.matrix_positivity(A, keep_vectors=True, **kw)
        ref = R.positivity_ref(A, **kw)
        delta = kw.get('delta', R.trapezoid_delta(c['omega']))
        worst = R.compare_positivity(got, ref, 2, delta)
        assert got['A_psd'].shape == A.shape and got['A_psd'].dtype == A.dtype and got['eigenvectors'].shape == (A.shape[-1], 2, 2)
        assert got['info']['n_matrices'] == A.shape[-1] and got['info']['ms'] > 0 and np.all(got['sweeps'] >= 0)
        assert got['worst_pair'][0] == int(np.argmax(ref['pair_violation'])) and tuple(got['worst_pair'][1:]) == (0, 1)
        print('%s: worst eigenvalue %.4f, %d of %d frequencies negative, negative weight %.5f of %.4f (%.2f %%), worst ratio '
              'to a gate %.3f' % (name, got['min_eigenvalue'].min(), got['n_negative'], A.shape[-1], got['negative_weight'],
                                  got['trace_weight'], 100 * got['negative_fraction'], worst))
        out[name] = got
    assert out['ew']['n_negative'] == 68 and out['pm']['n_negative'] == 67 and out['herm1']['n_negative'] == 50
    assert abs(out['ew']['negative_fraction'] - 0.0595) < 5e-5 and abs(out['pm']['negative_fraction'] - 0.0048) < 5e-5
    assert out['pm']['negative_fraction'] < out['ew']['negative_fraction']


@pytest.mark.parametrize('use_complex', [False, True], ids=['real', 'complex'])
def test_the_method_on_a_continued_job(use_complex):
    ew, res, delta, tau, G, err = _job(use_complex)
    A_out = np.asarray(res.A_out)
    got = ew.positivity(res)
    ref = R.positivity_ref(A_out, delta=delta)
    R.compare_positivity(got, ref, 2, delta)
    assert got['alpha'] == 'LineFitAnalyzer' and np.iscomplexobj(got['A_psd']) == use_complex
    g = R.gate(2)
    # A_psd: Hermitian to the bit, no eigenvalue below the error of an eigenvalue
    P = np.moveaxis(got['A_psd'], (0, 1), (-2, -1))
    assert np.array_equal(P, np.conj(np.swapaxes(P, -1, -2)))
    assert np.all(np.linalg.eigvalsh(P) >= -2 * g * ref['fro'][:, None])
    # every alpha: a leading axis, and the alpha of an index is the row of all
    every = ew.positivity(res, alpha='all')
    n_alpha, n_omega = len(res.alpha), len(delta)
    assert every['eigenvalues'].shape == (n_alpha, n_omega, 2) and every['A_psd'].shape == (2, 2, n_alpha, n_omega)
    assert every['negative_fraction'].shape == (n_alpha,) and every['n_negative'].shape == (n_alpha,)
    assert every['worst_pair'].shape == (n_alpha, 3) and every['alpha'] == 'all' and 'chi2' not in every
    A_all = np.array(res.A)
    if use_complex:
        assert np.all(np.isnan(A_all[[0, 1], [0, 1], 1])) and np.isnan(A_all).sum() == 2 * n_alpha * n_omega
        A_all[[0, 1], [0, 1], 1] = 0.0                                # the imaginary parts of the diagonal: zero elements
        A_all = A_all[:, :, 0] + 1j * A_all[:, :, 1]
    R.compare_positivity(every, R.positivity_ref(A_all, delta=delta), 2, delta)
    k = 3
    one = ew.positivity(res, alpha=k)
    assert one['alpha'] == k
    for name in ('eigenvalues', 'min_eigenvalue', 'pair_violation', 'distance', 'asymmetry', 'sweeps', 'negative_weight',
                 'trace_weight', 'negative_fraction', 'n_negative', 'trace_weight_psd'):
        assert np.array_equal(np.asarray(every[name])[k], one[name]), name
    assert np.array_equal(every['A_psd'][:, :, k], one['A_psd']) and tuple(every['worst_pair'][k]) == tuple(one['worst_pair'])
    # where every element took the analyzer's alpha at the same index, alpha=None is that row, bit for bit
    idx = set()
    for key in (((0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0)) if use_complex else ((0, 0), (0, 1), (1, 1))):
        ana = res.analyzer_results
        for i in key:
            ana = ana[i]
        idx.add(int(ana['LineFitAnalyzer']['alpha_index']))
    print('the alpha indices of the elements: %s; negative fraction per alpha: %s' % (sorted(idx), every['negative_fraction']))
    if len(idx) == 1:
        k = idx.pop()
        for name in ('eigenvalues', 'pair_violation', 'distance', 'negative_weight'):
            assert np.array_equal(np.asarray(every[name])[k], got[name]), name
        assert np.array_equal(every['A_psd'][:, :, k], got['A_psd'])
    # back-continuation: the longhand of chi2 in the element's own data space
    Kd = np.asarray(ew.maxent_diagonal.K.K_delta)
    shape = (2, 2, 2) if use_complex else (2, 2)
    assert got['chi2'].shape == shape and got['chi2_psd'].shape == shape and got['G_rec_psd'].shape == shape + (Kd.shape[0],)
    for i, j in ((0, 0), (0, 1), (1, 1)):                                 # the elements that were computed
        for c in ((0, 1) if use_complex else (None,)):
            key = (i, j) if c is None else (i, j, c)
            if c == 1 and i == j:
                assert np.isnan(got['chi2'][key])                         # never computed: a zero element
                continue
            part = (lambda x: x.real) if c in (None, 0) else (lambda x: x.imag)
            for name, X in (('chi2', A_out), ('chi2_psd', got['A_psd'])):
                long = np.sum(((np.dot(Kd, part(X[i, j])) - part(G[i, j])) / err) ** 2)
                assert abs(got[name][key] - long) <= 1e-12 * long, (name, key)
            np.testing.assert_allclose(got['G_rec_psd'][key], np.dot(Kd, part(got['A_psd'][i, j])), rtol=0, atol=1e-14)
    assert np.all(got['chi2_psd'][np.isfinite(got['chi2_psd'])] > 0)
    # the hermitian partner is filled from the element it follows from, its imaginary part with the other sign
    assert np.array_equal(got['chi2'][1, 0], got['chi2'][0, 1]) and np.array_equal(got['chi2_psd'][1, 0], got['chi2_psd'][0, 1])
    sign = np.array([1.0, -1.0])[:, None] if use_complex else 1.0
    assert np.array_equal(got['G_rec_psd'][1, 0], sign * got['G_rec_psd'][0, 1])
    print('chi2 -> chi2_psd per element:', np.round(got['chi2'].ravel(), 2), np.round(got['chi2_psd'].ravel(), 2))
    # a result made from other data is refused
    other = mx.ElementwiseMaxEnt(use_hermiticity=True, use_complex=use_complex)
    other.set_verbosity(mx.VerbosityFlags.Quiet)
    other.set_G_tau_data(tau, 0.5 * G)
    other.omega, other.alpha_mesh = ew.omega, ew.alpha_mesh
    other.set_error(err)
    with pytest.raises(ValueError, match='not made from the data'):
        other.positivity(res)
    assert 'chi2' not in other.positivity(res, back_continue=False)


def test_an_element_that_was_not_continued_is_named():
    g = _fixture('elementwise.npz')
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(g['tau'][::5], g['G_tau_noise'][:, :, ::5])
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=40)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    ew.set_error(float(g['noise']))
    res = ew.run_diagonal()
    with pytest.raises(ValueError, match=r'element \(0, 1\)'):
        ew.positivity(res)


def test_an_exactly_positive_matrix():
    tau, omega, K, G, A_mat = synthetic.matrix_G(3, 40, 60)
    delta = np.asarray(omega.delta, dtype=float)
    got = mx.matrix_positivity(A_mat, omega=omega)
    ref = R.positivity_ref(A_mat, delta=delta)
    R.compare_positivity(got, ref, 3, delta)
    g = R.gate(3)
    assert got['n_negative'] == 0
    assert np.all(R.fro(np.moveaxis(got['A_psd'] - A_mat, (0, 1), (-2, -1))) <= 4 * g * ref['fro'] + np.finfo(float).tiny)
    assert got['negative_fraction'] <= 4 * g * 3
    # a job whose A_out is that matrix: the repair costs nothing
    ew = mx.ElementwiseMaxEnt(use_hermiticity=True)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(tau, G)
    ew.omega = omega
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    ew.set_error(synthetic.SIGMA)
    res = ew.run()
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(type(res), 'get_A_out', lambda self, analyzer=None: np.array(A_mat))
        out = ew.positivity(res)
    finally:
        mp.undo()
    assert out['n_negative'] == 0
    ok = np.isfinite(out['chi2'])
    assert ok.all()
    # to rounding: an element of A_psd - A is within 4 g || A(omega) ||_F at every frequency, so the residuals differ by at
    # most || K_delta ||_2 sqrt(n_omega) 4 g max || A ||_F, and the roots of chi2 by that over the error bar
    Kd = np.asarray(ew.maxent_diagonal.K.K_delta)
    bound = np.linalg.norm(Kd, 2) * np.sqrt(len(delta)) * 4 * g * ref['fro'].max() / synthetic.SIGMA
    assert np.all(np.abs(np.sqrt(out['chi2_psd']) - np.sqrt(out['chi2'])) <= bound), (out['chi2'], out['chi2_psd'], bound)
    print('exactly positive: chi2 %s, chi2_psd - chi2 %s' % (out['chi2'].ravel(), (out['chi2_psd'] - out['chi2']).ravel()))


def test_chi2_after_set_cov():
    g = _fixture('elementwise.npz')
    tau, G = g['tau'][::5], g['G_tau_noise'][:, :, ::5]
    n = len(tau)
    rng = np.random.RandomState(3)
    B = rng.randn(n, n)
    cov = float(g['noise']) ** 2 * (np.eye(n) + 0.05 * np.dot(B, B.T) / n)
    ew = mx.ElementwiseMaxEnt(use_hermiticity=True)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(tau, G)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=40)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    ew.set_cov(cov)
    res = ew.run()
    got = ew.positivity(res)
    T, err = ew.maxent_diagonal.K.rotation, np.asarray(ew.maxent_diagonal.maxent_loop.err, dtype=float)
    assert T is not None
    Kd = np.asarray(ew.maxent_diagonal.K.K_delta)
    A_out = np.asarray(res.A_out)
    for i, j in ((0, 0), (0, 1), (1, 1)):
        for name, X in (('chi2', A_out), ('chi2_psd', got['A_psd'])):
            long = np.sum((np.dot(T, np.dot(Kd, X[i, j]) - G[i, j]) / err) ** 2)
            assert abs(got[name][i, j] - long) <= 1e-11 * long, (name, i, j, got[name][i, j], long)
    assert got['chi2'][1, 0] == got['chi2'][0, 1] and got['chi2_psd'][1, 0] == got['chi2_psd'][0, 1]
    # the fit itself: chi2 of A_out is the chi2 of the alpha the analyzer picked
    k = int(res.analyzer_results[0][0]['LineFitAnalyzer']['alpha_index'])
    assert abs(got['chi2'][0, 0] - res.chi2[0, 0, k]) <= 1e-6 * res.chi2[0, 0, k]
