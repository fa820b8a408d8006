"""Parametric bootstrap, the part that needs no GPU: the host mirror of the mock-data generator, the p-value, the two
entry points, and the refusals of ``parametric_bootstrap`` / ``resample_errors(quantiles=)`` that come before the device
is touched."""
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device, mock, posterior, resampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(n_data, n_omega, seed=0):
    rng = np.random.RandomState(seed)
    K = rng.randn(n_data, n_omega)
    H0 = rng.rand(n_omega) / n_omega
    err = 0.01 * (1.0 + rng.rand(n_data))
    return K, H0, err


def test_both_entry_points_are_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    for name in ('mxe_mock_data', 'mxe_resample_quantiles'):
        assert name in names
        assert ('int  %s(' % name) in header
        assert ('extern "C" int %s(' % name) in source
    assert 'mxe_mock.hip.h' in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')).read()
    assert ('#define MXE_QUANTILE_MAX_ROWS %d' % device.QUANTILE_MAX_ROWS) in header
    assert device.QUANTILE_MAX_ROWS >= 1024


def test_mock_rows_draw_the_numbers_of_the_generator():
    seed, stream, n_mock, n_data = 11, 5, 7, 10
    K, H0, err = _problem(n_data, 23)
    G = mock.mock_rows(K, H0, err, seed, stream, n_mock)
    z = posterior.sample_normals(seed, stream, n_mock, n_data)
    m = K.dot(H0)
    assert G.shape == (n_mock, n_data)
    for k in range(n_mock):
        np.testing.assert_array_equal(G[k], m + err * z[k])
    # another stream, other numbers
    assert not np.array_equal(G, mock.mock_rows(K, H0, err, seed, stream + 1, n_mock))
    # a prefix of n_mock gives a prefix of the rows
    np.testing.assert_array_equal(mock.mock_rows(K, H0, err, seed, stream, 3), G[:3])
    # an odd n_data cuts the last Box-Muller pair and changes nothing else
    odd = mock.mock_rows(K[:9], H0, err[:9], seed, stream, n_mock)
    np.testing.assert_array_equal(odd, G[:, :9])
    # a scalar error bar
    np.testing.assert_array_equal(mock.mock_rows(K, H0, 0.5, seed, stream, 2), m + 0.5 * z[:2])


def test_mock_rows_with_a_rotation():
    seed, stream, n_mock, n_data, rank = 3, 2, 4, 9, 6
    K, H0, err = _problem(n_data, 17, seed=1)
    Q = np.linalg.qr(np.random.RandomState(4).randn(n_data, n_data))[0]
    T = np.zeros((n_data, n_data))
    T[:rank] = Q[:rank]
    G = mock.mock_rows(K, H0, err, seed, stream, n_mock, T=T, rank=rank)
    z = posterior.sample_normals(seed, stream, n_mock, n_data)
    assert np.all(G[:, rank:] == 0.0)                    # rows >= rank are zero
    np.testing.assert_array_equal(G[:, :rank], T[:rank].dot(K.dot(H0)) + (err * z)[:, :rank])
    # the kept rows alone (rank, n_data) are taken as well as the padded matrix
    np.testing.assert_array_equal(mock.mock_rows(K, H0, err, seed, stream, n_mock, T=T[:rank], rank=rank), G)
    with pytest.raises(ValueError):
        mock.mock_rows(K, H0, err, seed, stream, n_mock, T=T)
    with pytest.raises(ValueError):
        mock.mock_rows(K, H0, err, seed, stream, n_mock, T=T, rank=n_data + 1)


def test_moments_of_4096_mocks():
    """(G - K H0) / err pooled over 4096 mocks of one set: the bounds of test_moments_of_65536_normals on N = 4096 x 16"""
    n_mock, n_data = 4096, 16
    K, H0, err = _problem(n_data, 31, seed=2)
    G = mock.mock_rows(K, H0, err, 20261019, 1, n_mock)
    z = ((G - K.dot(H0)) / err).ravel()
    n = len(z)
    assert n == n_mock * n_data
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)


def test_chi2_p_value():
    assert mock.chi2_p_value(3.0, [1.0, 2.0, 3.0, 4.0]) == (1 + 2) / 5.0
    assert mock.chi2_p_value(0.0, [1.0, 2.0]) == 1.0
    assert mock.chi2_p_value(9.0, [1.0, 2.0, 3.0]) == 1 / 4.0           # never 0
    # entries that are not finite are left out of both counts
    assert mock.chi2_p_value(3.0, [1.0, np.nan, 5.0, np.inf, 3.0]) == (1 + 2) / 4.0
    assert mock.chi2_p_value(3.0, [np.nan, np.nan]) == 1.0
    assert mock.chi2_p_value(3.0, []) == 1.0
    assert np.isnan(mock.chi2_p_value(np.nan, [1.0, 2.0]))
    assert mock.chi2_p_value(2.0, np.array([[1.0, 2.0], [3.0, np.nan]])) == (1 + 2) / 4.0


def test_spread_scale_of_the_parametric_bootstrap():
    for n in (2, 7, 200):
        assert resampling.spread_scale('parametric', n) == 1.0 / (n - 1.0) == resampling.spread_scale('bootstrap', n)
    assert resampling.spread_scale('parametric', 1) == 1.0 and resampling.spread_scale('parametric', 0) == 1.0


def _loaded():
    tau = np.linspace(0.0, 10.0, 12)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.set_G_tau_data(tau, -0.5 * (np.exp(-tau) + np.exp(tau - 10.0)))
    tm.set_error(1e-3)
    return tm


def test_refusals_before_the_device():
    tm = _loaded()
    with pytest.raises(ValueError, match='seed'):
        tm.parametric_bootstrap()
    for n in (0, 1, None):
        with pytest.raises(ValueError, match='n_mock'):
            tm.parametric_bootstrap(n_mock=n, seed=1)
    for q in ([-0.1], [0.5, 1.5], [np.nan], []):
        with pytest.raises(ValueError, match='quantiles'):
            tm.parametric_bootstrap(seed=1, quantiles=q)
    with pytest.raises(ValueError, match='quantiles'):
        tm.parametric_bootstrap(seed=1, n_mock=device.QUANTILE_MAX_ROWS + 1)
    for mode in ('per_resample', 'full_sample', None):
        with pytest.raises(ValueError, match='alpha_mode'):
            tm.parametric_bootstrap(seed=1, alpha_mode=mode)
    ew = mx.ElementwiseMaxEnt()
    with pytest.raises(ValueError, match='seed'):
        ew.parametric_bootstrap()
    with pytest.raises(ValueError, match='alpha_mode'):
        ew.parametric_bootstrap(seed=1, alpha_mode='x')
    pm = mx.PoormanMaxEnt()
    with pytest.raises(NotImplementedError, match='default model'):
        pm.parametric_bootstrap(seed=1)

    class Mine(object):
        def minimize(self, function, v0):
            return v0
    tm.minimizer = Mine()
    with pytest.raises(NotImplementedError, match='Minimizer'):
        tm.parametric_bootstrap(seed=1)
    ew.minimizer = Mine()
    with pytest.raises(NotImplementedError, match='Minimizer'):
        ew.parametric_bootstrap(seed=1)


def test_the_jackknife_has_no_quantiles():
    tm = _loaded()
    with pytest.raises(ValueError, match='jackknife'):
        tm.resample_errors(np.zeros((32, 12)), method='jackknife', quantiles=[0.16, 0.84])
    with pytest.raises(ValueError, match='jackknife'):
        mx.ElementwiseMaxEnt().resample_errors(np.zeros((32, 2, 2, 12)), quantiles=[0.5])
    with pytest.raises(ValueError, match='quantiles'):
        tm.resample_errors(np.zeros((32, 12)), method='bootstrap', n_resamples=4, seed=1, quantiles=[2.0])
    assert resampling.check_quantiles(None, 'jackknife', 5) is None
    np.testing.assert_array_equal(resampling.check_quantiles(0.5, 'bootstrap', 5), [0.5])


def test_sets_of_a_phase_with_rotations_of_their_own():
    """elements with their own covariances share the UNROTATED kernel and carry T, rank and padded errors; one rotation
    (or none) for all: the kernel as it stands"""
    tm = _loaded()
    Ku = np.array(tm.K.K)
    i = np.arange(12)
    specs = []
    for rho, thr in ((0.5, 1e-14), (0.3, 1e-6)):
        tm.cov_threshold = thr                              # (the second keeps fewer directions)
        tm.set_cov(1e-6 * rho ** np.abs(i[:, None] - i[None, :]))
        assert tm.K.rotation is not None
        np.testing.assert_array_equal(mock.unrotated_matrix(tm.K), Ku)
        specs.append(tm.maxent_loop.make_spec())
    assert specs[0]['T'].shape[0] == 12 and specs[1]['T'].shape[0] < 12
    K, err, T, rank = mock._phase_sets(dict(worker=tm, templates=specs))
    np.testing.assert_array_equal(K, Ku)
    assert err.shape == (2, 12) and T.shape == (2, 12, 12) and rank.tolist() == [12, specs[1]['T'].shape[0]]
    for s, spec in enumerate(specs):
        r = rank[s]
        np.testing.assert_array_equal(T[s, :r], spec['T'])
        assert not np.any(T[s, r:]) and np.all(err[s, r:] == 1.0)
        np.testing.assert_array_equal(err[s, :r], spec['err'])
        # the data of the job are (to rounding) the rotated unrotated model: T K = the kernel the spec was made with
        np.testing.assert_allclose(T[s, :r] @ Ku, spec['U_rot'] @ np.diag(tm.K.S) @ tm.K.V.T, atol=1e-10)
    K1, err1, T1, rank1 = mock._phase_sets(dict(worker=tm, templates=[specs[1], specs[1]]))
    assert T1 is None and rank1 is None and K1.shape == (rank[1], Ku.shape[1]) and err1.shape == (2, rank[1])
    np.testing.assert_array_equal(K1, tm.K.K)


def test_mock_data_refuses_without_a_launch():
    """what ``device.mock_data`` refuses itself, before the library is asked"""
    K, H0, err = _problem(5, 8)
    for kw in (dict(K=np.where(np.arange(8) == 3, np.nan, K)), dict(H0=np.where(np.arange(8) == 1, np.inf, H0)),
               dict(err=np.where(np.arange(5) == 2, 0.0, err)), dict(err=np.where(np.arange(5) == 2, np.nan, err)),
               dict(n_mock=0), dict(streams=[1, 2]), dict(T=np.eye(5)), dict(T=np.eye(5), rank=[6])):
        a = dict(K=K, H0=H0, err=err, seed=1, streams=[0], n_mock=3)
        a.update(kw)
        with pytest.raises(ValueError):
            device.mock_data(**a)
