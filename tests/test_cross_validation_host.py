"""k-fold cross-validation of alpha, the part that needs no GPU: the table of folds, the pick rules, the weights, the layout
of what the drivers return and what they attach to a result (the device calls replaced by numpy), and the refusals that
come before the library is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import cross_validation as cv, device
import cv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'mxe_cv_score' in names
    assert 'int  mxe_cv_score(' in header and 'extern "C" int mxe_cv_score(' in source
    assert 'mxe_cv.hip.h' in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')).read()
    assert hasattr(device.DeviceContext, 'cv_score')
    assert mx.cross_validation_score is cv.cross_validation_score and mx.fold_counts is cv.fold_counts
    for cls in (mx.TauMaxEnt, mx.ElementwiseMaxEnt, mx.DiagonalMaxEnt, mx.PoormanMaxEnt):
        assert hasattr(cls, 'cross_validate')


# ---- the folds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_bins,n_folds', [(4, 2), (10, 5), (32, 4), (33, 4), (35, 4), (7, 3), (101, 10)])
def test_fold_counts(n_bins, n_folds):
    c = cv.fold_counts(n_bins, n_folds)
    K = n_folds
    assert c.shape == (1 + 2 * K, n_bins) and c.dtype == np.int32
    assert np.all(c[0] == 1)
    train, val = c[1:1 + K], c[1 + K:]
    assert np.all((val == 0) | (val == 1))
    assert np.all(val.sum(axis=0) == 1)                                   # every bin is in exactly one validation row
    assert np.all(train + val == 1)
    sizes = val.sum(axis=1)
    assert sizes.max() - sizes.min() <= 1 and sizes.sum() == n_bins
    for f in range(K):                                                    # contiguous, in the order of the bins
        inside = np.flatnonzero(val[f])
        assert np.all(np.diff(inside) == 1)
        if f:
            assert inside[0] == np.flatnonzero(val[f - 1])[-1] + 1
    np.testing.assert_array_equal(c, cv_ref.fold_table(n_bins, n_folds))
    assert cv.fold_ranges(n_bins, n_folds) == cv_ref.fold_ranges(n_bins, n_folds)


@pytest.mark.parametrize('n_bins,n_folds', [(10, 1), (10, 0), (10, -2), (10, 6), (3, 2), (1, 1)])
def test_fold_counts_refuses(n_bins, n_folds):
    with pytest.raises(ValueError, match='folds'):
        cv.fold_counts(n_bins, n_folds)


# ---- the pick rules ------------------------------------------------------------------------------------------------------
def test_pick_takes_the_minimum_of_the_mean():
    alpha = np.array([100.0, 10.0, 1.0, 0.1])                             # (in visiting order: descending)
    fs = np.array([[9.0, 2.0, 1.0, 3.0], [7.0, 4.0, 2.0, 5.0]])
    p = cv.pick(alpha, fs)
    np.testing.assert_allclose(p['score'], [8.0, 3.0, 1.5, 4.0])
    np.testing.assert_allclose(p['score_err'], np.std(fs, axis=0, ddof=1) / np.sqrt(2.0))
    assert p['alpha_index_cv'] == 2 and not p['alpha_at_edge']
    # one-standard-error rule: score <= 1.5 + 0.5 -> only the minimum itself
    assert p['alpha_index_one_se'] == 2


def test_pick_one_standard_error_goes_to_the_larger_alpha():
    alpha = np.array([100.0, 10.0, 1.0, 0.1])
    fs = np.array([[9.0, 1.2, 0.5, 3.0], [7.0, 2.0, 1.5, 5.0]])             # score 8, 1.6, 1.0, 4; err at the minimum 0.5
    p = cv.pick(alpha, fs)
    assert p['alpha_index_cv'] == 2
    assert p['alpha_index_one_se'] == 2                                   # 1.6 > 1.0 + 0.5: the minimum itself
    fs[:, 1] = [0.9, 2.0]                                                  # 1.45 <= 1.0 + 0.5: in, and alpha 10 > alpha 1
    p = cv.pick(alpha, fs)
    assert p['alpha_index_cv'] == 2 and p['alpha_index_one_se'] == 1
    # an ascending mesh: the larger alpha is the later index
    p = cv.pick(alpha[::-1], fs[:, ::-1])
    assert p['alpha_index_cv'] == 1 and p['alpha_index_one_se'] == 2


def test_pick_ties_go_to_the_larger_alpha():
    fs = np.array([[5.0, 1.0, 1.0, 1.0, 6.0], [5.0, 1.0, 1.0, 1.0, 6.0]])
    down = np.array([1e4, 1e3, 1e2, 1e1, 1e0])
    assert cv.pick(down, fs)['alpha_index_cv'] == 1
    assert cv.pick(down[::-1], fs)['alpha_index_cv'] == 3
    assert cv.pick(down, fs)['alpha_index_one_se'] == 1


def test_pick_leaves_out_an_alpha_with_a_nan_fold():
    alpha = np.array([100.0, 10.0, 1.0, 0.1])
    fs = np.array([[9.0, 2.0, 0.1, 3.0], [7.0, 4.0, np.nan, 5.0]])
    p = cv.pick(alpha, fs)
    assert p['alpha_index_cv'] == 1 and np.isnan(p['score'][2]) and np.isnan(p['score_err'][2])
    assert np.isfinite(p['score'][[0, 1, 3]]).all()
    fs[0, 1] = np.inf
    assert cv.pick(alpha, fs)['alpha_index_cv'] == 3 and cv.pick(alpha, fs)['alpha_at_edge']


def test_pick_without_a_finite_alpha():
    p = cv.pick(np.array([10.0, 1.0]), np.full((3, 2), np.nan))
    assert p['alpha_index_cv'] == -1 and p['alpha_index_one_se'] == -1 and not p['alpha_at_edge']
    assert np.all(np.isnan(p['score']))


def test_pick_alpha_at_edge():
    alpha = np.array([100.0, 10.0, 1.0])
    assert cv.pick(alpha, [[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])['alpha_at_edge']
    assert cv.pick(alpha, [[3.0, 2.0, 1.0], [3.0, 2.0, 1.0]])['alpha_at_edge']
    assert not cv.pick(alpha, [[3.0, 1.0, 2.0], [3.0, 1.0, 2.0]])['alpha_at_edge']


# ---- the weights ---------------------------------------------------------------------------------------------------------
def test_weights_make_the_score_of_the_truth_a_chi2():
    """Bins drawn from N(K H0, diag(s^2)); at H = H0 the validation residual of fold f along direction k is the noise of the
    mean of N_f bins, variance s_k^2 / N_f, and w = N_f / (N sigma_k^2) with sigma_k^2 = s_k^2 / N (here: estimated from
    the bins, as ``bin_statistics`` does) is its inverse.  The K fold scores are independent chi^2 of ``rank`` degrees of
    freedom each, so their mean over the folds divided by rank has the standard deviation sqrt(2 / (K rank)); the test
    asks for 5 of them.  N = 400 bins, n_data = 50, K = 5 and the seed 20261021 are chosen so that the estimate of sigma
    (relative error sqrt(2 / 399) = 7 % per direction, a bias of (N - 1) / (N - 3) = 0.5 % on the score) stays far inside
    the bound 5 sqrt(2 / 250) = 0.45; the value found is printed."""
    N, n_data, n_omega, K = 400, 50, 30, 5
    rng = np.random.RandomState(20261021)
    Kmat = rng.randn(n_data, n_omega)
    H0 = rng.rand(n_omega) / n_omega
    s = 0.01 * (1.0 + rng.rand(n_data))
    bins = Kmat @ H0 + s * rng.randn(N, n_data)
    sigma = np.std(bins, axis=0, ddof=1) / np.sqrt(N)                     # the error of the full-sample mean
    ranges = cv_ref.fold_ranges(N, K)
    w = cv.fold_weights(sigma, N, ranges)
    assert w.shape == (K, n_data)
    scores = []
    for f, (a, b) in enumerate(ranges):
        np.testing.assert_allclose(w[f], (b - a) / (N * sigma ** 2), rtol=1e-15)
        z, sc, _ = cv_ref.score(H0[None], Kmat, bins[a:b].mean(axis=0), w[f])
        scores.append(float(sc[0]))
    value = np.mean(scores) / n_data
    print('mean fold score / rank = %.4f' % value)
    assert abs(value - 1.0) <= 5.0 * np.sqrt(2.0 / (K * n_data))


# ---- the drivers with the device replaced ----------------------------------------------------------------------------------
def _eig(bins, threshold, device=0):
    """numpy in place of ``device.bins_eig`` for 2-d bins: ascending eigenvalues of the covariance of the mean"""
    b = np.asarray(bins, dtype=float)
    n = b.shape[0]
    mean = b.mean(axis=0)
    X = (b - mean) / np.sqrt(n * (n - 1.0))
    lam, vec = np.linalg.eigh(X.T @ X)
    keep = device_keep(lam, threshold, n, b.shape[1])
    return dict(mean=mean, sigma=np.sqrt(lam[keep]), T=np.ascontiguousarray(vec[:, keep].T), rank=int(keep.sum()), sweeps=1)


def device_keep(lam, threshold, n_bins, n_data):
    return device.bins_keep(lam, threshold, n_bins, n_data)


def _resample(bins, counts, T, rank, device=0, want_dev=True, timing=None):
    b = np.asarray(bins, dtype=float)
    c = np.asarray(counts, dtype=float)
    means = (c @ b) / c.sum(axis=1)[:, None]
    G = means @ np.asarray(T, dtype=float).reshape(b.shape[1], b.shape[1]).T
    G[:, int(rank):] = 0.0
    return dict(mean=b.mean(axis=0), G=G)


N_BINS, N_TAU, N_FOLDS = 20, 6, 4


def _bins():
    rng = np.random.RandomState(3)
    tau = np.linspace(0.0, 10.0, N_TAU)
    G = -0.5 * (np.exp(-tau) + np.exp(tau - 10.0))
    return tau, G[None, :] + 1e-3 * rng.randn(N_BINS, N_TAU)


@pytest.fixture
def loaded(monkeypatch):
    """a TauMaxEnt that holds bins, the eigenbasis from numpy"""
    monkeypatch.setattr(device, 'bins_eig', _eig)
    tau, bins = _bins()
    tm = mx.TauMaxEnt(alpha_mesh=mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e2, n_points=5))
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.set_G_tau_bins(tau, bins)
    return tm, bins


def _fake_elements(seen):
    def fake(K, omega, loop, templates, G_rows, G_val, weights, T, rank, ranges, n_bins, device_ids=None, keep_rows=False):
        seen.update(G_rows=G_rows, G_val=G_val, weights=weights, T=T, rank=rank, ranges=ranges, n_bins=n_bins)
        outs = []
        n_omega = len(omega)
        for e, spec in enumerate(templates):
            alpha = np.asarray(spec['alpha'], dtype=float)
            # score 9, 1.2, 1.0 +- 0.26, 3, 8: the minimum at index 2, index 1 (the larger alpha) within one standard error
            fs = np.array([[9.0, 1.2, 1.0, 3.0, 8.0]] * len(ranges)) + 0.4 * (np.arange(len(ranges)) - 1.5)[:, None] * (np.arange(5) == 2)
            o = dict(alpha=alpha, fold_scores=fs)
            o.update(cv.pick(alpha, fs))
            o.update(train_chi2=np.ones_like(fs), left_out=[], folds=np.array(ranges), A_cv=np.full(n_omega, 1.0 + e),
                     A_one_se=np.full(n_omega, 2.0 + e), z=np.zeros((len(ranges), int(rank[e]))), calibration=0.0)
            outs.append(o)
        return outs, dict(kernel_ms=1.0, score_ms=0.5, launches=1, score_launches=2, devices=[0], alpha_train_factor=0.75)
    return fake


def test_what_the_tau_driver_hands_down_and_returns(loaded, monkeypatch):
    tm, bins = loaded
    seen = {}
    monkeypatch.setattr(device, 'bins_resample', _resample)
    monkeypatch.setattr(cv, 'element_cross_validation', _fake_elements(seen))
    st = tm.bin_statistics
    r = st['rank']
    t = {}
    out = tm.cross_validate(bins, n_folds=N_FOLDS, timing=t)
    ranges = cv_ref.fold_ranges(N_BINS, N_FOLDS)
    assert seen['ranges'] == ranges and seen['n_bins'] == N_BINS
    assert seen['G_rows'][0].shape == (1 + N_FOLDS, r) and seen['G_val'][0].shape == (N_FOLDS, N_TAU)
    assert seen['weights'][0].shape == (N_FOLDS, N_TAU) and seen['T'][0].shape == (N_TAU, N_TAU)
    for f, (a, b) in enumerate(ranges):
        outside = np.ones(N_BINS, dtype=bool)
        outside[a:b] = False
        np.testing.assert_allclose(seen['G_rows'][0][1 + f], st['T'] @ bins[outside].mean(axis=0), rtol=0, atol=1e-14)
        np.testing.assert_allclose(seen['G_val'][0][f, :r], st['T'] @ bins[a:b].mean(axis=0), rtol=0, atol=1e-14)
        np.testing.assert_allclose(seen['weights'][0][f, :r], (b - a) / (N_BINS * st['sigma'] ** 2), rtol=1e-15)
        assert not np.any(seen['weights'][0][f, r:]) and not np.any(seen['G_val'][0][f, r:])
    np.testing.assert_allclose(seen['G_rows'][0][0], st['T'] @ bins.mean(axis=0), rtol=0, atol=1e-14)
    for key in ('alpha', 'fold_scores', 'score', 'score_err', 'train_chi2', 'alpha_index_cv', 'alpha_index_one_se', 'alpha_at_edge',
                'A_cv', 'A_one_se', 'z', 'calibration', 'left_out', 'folds', 'info'):
        assert key in out, key
    assert out['fold_scores'].shape == (N_FOLDS, 5) and out['score'].shape == (5,) and out['alpha_index_cv'] == 2
    assert out['rule'] == 'min' and out['n_folds'] == N_FOLDS
    for key in ('kernel_ms', 'score_ms', 'launches', 'devices', 'alpha_train_factor', 'resample_ms'):
        assert key in out['info'], key
    assert t['ms'] == pytest.approx(1.5) and t['score_ms'] == 0.5


def test_attach_adds_an_analyzer_entry(loaded, monkeypatch):
    tm, bins = loaded
    monkeypatch.setattr(device, 'bins_resample', _resample)
    monkeypatch.setattr(cv, 'element_cross_validation', _fake_elements({}))
    spec = tm.maxent_loop.make_spec()
    for rule, index, level in (('min', 2, 1.0), ('one_se', 1, 2.0)):
        res = mx.MaxEntResult()
        res.add_element_results(dict(alpha=np.array(spec['alpha'])))
        out = tm.cross_validate(bins, n_folds=N_FOLDS, rule=rule, result=res)
        entry = res.analyzer_results['CrossValidationAnalyzer']
        assert entry['name'] == 'CrossValidationAnalyzer' and entry['alpha_index'] == index and entry['rule'] == rule
        assert out['alpha_index_cv'] == 2 and out['alpha_index_one_se'] == 1
        np.testing.assert_array_equal(entry['A_out'], np.full(len(tm.omega), level))
        np.testing.assert_array_equal(res.get_A_out('CrossValidationAnalyzer'), entry['A_out'])
        assert entry.maxent_result is res
    # an element-wise result: the entry goes to the element's own table, beside what is there
    res = mx.MaxEntResult(matrix_structure=(2, 2), element_wise=True, complex_elements=True)
    o = dict(out)
    res._analysis[(0, 1, 1)] = dict(LineFitAnalyzer='kept')
    cv.attach(res, (0, 1, 1), o, 'min')
    cv.attach(res, (0, 0, 0), o, 'one_se')
    assert res.analyzer_results[0][1][1]['LineFitAnalyzer'] == 'kept'
    assert res.analyzer_results[0][1][1]['CrossValidationAnalyzer']['alpha_index'] == 2
    assert res.analyzer_results[0][0][0]['CrossValidationAnalyzer']['alpha_index'] == 1
    # no alpha with all its folds: nothing is attached
    res = mx.MaxEntResult()
    cv.attach(res, None, dict(o, alpha_index_cv=-1), 'min')
    assert 'CrossValidationAnalyzer' not in res.analyzer_results


# ---- refusals before the library is touched ---------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(device, 'load_library', refuse)
    monkeypatch.setattr(device, 'device_count', refuse)


def test_refusals_before_the_library(loaded, no_library):
    tm, bins = loaded
    fresh = mx.TauMaxEnt()
    fresh.set_verbosity(mx.VerbosityFlags.Quiet)
    tau = np.linspace(0.0, 10.0, N_TAU)
    fresh.set_G_tau_data(tau, bins.mean(axis=0))
    fresh.set_error(1e-3)
    with pytest.raises(ValueError, match='no bins'):
        fresh.cross_validate(bins)
    with pytest.raises(ValueError, match='no bins'):
        mx.ElementwiseMaxEnt().cross_validate(np.zeros((N_BINS, 2, 2, N_TAU)))
    with pytest.raises(ValueError, match='no bins'):
        mx.DiagonalMaxEnt().cross_validate(np.zeros((N_BINS, 2, 2, N_TAU)))
    with pytest.raises(NotImplementedError, match='default model'):
        mx.PoormanMaxEnt().cross_validate(np.zeros((N_BINS, 2, 2, N_TAU)))
    with pytest.raises(ValueError, match='rule'):
        tm.cross_validate(bins, rule='best')
    with pytest.raises(ValueError, match='rule'):
        mx.ElementwiseMaxEnt().cross_validate(np.zeros((N_BINS, 2, 2, N_TAU)), rule=None)
    for k in (1, 0, N_BINS // 2 + 1):
        with pytest.raises(ValueError, match='folds'):
            tm.cross_validate(bins, n_folds=k)
    with pytest.raises(ValueError, match='bins of shape'):
        tm.cross_validate(bins[:-1])
    with pytest.raises(ValueError, match='cross_validate'):
        tm.cross_validate(bins[0])
    # a result of another alpha mesh
    spec = tm.maxent_loop.make_spec()
    for other in (np.array(spec['alpha'])[:-1], 2.0 * np.array(spec['alpha'])):
        res = mx.MaxEntResult()
        res.add_element_results(dict(alpha=other))
        with pytest.raises(ValueError, match='alphas of the result'):
            tm.cross_validate(bins, result=res)
    assert 'CrossValidationAnalyzer' not in res.analyzer_results

    # a user-supplied minimiser works on one cost function at a time
    class Mine(object):
        def minimize(self, function, v0):
            return v0
    tm.minimizer = Mine()
    with pytest.raises(NotImplementedError, match='Minimizer'):
        tm.cross_validate(bins)
