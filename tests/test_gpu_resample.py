"""Jackknife / bootstrap resampling on the device: ``mxe_bins_resample`` and ``mxe_resample_reduce`` against their
longdouble restatements (tests/resample_ref.py) with the standard bounds of their sums, and ``resample_errors`` end to
end against a loop of ``run()`` calls over the same resamples through the API without bins
(``set_G_*_data(mean_r)`` + ``set_cov(C)``).  Fixture: tests/golden/bins.npz (make_golden_bins.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, resampling
from resample_ref import bins_resample_ref, reduce_ref, EPS, LD

pytestmark = pytest.mark.gpu

GATE = 1e-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLD, 'bins.npz'))


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def cov_longdouble(bins):
    b = np.asarray(bins, dtype=LD)
    nb = b.shape[0]
    X = (b - b.mean(axis=0)) / np.sqrt(LD(nb) * (nb - 1))
    return np.asarray(X.T @ X, dtype=float), np.asarray(b.mean(axis=0), dtype=float)


def resampled_means(bins, counts):
    """the means of the resamples in longdouble, rounded: (n_res,) + the shape of one bin"""
    b = np.asarray(bins)
    flat = b.reshape(b.shape[0], -1)
    c = np.asarray(counts, dtype=LD)
    W = c / c.sum(axis=1)[:, None]
    if np.iscomplexobj(flat):
        m = np.asarray(W @ flat.real.astype(LD), dtype=float) + 1j * np.asarray(W @ flat.imag.astype(LD), dtype=float)
    else:
        m = np.asarray(W @ flat.astype(LD), dtype=float)
    return m.reshape((len(c),) + b.shape[1:])


# ---- mxe_bins_resample ------------------------------------------------------------------------------------------------
def _sets(rng, n_sets, n_bins, n_data):
    """bins with an offset far above their spread (the deviations are ~1e-3 of the data), orthonormal T, one set of lower rank"""
    bins = 1.0 + rng.rand(n_sets, 1, n_data) + 1e-3 * rng.randn(n_sets, n_bins, n_data) * np.linspace(1.0, 0.1, n_data)
    T = np.stack([np.linalg.qr(rng.randn(n_data, n_data))[0].T for _ in range(n_sets)])
    rank = np.full(n_sets, n_data, dtype=np.int32)
    rank[-1] = n_data // 2
    T[-1, rank[-1]:] = 0.0
    return np.ascontiguousarray(bins), np.ascontiguousarray(T), rank


def _tables(rng, n_bins):
    out = [('multinomial %d' % n, rng.multinomial(n_bins, np.ones(n_bins) / n_bins, size=n).astype(np.int32)) for n in (1, 15, 17)]
    out.append(('jackknife', resampling.jackknife_counts(n_bins, max(1, n_bins // 16))))
    return out


@pytest.mark.parametrize('n_data', [1, 17, 64, 65, 512])
def test_bins_resample_against_longdouble(n_data):
    rng = np.random.RandomState(100 + n_data)
    worst = 0.0
    for n_bins in (2, 3, 63, 65, 1025):
        bins, T, rank = _sets(rng, 3, n_bins, n_data)
        eig = device.bins_eig(bins, 0.0)
        for what, counts in _tables(rng, n_bins):
            got = device.bins_resample(bins, counts, T, rank)
            again = device.bins_resample(bins, counts, T, rank)
            for k in ('mean', 'G', 'dev'):
                assert got[k].tobytes() == again[k].tobytes(), (n_bins, what, k)          # two calls: the same bits
            for s in range(3):
                assert got['mean'][s].tobytes() == eig[s]['mean'].tobytes(), (n_bins, what, s)      # the mean of mxe_bins_eig
                ref = bins_resample_ref(bins[s], counts, T[s], rank[s], mean=got['mean'][s])
                err = np.abs(np.asarray(got['dev'][s] - ref['dev'], dtype=float))
                ok = err <= ref['bound_dev']
                with np.errstate(all='ignore'):
                    ratio = np.nanmax(np.where(ref['bound_dev'] > 0, err / ref['bound_dev'], 0.0))
                worst = max(worst, ratio)
                assert np.all(ok), 'n_bins %d, %s, set %d: dev error / bound = %.3f' % (n_bins, what, s, ratio)
                tm = np.abs(np.asarray((got['G'][s] - got['dev'][s]) - ref['Tmean'][None, :], dtype=float))
                assert np.all(tm <= ref['bound_Tm'][None, :]), (n_bins, what, s)
                assert not np.any(got['G'][s][:, rank[s]:]) and not np.any(got['dev'][s][:, rank[s]:])    # rows >= rank: exact zeros
            # a set alone: the bits it has in the batch
            alone = device.bins_resample(bins[1], counts, T[1], rank[1])
            for k in ('mean', 'G', 'dev'):
                assert alone[k].tobytes() == got[k][1].tobytes(), (n_bins, what, k)
    print('n_data %d: worst dev error / bound = %.3f' % (n_data, worst))


def _raw_resample(n_sets, n_bins, n_data, bins, n_res, counts, T, rank, outs):
    lib = device.load_library()
    return lib.mxe_bins_resample(0, n_sets, n_bins, n_data, bins.ctypes.data_as(DP), n_res, counts.ctypes.data_as(IP),
                                 T.ctypes.data_as(DP), rank.ctypes.data_as(IP), outs[0].ctypes.data_as(DP),
                                 outs[1].ctypes.data_as(DP), outs[2].ctypes.data_as(DP), None)


def test_bins_resample_refuses_bad_arguments_and_touches_nothing():
    rng = np.random.RandomState(3)
    n_sets, n_bins, n_data, n_res = 2, 6, 5, 4
    bins = np.ascontiguousarray(rng.randn(n_sets, n_bins, n_data))
    counts = np.ones((n_res, n_bins), dtype=np.int32)
    T = np.ascontiguousarray(np.stack([np.eye(n_data)] * n_sets))
    rank = np.full(n_sets, n_data, dtype=np.int32)

    def outs(n=n_data):
        return [np.full((n_sets, n), 7.0), np.full((n_sets, n_res, n), 7.0), np.full((n_sets, n_res, n), 7.0)]

    def refused(rc, o):
        return rc == -1 and all(np.all(a == 7.0) for a in o)
    o = outs()
    assert _raw_resample(n_sets, n_bins, n_data, bins, n_res, counts, T, rank, o) == 0 and not np.any(o[1] == 7.0)
    cases = {}
    c = counts.copy(); c[2, 3] = -1
    cases['a negative count'] = dict(counts=c)
    c = counts.copy(); c[1] = 0
    cases['a row of counts that sums to 0'] = dict(counts=c)
    for bad in (-1, n_data + 1):
        r = rank.copy(); r[1] = bad
        cases['rank %d' % bad] = dict(rank=r)
    for v in (np.nan, np.inf):
        b = bins.copy(); b[1, 2, 3] = v
        cases['%s in bins' % v] = dict(bins=b)
        t = T.copy(); t[0, 1, 1] = v
        cases['%s in T' % v] = dict(T=t)
    for name, kw in cases.items():
        a = dict(bins=bins, counts=counts, T=T, rank=rank)
        a.update(kw)
        o = outs()
        assert refused(_raw_resample(n_sets, n_bins, n_data, a['bins'], n_res, a['counts'], a['T'], a['rank'], o), o), name
    o = outs()
    assert refused(_raw_resample(n_sets, n_bins, n_data, bins, 0, counts, T, rank, o), o)          # n_res < 1
    assert refused(_raw_resample(0, n_bins, n_data, bins, n_res, counts, T, rank, o), o)           # the argument errors of mxe_bins_eig
    assert refused(_raw_resample(n_sets, 1, n_data, bins, n_res, counts, T, rank, o), o)
    assert refused(_raw_resample(n_sets, n_bins, 0, bins, n_res, counts, T, rank, o), o)
    big = [np.full((1, 513), 7.0), np.full((1, 2, 513), 7.0), np.full((1, 2, 513), 7.0)]
    rc = _raw_resample(1, 4, 513, np.zeros((1, 4, 513)), 2, np.ones((2, 4), dtype=np.int32), np.zeros((1, 513, 513)),
                       np.zeros(1, dtype=np.int32), big)
    assert refused(rc, big)                                                                      # n_data > 512
    with pytest.raises(ValueError):
        device.bins_resample(bins, c, T, rank)


def test_jackknife_deviations_carry_the_covariance_of_mxe_bins_eig(g):
    """(n - 1) / n sum_r dev[r][k]^2 = sigma_k^2: the jackknife spread of the rotated data IS the eigenvalue"""
    bins = g['s_bins']
    n = bins.shape[0]
    st = device.bins_eig(bins, float(g['cov_threshold']))
    assert st['rank'] == 40
    got = device.bins_resample(bins, resampling.jackknife_counts(n, 1), resampling.padded_T(st, 40), st['rank'])
    ratio = (n - 1.0) / n * np.sum(np.asarray(got['dev'], dtype=LD) ** 2, axis=0) / np.asarray(st['sigma'], dtype=LD) ** 2
    print('jackknife spread / sigma^2 - 1: %.2e .. %.2e' % (float(ratio.min() - 1), float(ratio.max() - 1)))
    assert np.all(np.abs(np.asarray(ratio - 1, dtype=float)) <= 1e-12)


def test_bootstrap_deviations_scatter_like_the_eigenvalues(g):
    """400 draws, seed 0: the sample standard deviation of dev[.][k] / sigma_k is sqrt((n - 1) / n) within five standard
    errors of a standard deviation from 400 draws (5 / sqrt(2 * 399) = 18 %)"""
    bins = g['s_bins']
    n = bins.shape[0]
    st = device.bins_eig(bins, float(g['cov_threshold']))
    got = device.bins_resample(bins, resampling.bootstrap_counts(n, 400, seed=0), resampling.padded_T(st, 40), st['rank'])
    sd = np.std(got['dev'] / st['sigma'][None, :], axis=0, ddof=1)
    want = np.sqrt((n - 1.0) / n)
    print('bootstrap sd / sigma: %.3f .. %.3f against %.3f' % (sd.min(), sd.max(), want))
    assert np.all(np.abs(sd / want - 1.0) <= 0.18)


# ---- mxe_resample_reduce with host rows -------------------------------------------------------------------------------
def _ctx(n_omega):
    n_s = min(n_omega, 4)
    rng = np.random.RandomState(n_omega)
    return device.DeviceContext(rng.randn(6, n_s), np.linspace(1.0, 0.1, n_s), np.linalg.qr(rng.randn(n_omega, n_s))[0])


def _check_reduce(got, ref, groups):
    for gi in groups:
        n = ref['used'][gi]
        assert got['used'][gi] == n
        if n == 0:
            assert np.all(np.isnan(got['mean'][gi])) and np.all(np.isnan(got['var'][gi]))
            continue
        assert np.all(np.abs(np.asarray(got['mean'][gi] - ref['mean'][gi], dtype=float)) <= ref['mean_bound'][gi]), gi
        assert np.all(np.abs(np.asarray(got['fmean'][gi] - ref['fmean'][gi], dtype=float)) <= ref['fmean_bound'][gi]), gi
        if n < 2:
            assert np.all(np.isnan(got['var'][gi])) and np.all(np.isnan(got['fcov'][gi]))
            continue
        assert np.all(np.abs(np.asarray(got['var'][gi] - ref['var'][gi], dtype=float)) <= ref['var_bound'][gi]), gi
        assert np.all(np.abs(np.asarray(got['fcov'][gi] - ref['fcov'][gi], dtype=float)) <= ref['fcov_bound'][gi]), gi
        assert np.array_equal(got['fcov'][gi], got['fcov'][gi].T)
    assert np.all(np.abs(np.asarray(got['fval'] - ref['fval'], dtype=float)) <= ref['fval_bound'])


@pytest.mark.parametrize('n_omega', [1, 63, 64, 65, 513])
def test_reduce_against_longdouble(n_omega):
    rng = np.random.RandomState(7 + n_omega)
    sizes = [0, 1, 2, 3, 17, 64, 65]
    off = np.concatenate([[0], np.cumsum(sizes)])
    H = np.ascontiguousarray(0.5 + rng.rand(int(off[-1]), n_omega) * np.linspace(1.0, 1e-3, n_omega)[None, :])
    ctx = _ctx(n_omega)
    try:
        for method in ('jackknife', 'bootstrap'):
            scale = np.array([resampling.spread_scale(method, s) for s in sizes])
            for n_f in (0, 1, 5):
                F = rng.randn(n_f, n_omega) if n_f else None
                got = ctx.resample_reduce(off, scale, H=H, F=F)
                ref = reduce_ref(H, off, scale, F)
                _check_reduce(got, ref, range(len(sizes)))
                assert got['fcov'].shape == (len(sizes), n_f, n_f) and got['fval'].shape == (H.shape[0], n_f)
                again = ctx.resample_reduce(off, scale, H=H, F=F)
                for k in ('mean', 'var', 'fval', 'fmean', 'fcov', 'used'):
                    assert got[k].tobytes() == again[k].tobytes(), k                      # bitwise repeat
                # a group alone: the bits it has inside the batch
                for gi in (3, 5):
                    sub = ctx.resample_reduce([0, sizes[gi]], scale[gi:gi + 1], H=H[off[gi]:off[gi + 1]], F=F)
                    for k in ('mean', 'var', 'fmean', 'fcov'):
                        assert sub[k][0].tobytes() == got[k][gi].tobytes(), (k, gi)
                    assert sub['fval'].tobytes() == got['fval'][off[gi]:off[gi + 1]].tobytes()
        # only what is asked for comes back
        part = ctx.resample_reduce(off, scale, H=H, want=('var',))
        assert sorted(part) == ['used', 'var'] and part['var'].tobytes() == ctx.resample_reduce(off, scale, H=H)['var'].tobytes()
    finally:
        ctx.close()


def test_reduce_leaves_out_rows_that_are_not_finite():
    rng = np.random.RandomState(5)
    n_omega = 65
    sizes = [3, 3, 3, 4]
    off = np.concatenate([[0], np.cumsum(sizes)])
    H = np.ascontiguousarray(0.5 + rng.rand(13, n_omega))
    F = rng.randn(2, n_omega)
    scale = np.array([2.0 / 3.0] * 3 + [0.75])
    ctx = _ctx(n_omega)
    try:
        clean = ctx.resample_reduce(off, scale, H=H, F=F)
        Hn = H.copy()
        Hn[4, 7] = np.nan                   # one row of group 1
        Hn[6] = np.nan                      # two rows of group 2
        Hn[8, 64] = np.inf
        got = ctx.resample_reduce(off, scale, H=Hn, F=F)
        assert got['used'].tolist() == [3, 2, 1, 4]
        ref = reduce_ref(Hn, off, scale, F)
        assert ref['used'].tolist() == [3, 2, 1, 4]
        _check_reduce(dict(got, fval=np.where(np.isfinite(got['fval']), got['fval'], 0.0)),
                      dict(ref, fval=np.where(np.isfinite(np.asarray(ref['fval'], dtype=float)), ref['fval'], 0.0),
                           fval_bound=np.where(np.isfinite(ref['fval_bound']), ref['fval_bound'], 0.0)), range(4))
        assert np.all(np.isnan(got['var'][2])) and np.all(np.isnan(got['fcov'][2]))
        assert got['mean'][2].tobytes() == Hn[7].tobytes()              # the mean of the one row that is left
        for k in ('mean', 'var', 'fmean', 'fcov'):                      # the other groups are not touched
            for gi in (0, 3):
                assert got[k][gi].tobytes() == clean[k][gi].tobytes()
        # without a launch there are no rows on the device to read
        with pytest.raises(device.MaxEntDeviceError, match='call order'):
            ctx.resample_reduce([0, 2], [0.5], problem_index=[0, 1])
        with pytest.raises(ValueError):
            ctx.resample_reduce([1, 2], [0.5], H=H[:2])
        with pytest.raises(ValueError):
            ctx.resample_reduce([0, 2, 1], [0.5, 0.5], H=H[:2])
    finally:
        ctx.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------
WINDOWS = [(-3.0, 0.0), (0.0, 3.0)]


def _single(g, **kw):
    tm = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), **kw)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    return tm


def _check_against_own_samples(out, delta, rowsH, n_win, n_fun, method='jackknife'):
    """A_mean, A_err, A_bias, window_* and functional_* against the longdouble reduction of the samples of the same call"""
    Hs = out['samples']['H']
    n = Hs.shape[0]
    assert out['n_used'] == n
    ref = reduce_ref(Hs, [0, n], [resampling.spread_scale(method, n)], rowsH)
    d = np.asarray(delta, dtype=LD)
    A_mean, A_var = ref['mean'][0] / d, ref['var'][0] / d ** 2
    # (beyond the reduce gates: the division by delta, the square root and the square taken here, a rounding each)
    assert np.all(np.abs(np.asarray(out['A_mean'] - A_mean, dtype=float)) <= ref['mean_bound'][0] / delta + EPS * np.abs(out['A_mean']))
    assert np.all(np.abs(np.asarray(out['A_err'] ** 2 - A_var, dtype=float)) <= ref['var_bound'][0] / delta ** 2 + 4 * EPS * out['A_err'] ** 2)
    if method == 'jackknife':
        np.testing.assert_array_equal(out['A_bias'], (n - 1) * (out['A_mean'] - out['A']))
    val = np.concatenate([out['window_weight'], out['functional_value']])
    err = np.concatenate([out['window_err'], out['functional_err']])
    assert np.all(np.abs(np.asarray(val - ref['fmean'][0], dtype=float)) <= ref['fmean_bound'][0])
    var_ref = np.asarray(np.diagonal(ref['fcov'][0]), dtype=float)
    assert np.all(np.abs(err ** 2 - var_ref) <= np.diagonal(ref['fcov_bound'][0]) + 4 * EPS * var_ref)
    cov_ref = np.asarray(ref['fcov'][0], dtype=float)[n_win:, n_win:]
    assert np.all(np.abs(out['functional_cov'] - cov_ref) <= ref['fcov_bound'][0][n_win:, n_win:])
    assert np.all(np.abs(np.asarray(out['samples']['functional'] - ref['fval'], dtype=float)) <= ref['fval_bound'])
    assert np.all(err > 0) and np.all(out['A_err'] > 0)


def test_single_element_equals_a_loop_of_runs(g):
    bins, tau = g['s_bins'], g['s_tau']
    tm = _single(g)
    tm.set_G_tau_bins(tau, bins)
    name = tm.analyzers[0].name
    omega = np.asarray(tm.omega)
    F = np.stack([omega, omega ** 2])
    G_before, err_before = np.array(tm.G), np.array(tm.err)
    out = tm.resample_errors(bins, method='jackknife', block=16, windows=WINDOWS, functionals=F, keep_samples=True)
    assert np.array_equal(G_before, tm.G) and np.array_equal(err_before, tm.err)        # the object is as it was
    assert out['n_resamples'] == 16 and out['n_used'] == 16 and out['method'] == 'jackknife'
    assert out['info']['n_datasets'] == 1 and out['info']['left_out'] == []
    assert out['info']['audit_max'] < GATE
    assert out['samples']['H'].shape == (16, 60) and out['samples']['functional'].shape == (16, 4)
    # the reference loop: one fresh object per resample through the API without bins
    C, _ = cov_longdouble(bins)
    counts = resampling.resample_counts('jackknife', 256, block=16)
    means = resampled_means(bins, counts)
    worst = 0.0
    for r in range(17):
        th = _single(g)
        th.set_G_tau_data(tau, means[r])
        th.set_cov(C)
        res = th.run()
        pick = int(res.analyzer_results[name]['alpha_index'])
        assert np.all(res.converged) and th.last_launch['audit_max'] < GATE
        H_loop = np.asarray(res.H)[pick]
        if r == 0:
            assert out['alpha_index'] == pick and out['alpha'] == pytest.approx(float(res.alpha[pick]), rel=1e-13)
            e = rel_l2(out['A'] * tm.omega.delta, H_loop)
        else:
            assert out['alpha_index_samples'][r - 1] == pick, r
            e = rel_l2(out['samples']['H'][r - 1], H_loop)
        worst = max(worst, float(e))
        assert e < GATE, (r, e)
    print('resamples vs loop of run(): worst rel. L2 %.2e, audit of the launch %.2e' % (worst, out['info']['audit_max']))
    # chain 0 is the run() of the object itself
    res = tm.run()
    assert rel_l2(out['A'] * tm.omega.delta, np.asarray(res.H)[out['alpha_index']]) < GATE
    rowsH = np.concatenate([resampling.window_rows(tm.omega, WINDOWS), F])
    _check_against_own_samples(out, tm.omega.delta, rowsH, 2, 2)
    # one alpha for all samples
    fs = tm.resample_errors(bins, block=16, alpha_mode='full_sample', pointwise=True)
    assert np.all(fs['alpha_index_samples'] == fs['alpha_index']) and fs['alpha_index'] == out['alpha_index']
    fx = tm.resample_errors(bins, block=16, alpha=3, windows=WINDOWS)
    assert fx['alpha_index'] == 3 and np.all(fx['alpha_index_samples'] == 3) and fx['n_used'] == 16
    assert fx['alpha'] == pytest.approx(float(res.alpha[3]), rel=1e-13)
    # bins that are not those of the setter: refused before anything is solved
    other = bins.copy()
    other[3, 5] += 1e-9
    with pytest.raises(ValueError, match='mean'):
        tm.resample_errors(other, block=16)
    # bootstrap runs through the same path with its own scale
    bs = tm.resample_errors(bins, method='bootstrap', n_resamples=8, seed=2, windows=WINDOWS, functionals=F, keep_samples=True)
    assert bs['n_resamples'] == 8 and 'A_bias' not in bs
    _check_against_own_samples(bs, tm.omega.delta, rowsH, 2, 2, method='bootstrap')


def test_preblur_refers_to_A(g):
    bins, tau = g['s_bins'], g['s_tau']
    tm = _single(g)
    tm.A_of_H = mx.PreblurA_of_H(b=0.2, omega=tm.omega)
    tm.K = mx.PreblurKernel(K=tm.K, b=0.2)
    tm.set_G_tau_bins(tau, bins)
    out = tm.resample_errors(bins, block=32, windows=WINDOWS, keep_samples=True)
    assert out['n_used'] == 8
    B = tm.maxent_loop.A_of_H.matrix()
    A_s = out['samples']['H'] @ np.asarray(B).T
    np.testing.assert_allclose(out['A_mean'], A_s.mean(axis=0), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(out['A_err'], np.sqrt(7.0 / 8.0 * ((A_s - A_s.mean(axis=0)) ** 2).sum(axis=0)), rtol=1e-8, atol=1e-13)
    inside = resampling.window_rows(tm.omega, WINDOWS)
    np.testing.assert_allclose(out['window_weight'], ((A_s * tm.omega.delta) @ inside.T).mean(axis=0), rtol=1e-10)
    assert 'functional_cov' not in out


def _ew(g, cls=None, herm=True):
    ew = (cls or mx.ElementwiseMaxEnt)(use_hermiticity=herm, cov_threshold=float(g['cov_threshold']))
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    return ew


def test_elementwise_equals_a_loop_of_runs(g):
    bins, tau = g['e_bins'], g['e_tau']
    ew = _ew(g)
    ew.set_G_tau_bins(tau, bins)
    name = ew.maxent_diagonal.analyzers[0].name
    out = ew.resample_errors(bins, block=25, windows=WINDOWS, keep_samples=True)
    info = out['info']
    assert out['n_resamples'] == 8 and info['audit_max'] < GATE
    assert info['n_datasets'] == info['n_elements'] == [2, 1]            # one data set per element of a phase
    assert out['A_err'].shape == (2, 2, 60) and out['window_err'].shape == (2, 2, 2) and out['n_used'].shape == (2, 2)
    assert out['alpha_index_samples'].shape == (2, 2, 8) and out['samples']['H'].shape == (2, 2, 8, 60)
    assert np.all(out['n_used'] == 8)
    for k in ('A', 'A_err', 'A_mean', 'A_bias', 'window_weight', 'window_err', 'alpha_index'):
        np.testing.assert_array_equal(out[k][1, 0], out[k][0, 1])       # the partner from hermiticity
    C = np.empty((2, 2, 30, 30))
    for i in range(2):
        for j in range(2):
            C[i, j] = cov_longdouble(bins[:, i, j, :])[0]
    means = resampled_means(bins, resampling.resample_counts('jackknife', 200, block=25))
    delta = ew.omega.delta
    worst = 0.0
    for r in range(9):
        # (one fresh worker per element, as tests/test_gpu_bins.py has it: a worker that is reused hops from the previous
        #  element's rotation in set_cov, which is the reference's behaviour and not the job of a resample)
        for (i, j) in ((0, 0), (0, 1), (1, 1)):
            th = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), **({} if i == j else dict(cost_function='plusminus')))
            th.set_verbosity(mx.VerbosityFlags.Quiet)
            th.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
            th.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
            th.set_G_tau_data(tau, means[r][i, j])
            th.set_cov(C[i, j])
            res = th.run()
            pick = int(res.analyzer_results[name]['alpha_index'])
            H_loop = np.asarray(res.H)[pick]
            if r == 0:
                assert out['alpha_index'][i, j] == pick
                e = rel_l2(out['A'][i, j] * delta, H_loop)
            else:
                assert out['alpha_index_samples'][i, j, r - 1] == pick, (r, i, j)
                e = rel_l2(out['samples']['H'][i, j, r - 1], H_loop)
            worst = max(worst, float(e))
            assert e < GATE, (r, i, j, e)
    print('element-wise resamples vs loop of run(): worst rel. L2 %.2e, audit of the launches %.2e' % (worst, info['audit_max']))
    rowsH = resampling.window_rows(ew.omega, WINDOWS)
    for (i, j) in ((0, 0), (0, 1), (1, 1)):
        Hs = out['samples']['H'][i, j]
        ref = reduce_ref(Hs, [0, 8], [7.0 / 8.0], rowsH)
        assert np.all(np.abs(np.asarray(out['A_mean'][i, j] - ref['mean'][0] / delta, dtype=float))
                      <= ref['mean_bound'][0] / delta + EPS * np.abs(out['A_mean'][i, j]))
        assert np.all(np.abs(np.asarray(out['window_weight'][i, j] - ref['fmean'][0], dtype=float)) <= ref['fmean_bound'][0])
    # the diagonal driver: the same diagonal, nothing off it
    dg = _ew(g, cls=mx.DiagonalMaxEnt)
    dg.set_G_tau_bins(tau, bins)
    od = dg.resample_errors(bins, block=25, windows=WINDOWS)
    assert od['info']['n_datasets'] == od['info']['n_elements'] == [2]
    assert np.all(np.isnan(od['A_err'][0, 1])) and np.all(np.isnan(od['A_err'][1, 0]))
    for i in range(2):
        assert rel_l2(od['A_mean'][i, i], out['A_mean'][i, i]) < GATE
        np.testing.assert_allclose(od['A_err'][i, i], out['A_err'][i, i], rtol=1e-4)
        np.testing.assert_array_equal(od['alpha_index_samples'][i, i], out['alpha_index_samples'][i, i])


def _iw_bins(g, n_iw=20, n_bins=160, seed=11):
    beta = float(g['s_beta'])
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    iomega = (2 * np.arange(n_iw) + 1) * np.pi / beta
    K = mx.IOmegaKernel(iomega, omega)
    G = (K.K_complex * omega.delta[None, :]) @ g['s_A_true']
    rng = np.random.RandomState(seed)
    z = rng.randn(n_bins, n_iw) + 1j * rng.randn(n_bins, n_iw)
    z[:, 1:] += 0.5 * z[:, :-1]                                         # correlated along the frequency axis
    return iomega, G[None, :] + 2e-3 * z / (1.0 + 0.1 * np.arange(n_iw))[None, :]


def test_matsubara_bins_equal_a_loop_of_runs(g):
    iomega, bins = _iw_bins(g)
    tm = _single(g)
    tm.set_G_iw_bins(iomega, bins)
    name = tm.analyzers[0].name
    out = tm.resample_errors(bins, block=20, windows=WINDOWS, keep_samples=True)
    assert out['n_resamples'] == 8 and out['n_used'] == 8 and out['info']['n_datasets'] == 1
    assert out['info']['audit_max'] < GATE
    stacked = np.concatenate([bins.real, bins.imag], axis=-1)
    C, _ = cov_longdouble(stacked)
    means = resampled_means(stacked, resampling.resample_counts('jackknife', 160, block=20))
    for r in range(9):
        th = _single(g)
        th.set_G_iw_data(iomega, means[r][:20] + 1j * means[r][20:])
        th.set_cov(C)
        res = th.run()
        pick = int(res.analyzer_results[name]['alpha_index'])
        H_loop = np.asarray(res.H)[pick]
        if r == 0:
            assert out['alpha_index'] == pick
            assert rel_l2(out['A'] * tm.omega.delta, H_loop) < GATE
        else:
            assert out['alpha_index_samples'][r - 1] == pick, r
            assert rel_l2(out['samples']['H'][r - 1], H_loop) < GATE, r
    with pytest.raises(ValueError, match='shape'):
        tm.resample_errors(stacked, block=20)                           # the stacked real form is not what the setter received
