"""Binned Monte Carlo data on the device: ``mxe_bins_eig`` against 40-digit truth (tests/golden/bins_truth.npz,
make_golden_bins_truth.py), and ``set_G_tau_bins`` / ``set_G_iw_bins`` end to end against the reference's results for
the mean and the covariance of the same bins (tests/golden/bins.npz, make_golden_bins.py) and against this package's
own host path (``set_G_*_data(mean)`` + ``set_cov(C)``).  The gates of the decomposition are those of
tests/test_gpu_svd_matrices.py."""
import ctypes
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device

pytestmark = pytest.mark.gpu

GATE = 1e-6
EPS = np.finfo(float).eps
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SWEEP_CAP = 60
NAMES = ['well_96x48', 'graded_96x48', 'short_24x40', 'dup_80x36', 'const_64x32']


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


@pytest.fixture(scope='module')
def truth():
    return np.load(os.path.join(GOLD, 'bins_truth.npz'))


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLD, 'bins.npz'))


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def cov_longdouble(bins):
    b = np.asarray(bins, dtype=np.longdouble)
    nb = b.shape[0]
    X = (b - b.mean(axis=0)) / np.sqrt(np.longdouble(nb) * (nb - 1))
    return np.asarray(X.T @ X, dtype=float), np.asarray(b.mean(axis=0), dtype=float)


# ---- the kernel against truth -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_decomposition_against_forty_digit_truth(truth, name):
    bins, S, rank = truth['bins_' + name], truth['S_' + name], int(truth['rank_' + name])
    r = device.bins_eig(bins, 0.0)
    sig = r['sigma'][::-1]                      # descending like the truth
    print('%s: rank %d (true %d), sweeps %d' % (name, r['rank'], rank, r['sweeps']))
    assert r['rank'] == rank == len(sig) and r['T'].shape == (rank, bins.shape[1])
    err = np.abs(sig - S[:rank]).max() / S[0]
    print('   max |sigma - truth| / sigma_max = %.2e' % err)
    assert err <= 1e-12
    assert np.all(np.diff(r['sigma']) >= 0)     # ascending like eigh
    emean = np.abs(r['mean'] - truth['mean_' + name]).max()
    print('   max |mean - truth| = %.2e (2 eps max|bins| = %.2e)' % (emean, 2 * EPS * np.abs(bins).max()))
    assert emean <= 2 * EPS * np.abs(bins).max()
    T = r['T']
    orth = np.abs(T @ T.T - np.eye(rank)).max()
    print('   max |T T^T - 1| = %.2e' % orth)
    assert orth <= 1e-12
    X = np.asarray(truth['X_' + name], dtype=np.longdouble)
    C = np.asarray(X.T @ X, dtype=float)
    dropped = float(S[rank] ** 2) if rank < len(S) else 0.0
    rec = np.linalg.norm(T.T @ (r['sigma'][:, None] ** 2 * T) - C, 2)
    print('   |T^T diag(lambda) T - C|_2 = %.2e lambda_max (dropped: %.2e)' % (rec / S[0] ** 2, dropped / S[0] ** 2))
    assert rec <= 1e-13 * S[0] ** 2 + dropped
    # each eigenvector has its component of largest magnitude positive
    assert np.all(T[np.arange(rank), np.abs(T).argmax(axis=1)] > 0)
    assert 0 < r['sweeps'] < SWEEP_CAP


def test_small_eigenvalues_keep_their_relative_accuracy(truth):
    """column-graded bins, sigma over 10 decades: the device's SVD of X against LAPACK's eigh(C) (which loses everything
    below eps lambda_max) and LAPACK's svd(X); the yardstick is measured here: 4 x the worst relative error of svd(X)"""
    name = 'graded_96x48'
    bins, S, X = truth['bins_' + name], truth['S_' + name], truth['X_' + name]
    r = device.bins_eig(bins, 0.0)
    assert r['rank'] == 48
    dev = np.abs(r['sigma'][::-1] - S) / S
    lam = np.linalg.eigvalsh(X.T @ X)[::-1]
    eigh = np.abs(np.sqrt(np.abs(lam)) - S) / S
    svd = np.abs(np.linalg.svd(X, compute_uv=False) - S) / S
    for k in range(48):
        print('sigma_%02d %.3e   rel. error: device %.2e   eigh(C) %.2e   svd(X) %.2e' % (k, S[k], dev[k], eigh[k], svd[k]))
    print('worst: device %.3e   eigh(C) %.3e   svd(X) %.3e' % (dev.max(), eigh.max(), svd.max()))
    assert dev.max() < 4 * svd.max()


def test_threshold_cuts_the_eigenvalues_not_the_singular_values_and_keeps_equality(truth):
    """the absolute cut of the kernel: on lambda = sigma^2, ``>=``; the device's mask against ``device.bins_keep``"""
    name = 'graded_96x48'
    bins, S = truth['bins_' + name], truth['S_' + name]
    lam_truth = S ** 2                                   # descending, 9.6e-3 ... 7.8e-23
    full = device.bins_eig(bins, 0.0)
    lam_dev = full['sigma'] ** 2                         # ascending
    assert full['rank'] == 48
    for keep in (47, 30, 21, 5, 1):
        thr = float(np.sqrt(lam_truth[keep - 1] * lam_truth[keep]))       # between two truth eigenvalues
        r = device.bins_eig(bins, thr)
        mask = device.bins_keep(lam_dev, thr, *bins.shape)
        print('threshold %.3e: rank %d (truth: %d eigenvalues above, %d singular values above)'
              % (thr, r['rank'], (lam_truth >= thr).sum(), (S >= thr).sum()))
        assert r['rank'] == keep == mask.sum() != (S >= thr).sum()
        # what is kept is the upper end of the full decomposition, bit for bit
        assert r['sigma'].tobytes() == full['sigma'][48 - keep:].tobytes()
        assert r['T'].tobytes() == full['T'][48 - keep:].tobytes()
    # an eigenvalue equal to the threshold is kept, the next number above it cuts it
    for k in (3, 17, 40):
        var = _raw_var(bins, 0.0)
        thr = float(var[k])
        assert _raw_rank(bins, thr) == 48 - k
        assert _raw_rank(bins, float(np.nextafter(thr, np.inf))) == 48 - k - 1
    # a threshold above everything: rank 0 from the library, an exception from the setter
    assert _raw_rank(bins, 1.0) == 0
    with pytest.raises(AssertionError, match='cov_threshold'):
        mx.TauMaxEnt(cov_threshold=1.0).set_G_tau_bins(np.linspace(0, 1, 48), bins)


def _raw(bins, thr):
    lib = device.load_library()
    b = np.ascontiguousarray(bins[None], dtype=float)
    m, n = bins.shape
    mean, var, T = np.empty((1, n)), np.empty((1, n)), np.empty((1, n, n))
    rank, sweeps = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    rc = lib.mxe_bins_eig(0, 1, m, n, b.ctypes.data_as(dp), float(thr), mean.ctypes.data_as(dp), var.ctypes.data_as(dp),
                          T.ctypes.data_as(dp), rank.ctypes.data_as(ip), sweeps.ctypes.data_as(ip))
    assert rc == 0
    return var[0], int(rank[0])


def _raw_var(bins, thr):
    return _raw(bins, thr)[0]


def _raw_rank(bins, thr):
    var, rank = _raw(bins, thr)
    assert np.all(var[:rank] >= thr) and np.all(var[rank:] == 0.0)
    return rank


def test_launches_repeat_bit_for_bit_and_sets_do_not_see_each_other(truth):
    a, b = truth['bins_well_96x48'], truth['bins_graded_96x48']
    alone = device.bins_eig(a, 0.0)
    again = device.bins_eig(a, 0.0)
    batch = device.bins_eig(np.stack([b, a, b * 3.0, a]), 0.0)
    for other in (again, batch[1], batch[3]):
        for k in ('mean', 'sigma', 'T'):
            assert alone[k].tobytes() == other[k].tobytes(), k
        assert alone['rank'] == other['rank'] and alone['sweeps'] == other['sweeps']
    assert batch[0]['sigma'].tobytes() == device.bins_eig(b, 0.0)['sigma'].tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------
def _single(g, **kw):
    tm = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), **kw)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    return tm


def test_single_element_bins_match_truth_reference_and_host_path(g):
    tm = _single(g)
    tm.set_G_tau_bins(g['s_tau'], g['s_bins'])
    st = tm.bin_statistics
    assert st['rank'] == 40 and st['n_bins'] == 256 and st['T'].shape == (40, 40) and 0 < st['sweeps'] < SWEEP_CAP
    np.testing.assert_allclose(st['mean'], g['s_mean'], rtol=0, atol=2 * EPS * np.abs(g['s_bins']).max())
    res = tm.run()
    np.testing.assert_allclose(res.alpha, g['s_alpha'], rtol=1e-13)
    e = rel_l2(np.asarray(res.H), g['s_H_truth'])
    print('bins path vs truth: %.2e, audit %.2e' % (e.max(), tm.last_launch['audit_max']))
    assert e.max() < GATE and tm.last_launch['audit_max'] < GATE
    assert rel_l2(np.asarray(res.A), g['s_A']).max() < 2e-4            # (the reference's raw output: its slack)
    np.testing.assert_allclose(res.chi2, g['s_chi2'], rtol=1e-4)
    assert rel_l2(res.analyzer_results['LineFitAnalyzer']['A_out'], g['s_A_out']) < 2e-4
    # the same job through the host path
    th = _single(g)
    th.set_G_tau_data(g['s_tau'], g['s_mean'])
    th.set_cov(g['s_cov'])
    rh = th.run()
    assert len(th.err) == len(tm.err) == 40
    eh = rel_l2(np.asarray(res.H), np.asarray(rh.H))
    print('bins path vs host path: %.2e' % eh.max())
    assert eh.max() < GATE
    # results come back in the original basis
    np.testing.assert_allclose(res.G_orig, st['mean'], rtol=0, atol=0)
    assert np.asarray(res.G_rec).shape[-1] == 40


def test_a_cov_threshold_that_drops_directions_drops_the_same_in_both_paths(g):
    lam = np.linalg.eigvalsh(g['s_cov'])                                # ascending, 1.8e-10 ... 3.5e-8
    for drop in (7, 25):
        thr = float(np.sqrt(lam[drop - 1] * lam[drop]))
        tm = mx.TauMaxEnt(cov_threshold=thr)
        th = mx.TauMaxEnt(cov_threshold=thr)
        for t in (tm, th):
            t.set_verbosity(mx.VerbosityFlags.Quiet)
            t.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
            t.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
        tm.set_G_tau_bins(g['s_tau'], g['s_bins'])
        th.set_G_tau_data(g['s_tau'], g['s_mean'])
        th.set_cov(g['s_cov'])
        assert tm.bin_statistics['rank'] == len(tm.err) == len(th.err) == 40 - drop
        np.testing.assert_allclose(tm.err, th.err, rtol=1e-10)
        assert np.all(tm.err ** 2 >= thr)
        e = rel_l2(np.asarray(tm.run().H), np.asarray(th.run().H))
        print('cov_threshold %.3e: rank %d, bins path vs host path %.2e' % (thr, len(tm.err), e.max()))
        assert e.max() < GATE and tm.last_launch['audit_max'] < GATE


def _ew(g, herm=False, cplx=False):
    ew = mx.ElementwiseMaxEnt(use_hermiticity=herm, use_complex=cplx, cov_threshold=float(g['cov_threshold']))
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    return ew


def test_elementwise_bins_match_truth_reference_and_host_path(g):
    ew = _ew(g)
    ew.set_G_tau_bins(g['e_tau'], g['e_bins'])
    assert sorted(ew.bin_statistics) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert all(st['rank'] == 30 and st['n_bins'] == 200 for st in ew.bin_statistics.values())
    res = ew.run()
    np.testing.assert_allclose(res.alpha, g['e_alpha'], rtol=1e-13)
    e = rel_l2(np.asarray(res.H), g['e_H_truth'])
    print('bins path vs truth: %.2e' % e.max())
    assert np.all(np.isfinite(e)) and e.max() < GATE
    assert all(info['audit_max'] < GATE for info in ew.last_launches) and len(ew.last_launches) >= 1
    for i in range(2):
        for j in range(2):
            assert rel_l2(res.A[i, j], g['e_A'][i, j]).max() < 2e-4, (i, j)
            np.testing.assert_allclose(res.chi2[i, j], g['e_chi2'][i, j], rtol=1e-4)
    assert rel_l2(res.A_out, g['e_A_out']).max() < 2e-4
    # the host path, one fresh worker per element (a reused worker hops from the previous element's rotation)
    for i in range(2):
        for j in range(2):
            th = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), **({} if i == j else dict(cost_function='plusminus')))
            th.set_verbosity(mx.VerbosityFlags.Quiet)
            th.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
            th.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
            th.set_G_tau_data(g['e_tau'], g['e_mean'][i, j])
            th.set_cov(g['e_cov'][i, j])
            rh = th.run()
            assert len(th.err) == ew.bin_statistics[(i, j)]['rank']
            assert rel_l2(np.asarray(res.H[i, j]), np.asarray(rh.H)).max() < GATE, (i, j)


def test_hermiticity_and_complex_variants(g):
    base = _ew(g)
    base.set_G_tau_bins(g['e_tau'], g['e_bins'])
    ref = base.run()
    herm = _ew(g, herm=True)
    herm.set_G_tau_bins(g['e_tau'], g['e_bins'])
    assert sorted(herm.bin_statistics) == [(0, 0), (0, 1), (1, 1)]          # only i <= j goes down
    rh = herm.run()
    for idx in ((0, 0), (0, 1), (1, 1)):
        assert rel_l2(np.asarray(rh.H[idx]), np.asarray(ref.H[idx])).max() < GATE
    np.testing.assert_array_equal(rh.A_out[1, 0], rh.A_out[0, 1])
    # complex: the imaginary parts are sets of their own, with the covariance of their own mean
    im = 0.5 * g['e_bins'][:, ::-1, ::-1, :]
    cx = _ew(g, herm=True, cplx=True)
    cx.set_G_tau_bins(g['e_tau'], g['e_bins'] + 1j * im)
    assert sorted(cx.bin_statistics) == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0)]
    rc = cx.run()
    assert rc.H.shape == (2, 2, 2, 6, 60) and np.iscomplexobj(rc.A_out)
    assert all(info['audit_max'] < GATE for info in cx.last_launches)
    for idx in ((0, 0), (0, 1), (1, 1)):
        assert rel_l2(np.asarray(rc.H[idx + (0,)]), np.asarray(ref.H[idx])).max() < GATE
    # Im G_01 = 0.5 Re G_10 in every bin: the host path with that mean and covariance
    th = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), cost_function='plusminus')
    th.set_verbosity(mx.VerbosityFlags.Quiet)
    th.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    th.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    th.set_G_tau_data(g['e_tau'], 0.5 * g['e_mean'][1, 0])
    th.set_cov(0.25 * g['e_cov'][1, 0])
    assert rel_l2(np.asarray(rc.H[0, 1, 1]), np.asarray(th.run().H)).max() < GATE
    # real bins with use_complex: no imaginary parts to solve
    rr = _ew(g, herm=True, cplx=True)
    rr.set_G_tau_bins(g['e_tau'], g['e_bins'])
    assert sorted(rr.bin_statistics) == [(0, 0, 0), (0, 1, 0), (1, 1, 0)]
    r2 = rr.run()
    assert (0, 1, 1) in [tuple(z) for z in r2.zero_elements]
    assert rel_l2(np.asarray(r2.H[0, 1, 0]), np.asarray(ref.H[0, 1])).max() < GATE


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


def test_matsubara_bins_equal_the_host_path(g):
    iomega, bins = _iw_bins(g)
    tm = _single(g)
    tm.set_G_iw_bins(iomega, bins)
    assert isinstance(tm.K, mx.IOmegaKernel) and tm.bin_statistics['rank'] == 40
    stacked = np.concatenate([bins.real, bins.imag], axis=-1)
    C, mean = cov_longdouble(stacked)
    np.testing.assert_allclose(tm.bin_statistics['mean'], mean, rtol=0, atol=2 * EPS * np.abs(stacked).max())
    res = tm.run()
    assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE
    assert np.iscomplexobj(res.G_orig) and np.asarray(res.G_orig).shape == (20,)
    assert np.iscomplexobj(res.G_rec) and np.asarray(res.G_rec).shape[-1] == 20
    th = _single(g)
    th.set_G_iw_data(iomega, mean[:20] + 1j * mean[20:])
    th.set_cov(C)
    rh = th.run()
    assert len(th.err) == len(tm.err) == 40
    assert rel_l2(np.asarray(res.H), np.asarray(rh.H)).max() < GATE
    # element-wise: the hermitian split of every bin
    b4 = np.empty((160, 2, 2, 20), dtype=complex)
    for i in range(2):
        for j in range(2):
            b4[:, i, j, :] = _iw_bins(g, seed=20 + 2 * i + j)[1] * (1.0 if i == j else 0.3)
    ew = _ew(g, herm=True)
    ew.set_G_iw_bins(iomega, b4)
    re = ew.run()
    assert all(info['audit_max'] < GATE for info in ew.last_launches)
    sym = 0.5 * (b4[:, 0, 1, :] + b4[:, 1, 0, :])
    C01, m01 = cov_longdouble(np.concatenate([sym.real, sym.imag], axis=-1))
    th = _single(g, cost_function='plusminus')
    th.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    th.set_G_iw_data(iomega, m01[:20] + 1j * m01[20:])
    th.set_cov(C01)
    rh = th.run()
    assert rel_l2(np.asarray(re.H[0, 1]), np.asarray(rh.H)).max() < GATE


def test_posterior_errors_on_a_bins_result(g):
    windows = [(-3.0, 0.0), (0.0, 3.0), (-9.0, 9.0)]
    tm = _single(g)
    tm.set_G_tau_bins(g['s_tau'], g['s_bins'])
    pe = tm.posterior_errors(tm.run(), windows=windows)
    th = _single(g)
    th.set_G_tau_data(g['s_tau'], g['s_mean'])
    th.set_cov(g['s_cov'])
    ph = th.posterior_errors(th.run(), windows=windows)
    for k in ('window_weight', 'window_err', 'window_prior_err'):
        print(k, pe[k], ph[k])
        np.testing.assert_allclose(pe[k], ph[k], rtol=1e-6)
    assert np.all(pe['window_err'] > 0)


def test_tiny_and_huge_bins_converge_like_bins_of_order_one(truth):
    """products of two squared row norms under- or overflow long before the norms do: the rotation test must not form them"""
    bins, S = truth['bins_well_96x48'], truth['S_well_96x48']
    ref = device.bins_eig(bins, 0.0)
    for scale in (2.0 ** -300, 2.0 ** 240):             # (powers of two: the scaled problem is the same problem exactly)
        r = device.bins_eig(bins * scale, 0.0)
        assert r['rank'] == 48 and r['sweeps'] == ref['sweeps']
        assert np.abs(r['sigma'][::-1] / scale - S).max() <= 1e-12 * S[0]


# ---- sizes and limits ----------------------------------------------------------------------------------------------
def test_512_data_points_run_and_513_are_refused():
    rng = np.random.RandomState(77)
    bins = rng.randn(640, 512) * np.linspace(1.0, 0.05, 512)[None, :]
    r = device.bins_eig(bins, 0.0)
    assert r['rank'] == 512 and 0 < r['sweeps'] < SWEEP_CAP
    C, mean = cov_longdouble(bins)
    lam = np.linalg.eigvalsh(C)
    assert np.abs(r['sigma'] - np.sqrt(lam)).max() <= 1e-12 * np.sqrt(lam[-1])
    assert np.abs(r['T'] @ r['T'].T - np.eye(512)).max() <= 1e-12
    # the short side at full width
    r2 = device.bins_eig(bins[:100], 0.0)
    assert r2['rank'] == 99 and 0 < r2['sweeps'] < SWEEP_CAP
    # 513: MXE_ERR_ARG from the library before anything is launched, an exception from the wrapper and the setters
    lib = device.load_library()
    b = np.zeros((1, 4, 513))
    out = [np.zeros((1, 513)), np.zeros((1, 513)), np.zeros((1, 513, 513))]
    ints = [np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    rc = lib.mxe_bins_eig(0, 1, 4, 513, b.ctypes.data_as(dp), 0.0, *[a.ctypes.data_as(dp) for a in out],
                          *[a.ctypes.data_as(ip) for a in ints])
    assert rc == -1
    with pytest.raises(device.MaxEntDeviceError):
        device.bins_eig(rng.randn(600, 513), 0.0)
    with pytest.raises(AssertionError):
        mx.TauMaxEnt().set_G_tau_bins(np.linspace(0, 1, 513), rng.randn(600, 513))
    # a NaN is MXE_ERR_ARG too
    b = np.ones((1, 4, 8))
    b[0, 2, 3] = np.nan
    out = [np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 8, 8))]
    rc = lib.mxe_bins_eig(0, 1, 4, 8, b.ctypes.data_as(dp), 0.0, *[a.ctypes.data_as(dp) for a in out],
                          *[a.ctypes.data_as(ip) for a in ints])
    assert rc == -1
