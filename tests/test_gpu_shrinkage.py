"""Shrinkage covariance of the mean on the device: the intensity of ``mxe_bins_eig_shrunk`` against its longdouble
restatement (tests/shrinkage_ref.py), the decomposition of C* = (1 - lambda) X^T X + lambda diag(c) with the gates of
tests/test_gpu_bins.py, and the ``shrinkage`` argument of the setters end to end.

The gate of the intensity is |lambda_dev - lambda_ref| <= C_GATE (m + 4) eps kappa lambda_ref: the rounding of an m-term
sum whose numerator cancels by kappa = sum (G2 + m w^2) / sum (G2 - m w^2).  C_GATE = 8 x the worst constant measured on
an MI355X over SHAPES (C_MEASURED, printed by every case; DESIGN.md section 4y has the table); a constant above 64 would
mean a cancellation the kernel should not have.

Measured on an MI355X: constants 0.034, 0.031, 0.001, 0.013, 0.001, 0.017, 0.103 (16 x 512), 0.016, 0.039 in the order of
SHAPES; with columns times 10^+-8 at most 0.103, shifted by 10^6 sigma at most 0.039.  Decomposition, worst of the ten
shapes: eigenvalues 1.9e-15 lambda_max, |T T^T - 1| 1.4e-15, |T^T diag(sigma^2) T - C*|_2 2.8e-15 lambda_max.  chi^2 per
direction at 130 x 65: 0.822 with shrinkage, 2.091 without."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device
import shrinkage_ref as R
from shrinkage_ref import EPS, LD

pytestmark = pytest.mark.gpu

GATE = 1e-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SWEEP_CAP = 60
C_MEASURED = 0.1031             # the worst |lambda_dev - lambda_ref| / ((m + 4) eps kappa lambda_ref) over SHAPES
C_GATE = 8 * C_MEASURED
KEYS_PLAIN = {'mean', 'sigma', 'T', 'rank', 'sweeps', 'n_bins'}
KEYS_SHRUNK = KEYS_PLAIN | {'shrinkage', 'shrinkage_raw', 'variance'}

_CASES = {}


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLD, 'bins.npz'))


def _rho(m, n):
    return 0.95 if (m, n) == (130, 65) else 0.9


def _case(m, n, seed=0):
    """bins, their longdouble intensity and the device's answer with ``'auto'``, once per shape"""
    key = (m, n, seed)
    if key not in _CASES:
        bins = R.ar1_bins(m, n, _rho(m, n), seed)
        bins.setflags(write=False)
        _CASES[key] = (bins, R.intensity(bins), device.bins_eig_shrunk(bins, 0.0, 'auto'))
    return _CASES[key]


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _constant(m, ref, lam_dev):
    return abs(LD(lam_dev) - ref['lam']) / (LD(m + 4) * EPS * ref['kappa'] * ref['lam'])


def _same_bits(a, b, keys=('mean', 'sigma', 'T', 'variance')):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert a['rank'] == b['rank'] and a['sweeps'] == b['sweeps']
    assert np.float64(a['shrinkage']).tobytes() == np.float64(b['shrinkage']).tobytes()
    assert np.float64(a['shrinkage_raw']).tobytes() == np.float64(b['shrinkage_raw']).tobytes()


# ---- the intensity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n', R.SHAPES)
def test_intensity_against_the_longdouble_reference(m, n):
    bins, ref, st = _case(m, n)
    if n == 1:                                          # no pair of columns: lambda = 1, nothing was estimated
        assert st['shrinkage'] == 1.0 and np.isnan(st['shrinkage_raw'])
        return
    c = float(_constant(m, ref, st['shrinkage']))
    print('%4d x %3d: lambda %.15g (reference %.15g), kappa %.3f, constant %.3f'
          % (m, n, st['shrinkage'], float(ref['lam']), float(ref['kappa']), c))
    assert 0.0 < st['shrinkage_raw'] < 1.0 and st['shrinkage'] == st['shrinkage_raw']
    assert abs(LD(st['shrinkage']) - ref['lam']) <= R.lambda_bound(m, ref, C_GATE), c
    assert C_GATE <= 64


def _moved(m, n, seed=0):
    """bins on a grid of 2^-20 standard deviations (scales of 2^-k over three decades), and the same bins with every column
    scaled by 2^+-27 (1.3e8) and shifted by 2^20 (1.05e6) of its standard deviations: every operation is exact, the second
    problem is the first one"""
    y = R.ar1_bins(m, n, _rho(m, n), seed) / 10.0 ** (-1.5 * np.arange(n) / max(n - 1, 1))[None, :]
    q = np.rint(y * 2.0 ** 20)
    unit = 2.0 ** -np.floor(10.0 * np.arange(n) / max(n - 1, 1))
    base = q * 2.0 ** -20 * unit[None, :]
    big = np.where(np.arange(n) % 2 == 0, 2.0 ** 27, 2.0 ** -27)
    moved = (q + 2.0 ** 40) * 2.0 ** -20 * (unit * big)[None, :]
    assert np.array_equal((moved / (unit * big)[None, :] - 2.0 ** 20) * unit[None, :], base)
    return base, moved


@pytest.mark.parametrize('m,n', [(24, 40), (130, 65), (2000, 8), (5, 63)])
def test_intensity_under_column_scales_and_shifts(m, n):
    """a missing standardisation shows in the first part, a mean that loses digits in the second and third"""
    bins, ref, st = _case(m, n)
    bound = R.lambda_bound(m, ref, C_GATE)
    # columns times 10^+-8: the unscaled value (every scaled bin is rounded once: a relative eps per term of the sums)
    scale = np.where(np.arange(n) % 2 == 0, 1e8, 1e-8)
    got = device.bins_eig_shrunk(bins * scale[None, :], 0.0, 'auto')
    print('scaled: lambda %.15g, constant %.3f' % (got['shrinkage'], float(_constant(m, ref, got['shrinkage']))))
    assert abs(LD(got['shrinkage']) - ref['lam']) <= bound
    np.testing.assert_allclose(got['variance'], st['variance'] * scale ** 2, rtol=1e-13)
    # scales and shifts of 10^6 sigma that are exact: the unmoved value
    base, moved = _moved(m, n)
    ref_b = R.intensity(base)
    got_b, got_m = device.bins_eig_shrunk(base, 0.0, 'auto'), device.bins_eig_shrunk(moved, 0.0, 'auto')
    print('exactly moved: lambda %.15g (unmoved %.15g, reference %.15g), constant %.3f'
          % (got_m['shrinkage'], got_b['shrinkage'], float(ref_b['lam']), float(_constant(m, ref_b, got_m['shrinkage']))))
    assert abs(LD(got_b['shrinkage']) - ref_b['lam']) <= R.lambda_bound(m, ref_b, C_GATE)
    assert abs(LD(got_m['shrinkage']) - ref_b['lam']) <= R.lambda_bound(m, ref_b, C_GATE)
    # scales of 10^+-8 and shifts of 10^6 sigma as they round: the reference on the same numbers
    sd = bins.std(axis=0)
    far = (bins + 1e6 * sd[None, :]) * scale[None, :]
    ref_f = R.intensity(far)
    got_f = device.bins_eig_shrunk(far, 0.0, 'auto')
    print('moved with rounding: lambda %.15g (reference %.15g), constant %.3f'
          % (got_f['shrinkage'], float(ref_f['lam']), float(_constant(m, ref_f, got_f['shrinkage']))))
    assert abs(LD(got_f['shrinkage']) - ref_f['lam']) <= R.lambda_bound(m, ref_f, C_GATE)


# ---- the decomposition -----------------------------------------------------------------------------------------------
def _assert_decomposition(bins, st, what):
    """the gates of tests/test_gpu_bins.py on C* with the lambda the device used"""
    m, n = bins.shape
    Cs = np.asarray(R.shrunk_cov(bins, st['shrinkage']), dtype=float)
    lam_ref = np.linalg.eigvalsh(Cs)
    rank, T, lam = st['rank'], st['T'], st['sigma'] ** 2
    assert rank == n == len(lam) and T.shape == (n, n), (what, rank)
    e_val = np.abs(lam - lam_ref).max() / lam_ref[-1]
    e_sig = np.abs(st['sigma'] - np.sqrt(lam_ref)).max() / np.sqrt(lam_ref[-1])
    orth = np.abs(T @ T.T - np.eye(n)).max()
    rec = np.linalg.norm(T.T @ (lam[:, None] * T) - Cs, 2) / lam_ref[-1]
    print('%s: lambda %.4g, rank %d, sweeps %d; eigenvalues %.2e, sigma %.2e of the largest, |T T^T - 1| %.2e, '
          '|T^T diag T - C*|_2 %.2e lambda_max' % (what, st['shrinkage'], rank, st['sweeps'], e_val, e_sig, orth, rec))
    assert e_val <= 1e-12 and e_sig <= 1e-12
    assert orth <= 1e-12
    assert rec <= 1e-13
    assert np.all(np.diff(st['sigma']) >= 0)
    assert np.all(T[np.arange(n), np.abs(T).argmax(axis=1)] > 0)
    assert 0 < st['sweeps'] < SWEEP_CAP or n == 1
    c = np.asarray(R.cov_parts(bins)[2], dtype=float)
    np.testing.assert_allclose(st['variance'], c, rtol=1e-13)
    mean = np.asarray(R.cov_parts(bins)[3], dtype=float)
    assert np.abs(st['mean'] - mean).max() <= 2 * EPS * np.abs(bins).max()


@pytest.mark.parametrize('m,n', R.SHAPES)
def test_decomposition_of_the_shrunk_covariance(m, n):
    bins, ref, st = _case(m, n)
    _assert_decomposition(bins, st, '%d x %d' % (m, n))
    assert st['mean'].tobytes() == device.bins_eig(bins, 0.0)['mean'].tobytes()       # the mean of mxe_bins_eig


def test_fewer_bins_than_data_keep_every_direction():
    bins, ref, st = _case(24, 40)
    plain = device.bins_eig(bins, 0.0)
    assert plain['rank'] == 23 and st['rank'] == 40
    assert set(st) == (KEYS_SHRUNK - {'n_bins'}) and set(plain) == (KEYS_PLAIN - {'n_bins'})
    got = mx.shrink_bins(bins)
    assert set(got) == KEYS_SHRUNK and got['n_bins'] == 24
    _same_bits(got, st)
    # a threshold still cuts from below
    thr = float(np.sqrt(st['sigma'][9] ** 2 * st['sigma'][10] ** 2))
    cut = device.bins_eig_shrunk(bins, thr, 'auto')
    assert cut['rank'] == 30 and cut['sigma'].tobytes() == st['sigma'][10:].tobytes()
    assert cut['T'].tobytes() == st['T'][10:].tobytes()


@pytest.mark.parametrize('m,n', [(24, 40), (130, 65), (4, 7)])
def test_fixed_intensities(m, n):
    bins = _case(m, n)[0]
    c = np.asarray(R.cov_parts(bins)[2], dtype=float)
    # lambda = 1: the variances, in their order
    one = device.bins_eig_shrunk(bins, 0.0, 1.0)
    assert one['shrinkage'] == 1.0 and np.isnan(one['shrinkage_raw']) and one['rank'] == n
    np.testing.assert_allclose(one['sigma'] ** 2, np.sort(c), rtol=1e-14)
    P = np.zeros((n, n))
    P[np.arange(n), np.argsort(c, kind='stable')] = 1.0
    assert np.abs(one['T'] - P).max() <= 1e-14
    # lambda in between and lambda = 0 (the sample covariance through the QR of [X ; 0])
    for lam in (0.3, 0.0):
        st = device.bins_eig_shrunk(bins, 0.0, lam)
        assert st['shrinkage'] == lam and np.isnan(st['shrinkage_raw'])
        if lam > 0.0:
            _assert_decomposition(bins, st, '%d x %d, lambda %.1f' % (m, n, lam))
        else:
            plain = device.bins_eig(bins, 0.0)
            assert st['rank'] == plain['rank'] == min(m - 1, n)
            np.testing.assert_allclose(st['sigma'], plain['sigma'], rtol=0, atol=1e-12 * plain['sigma'][-1])


def test_a_constant_column_is_left_out_and_its_direction_dropped():
    a, b = _case(12, 5)[0], R.ar1_bins(12, 5, 0.9, seed=3)
    flat = np.array(R.ar1_bins(12, 5, 0.9, seed=4))
    flat[:, 2] = 0.75
    ref = R.intensity(flat)
    assert ref['used'].tolist() == [True, True, False, True, True] and 0 < ref['raw'] < 1
    batch = device.bins_eig_shrunk(np.stack([a, flat, b]), 0.0, 'auto')
    st = batch[1]
    print('constant column: lambda %.15g (reference %.15g), rank %d' % (st['shrinkage'], float(ref['lam']), st['rank']))
    assert abs(LD(st['shrinkage']) - ref['lam']) <= R.lambda_bound(12, ref, C_GATE)
    assert st['rank'] == 4 and st['variance'][2] == 0.0 and st['mean'][2] == 0.75
    assert np.abs(st['T'][:, 2]).max() == 0.0
    Cs = np.asarray(R.shrunk_cov(flat, st['shrinkage']), dtype=float)
    assert np.linalg.norm(st['T'].T @ (st['sigma'][:, None] ** 2 * st['T']) - Cs, 2) <= 1e-13 * st['sigma'][-1] ** 2
    _same_bits(batch[0], device.bins_eig_shrunk(a, 0.0, 'auto'))
    _same_bits(batch[2], device.bins_eig_shrunk(b, 0.0, 'auto'))


def test_sets_of_a_launch_do_not_see_each_other_and_launches_repeat():
    sets = [R.ar1_bins(24, 40, rho, seed) * scale for seed, (rho, scale) in
            enumerate([(0.9, 1.0), (0.5, 3.0), (0.95, 1e-3), (0.0, 1.0), (0.7, 50.0), (0.9, 1.0)], start=10)]
    batch = device.bins_eig_shrunk(np.stack(sets), 0.0, 'auto')
    again = device.bins_eig_shrunk(np.stack(sets), 0.0, 'auto')
    lams = [st['shrinkage'] for st in batch]
    print('lambda of the six sets:', lams)
    assert len(set(lams)) == 6
    for s in range(6):
        _same_bits(batch[s], again[s])
        _same_bits(batch[s], device.bins_eig_shrunk(sets[s], 0.0, 'auto'))
    fixed = device.bins_eig_shrunk(np.stack(sets), 0.0, 0.25)
    for s in (0, 3, 5):
        _same_bits(fixed[s], device.bins_eig_shrunk(sets[s], 0.0, 0.25))


# ---- the setters -----------------------------------------------------------------------------------------------------
def _single(g, **kw):
    tm = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), **kw)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    return tm


def _ew(g, herm=False, cplx=False):
    ew = mx.ElementwiseMaxEnt(use_hermiticity=herm, use_complex=cplx, cov_threshold=float(g['cov_threshold']))
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    return ew


def test_fixed_intensity_equals_the_host_path_with_the_shrunk_covariance(g):
    bins = g['s_bins'][:24]                              # 24 bins of 40 values
    tm = _single(g)
    tm.set_G_tau_bins(g['s_tau'], bins, shrinkage=0.3)
    st = tm.bin_statistics
    assert set(st) == KEYS_SHRUNK and st['rank'] == 40 == len(tm.err) and st['shrinkage'] == 0.3 and st['n_bins'] == 24
    res = tm.run()
    assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE
    th = _single(g)
    th.set_G_tau_data(g['s_tau'], np.asarray(R.cov_parts(bins)[3], dtype=float))
    th.set_cov(np.asarray(R.shrunk_cov(bins, 0.3), dtype=float))
    rh = th.run()
    assert len(th.err) == 40
    np.testing.assert_allclose(tm.err, th.err, rtol=1e-10)
    e = rel_l2(np.asarray(res.H), np.asarray(rh.H))
    print('shrunk bins path vs host path: %.2e, audit %.2e' % (e.max(), tm.last_launch['audit_max']))
    assert e.max() < GATE and th.last_launch['audit_max'] < GATE
    np.testing.assert_allclose(res.G_orig, st['mean'], rtol=0, atol=0)


def test_without_shrinkage_the_setters_are_the_ones_of_before(g):
    bins = g['s_bins'][:24]
    plain = device.bins_eig(bins, float(g['cov_threshold']))
    for arg in (None, 0.0):
        tm = _single(g)
        before = len(tm.logtaker._errors)
        tm.set_G_tau_bins(g['s_tau'], bins, shrinkage=arg)
        st = tm.bin_statistics
        assert set(st) == KEYS_PLAIN and st['rank'] == 23
        for k in ('mean', 'sigma', 'T'):
            assert st[k].tobytes() == plain[k].tobytes(), k
        assert len(tm.logtaker._errors) == before + 1 and 'rank-deficient' in tm.logtaker._errors[-1]
    ew = _ew(g)
    ew.set_G_tau_bins(g['e_tau'], g['e_bins'][:24], shrinkage=None)
    for (i, j), st in ew.bin_statistics.items():
        assert set(st) == KEYS_PLAIN and st['rank'] == 23
        assert st['T'].tobytes() == device.bins_eig(g['e_bins'][:24, i, j, :], float(g['cov_threshold']))['T'].tobytes()


def _iw_bins(g, n_iw=20, n_bins=30, seed=11):
    beta = float(g['s_beta'])
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    iomega = (2 * np.arange(n_iw) + 1) * np.pi / beta
    K = mx.IOmegaKernel(iomega, omega)
    G = (K.K_complex * omega.delta[None, :]) @ g['s_A_true']
    rng = np.random.RandomState(seed)
    z = rng.randn(n_bins, n_iw) + 1j * rng.randn(n_bins, n_iw)
    z[:, 1:] += 0.5 * z[:, :-1]
    return iomega, G[None, :] + 2e-3 * z / (1.0 + 0.1 * np.arange(n_iw))[None, :]


def test_single_element_setters_with_an_estimated_intensity(g):
    thr = float(g['cov_threshold'])
    # G(tau)
    bins = g['s_bins'][:24]
    tm = _single(g)
    before = len(tm.logtaker._errors)
    tm.set_G_tau_bins(g['s_tau'], bins, shrinkage='auto')
    st = tm.bin_statistics
    assert len(tm.logtaker._errors) == before                       # no direction is lost: no warning
    ref = R.intensity(bins)
    assert set(st) == KEYS_SHRUNK and st['rank'] == 40 == len(tm.err)
    assert abs(LD(st['shrinkage']) - ref['lam']) <= R.lambda_bound(24, ref, C_GATE)
    _same_bits(st, device.bins_eig_shrunk(bins, thr, 'auto'))
    res = tm.run()
    assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE
    # G(i omega_n): the stacked [Re ; Im] values
    iomega, zb = _iw_bins(g)
    tw = _single(g)
    tw.set_G_iw_bins(iomega, zb, shrinkage='auto')
    stacked = np.concatenate([zb.real, zb.imag], axis=-1)
    sw = tw.bin_statistics
    assert isinstance(tw.K, mx.IOmegaKernel) and sw['rank'] == 40 and set(sw) == KEYS_SHRUNK
    _same_bits(sw, device.bins_eig_shrunk(stacked, thr, 'auto'))
    rw = tw.run()
    assert np.all(rw.converged) and tw.last_launch['audit_max'] < GATE
    # Legendre coefficients
    b = np.load(os.path.join(GOLD, 'legendre_bins.npz'))
    tl = mx.TauMaxEnt()
    tl.set_verbosity(mx.VerbosityFlags.Quiet)
    tl.omega = mx.DataOmegaMesh(b['omega'])
    tl.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    tl.set_G_l_bins(b['s_bins'], float(b['beta']), shrinkage='auto')
    sl = tl.bin_statistics
    assert type(tl.K) is mx.LegendreKernel and sl['rank'] == 30 == len(tl.err) and sl['n_bins'] == 24
    _same_bits(sl, device.bins_eig_shrunk(b['s_bins'], tl.cov_threshold, 'auto'))
    rl = tl.run()
    assert np.all(rl.converged) and tl.last_launch['audit_max'] < GATE
    print('lambda: G(tau) %.4f, G(i omega_n) %.4f, G_l %.4f' % (st['shrinkage'], sw['shrinkage'], sl['shrinkage']))


@pytest.mark.parametrize('cplx', [False, True])
def test_elementwise_setters_give_every_set_its_own_intensity(g, cplx):
    thr = float(g['cov_threshold'])
    bins = g['e_bins'][:24]                              # (24, 2, 2, 30)
    if cplx:
        bins = bins + 0.5j * bins[:, ::-1, ::-1, :]
    ew = _ew(g, herm=cplx, cplx=cplx)
    ew.set_G_tau_bins(g['e_tau'], bins, shrinkage='auto')
    keys = sorted(ew.bin_statistics)
    assert keys == ([(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0)] if cplx else [(0, 0), (0, 1), (1, 0), (1, 1)])
    lams = []
    for key in keys:
        st = ew.bin_statistics[key]
        part = bins[:, key[0], key[1], :]
        one = np.ascontiguousarray(part.imag if (cplx and key[2] == 1) else part.real)
        assert set(st) == KEYS_SHRUNK and st['rank'] == 30 and st['n_bins'] == 24
        _same_bits(st, device.bins_eig_shrunk(one, thr, 'auto'))
        lams.append(st['shrinkage'])
    print('lambda per set:', dict(zip(keys, lams)))
    assert len(set(lams)) == 4                           # (with use_complex the fourth set is Im G_01 = 0.5 Re G_10)
    res = ew.run()
    assert all(info['audit_max'] < GATE for info in ew.last_launches) and ew.last_launches
    assert np.all(np.isfinite(np.asarray(res.A_out)))
    # Matsubara and Legendre bins reach the same call
    iomega = _iw_bins(g)[0]
    b4 = np.empty((30, 2, 2, 20), dtype=complex)
    for i in range(2):
        for j in range(2):
            b4[:, i, j, :] = _iw_bins(g, seed=20 + 2 * i + j)[1] * (1.0 if i == j else 0.3)
    ei = _ew(g, herm=True, cplx=cplx)
    ei.set_G_iw_bins(iomega, b4, shrinkage='auto')
    assert all(set(st) == KEYS_SHRUNK and st['rank'] == 40 for st in ei.bin_statistics.values())
    sym = 0.5 * (b4[:, 0, 1, :] + b4[:, 1, 0, :])
    _same_bits(ei.bin_statistics[(0, 1, 0) if cplx else (0, 1)],
               device.bins_eig_shrunk(np.concatenate([sym.real, sym.imag], axis=-1), thr, 'auto'))
    b = np.load(os.path.join(GOLD, 'legendre_bins.npz'))
    el = mx.ElementwiseMaxEnt(use_hermiticity=False, use_complex=cplx)
    el.set_verbosity(mx.VerbosityFlags.Quiet)
    el.omega = mx.DataOmegaMesh(b['omega'])
    el.set_G_l_bins(b['e_bins'], float(b['beta']), l=b['e_l'], shrinkage=0.5)
    assert all(st['shrinkage'] == 0.5 and st['rank'] == 12 and st['n_bins'] == 12 for st in el.bin_statistics.values())


def test_resampling_and_bin_checks_run_on_a_shrunk_job(g):
    bins = g['s_bins'][:24]
    tm = _single(g)
    tm.set_G_tau_bins(g['s_tau'], bins, shrinkage='auto')
    assert tm.bin_statistics['rank'] == 40
    jk = tm.resample_errors(bins, method='jackknife')
    assert jk['n_used'] == 24 and np.all(np.isfinite(jk['A_err'])) and np.any(jk['A_err'] > 0)
    assert tm.bin_statistics['rank'] == 40 == len(tm.err)
    cb = tm.check_bins(bins)
    assert cb['basis'] == 'eigen' and cb['err2'].shape[1] == 40 and np.all(np.isfinite(cb['err2']))
    # level 0 of the ladder in the eigenbasis of C* is the variance of the sample covariance along those directions
    T = tm.bin_statistics['T']
    C = np.asarray(R.cov_parts(bins)[1], dtype=float)
    np.testing.assert_allclose(cb['err2'][0], np.einsum('kj,jl,kl->k', T, C, T), rtol=1e-9)
    res = tm.run()
    pe = tm.posterior_errors(res, windows=[(-3.0, 3.0)])
    assert np.isfinite(pe['window_err'][0]) and pe['window_err'][0] > 0
    fd = tm.fit_diagnostics(res)
    assert fd is not None


def test_refused_arguments_leave_the_object_as_it_was(g):
    bins = g['s_bins'][:24]
    tm = _single(g)
    tm.set_G_tau_bins(g['s_tau'], bins, shrinkage='auto')
    st, G, err, K = tm.bin_statistics, np.array(tm.G), np.array(tm.err), tm.K
    for bad in (1.5, 'bogus'):
        with pytest.raises(ValueError, match='shrinkage'):
            tm.set_G_tau_bins(g['s_tau'], g['s_bins'][:30], shrinkage=bad)
    with pytest.raises(ValueError, match='4 bins'):
        tm.set_G_tau_bins(g['s_tau'], g['s_bins'][:3], shrinkage='auto')
    assert tm.bin_statistics is st and tm.K is K and np.array_equal(tm.G, G) and np.array_equal(tm.err, err)
    ew = _ew(g)
    ew.set_G_tau_bins(g['e_tau'], g['e_bins'][:24], shrinkage='auto')
    public = ew.bin_statistics
    for bad in (1.5, 'bogus'):
        with pytest.raises(ValueError, match='shrinkage'):
            ew.set_G_tau_bins(g['e_tau'], g['e_bins'][:30], shrinkage=bad)
    with pytest.raises(ValueError, match='4 bins'):
        ew.set_G_tau_bins(g['e_tau'], g['e_bins'][:3], shrinkage='auto')
    assert ew.bin_statistics is public
    # the library: lambda above 1 and an estimate from three bins are argument errors
    lib = device.load_library()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    for m, lam in ((5, 1.5), (3, -1.0)):
        b = np.ascontiguousarray(bins[None, :m, :8])
        dbl = [np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 8, 8)), np.zeros(1), np.zeros(1), np.zeros((1, 8))]
        ints = [np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]
        rc = lib.mxe_bins_eig_shrunk(0, 1, m, 8, b.ctypes.data_as(dp), 0.0, lam, *[a.ctypes.data_as(dp) for a in dbl[:3]],
                                     *[a.ctypes.data_as(ip) for a in ints], *[a.ctypes.data_as(dp) for a in dbl[3:]], None)
        assert rc == -1


# ---- what it is for --------------------------------------------------------------------------------------------------
def test_chi2_of_fresh_noise_is_calibrated_with_shrinkage_and_not_without():
    """130 bins of 65 values, rho = 0.95: chi^2 per direction of 200 noise vectors drawn from the true covariance of the
    mean, whitened with the device's T and sigma.  The reference alone (LAPACK on C*, seed 0): 0.82 and 2.09; the theory
    for the sample covariance is (m - 1) / (m - n - 2) = 2.05."""
    m, n, rho = 130, 65, 0.95
    bins, ref, st = _case(m, n)
    noise = R.fresh_noise(R.ar1_true_cov_of_mean(m, n, rho), 200, 100)
    plain = device.bins_eig(bins, 0.0)
    chi_s = R.chi2_per_direction(st['T'], st['sigma'], noise)
    chi_p = R.chi2_per_direction(plain['T'], plain['sigma'], noise)
    s_ref, T_ref = R.eig_float(R.shrunk_cov(bins, ref['lam']))
    p_ref, P_ref = R.eig_float(R.shrunk_cov(bins, 0.0))
    ref_s, ref_p = R.chi2_per_direction(T_ref, s_ref, noise), R.chi2_per_direction(P_ref, p_ref, noise)
    print('chi^2 per direction: shrunk %.3f (reference %.3f), sample covariance %.3f (reference %.3f)'
          % (chi_s, ref_s, chi_p, ref_p))
    assert st['rank'] == plain['rank'] == n
    assert 0.6 <= ref_s <= 1.3 and ref_p > 1.6
    assert 0.6 <= chi_s <= 1.3
    assert chi_p > 1.6
