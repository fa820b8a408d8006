"""Shrinkage covariance of the mean, host side (no GPU): the longdouble reference the device tests rely on
(tests/shrinkage_ref.py) is checked against the mathematics, the ``shrinkage`` argument is refused before the device is
asked for anything, and ``mxe_bins_eig_shrunk`` is declared, exported and refuses its arguments without a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device
import shrinkage_ref as R
from shrinkage_ref import EPS, LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n', [(24, 40), (12, 5), (130, 65)])
def test_augmented_matrix_has_the_shrunk_covariance_as_its_gram_matrix(m, n):
    bins = R.ar1_bins(m, n)
    for lam in (0.0, 0.3, float(R.intensity(bins)['lam']), 1.0):
        Y = R.augmented(bins, lam)
        C = R.shrunk_cov(bins, lam)
        assert Y.shape == (m + n, n)
        err = np.abs(Y.T @ Y - C).max() / np.abs(C).max()
        assert err <= 8 * np.finfo(LD).eps * (m + n), (lam, float(err))
    # the variances are kept, only the correlations shrink
    _, C0, c, _ = R.cov_parts(bins)
    Cs = R.shrunk_cov(bins, 0.3)
    np.testing.assert_allclose(np.diag(Cs).astype(float), c.astype(float), rtol=1e-15)
    off = ~np.eye(n, dtype=bool)
    np.testing.assert_allclose(Cs[off].astype(float), 0.7 * C0[off].astype(float), rtol=1e-15)


def test_intensity_does_not_change_under_column_scales_and_shifts():
    bins = R.ar1_bins(24, 40)
    ref = R.intensity(bins)
    rng = np.random.RandomState(5)
    scale = 2.0 ** rng.randint(-27, 28, size=40)          # (powers of two: the same problem exactly)
    shift = rng.randint(-1000, 1000, size=40) * scale
    moved = R.intensity(np.asarray(bins, dtype=LD) * scale + shift)
    assert abs(moved['raw'] - ref['raw']) <= 1e-15 * ref['raw']
    assert abs(moved['kappa'] - ref['kappa']) <= 1e-12 * ref['kappa']


def test_intensity_of_every_device_case_is_strictly_inside_zero_and_one():
    """no clipping hides an error of the device in the tests of tests/test_gpu_shrinkage.py"""
    seen = {}
    for m, n in R.SHAPES:
        r = R.intensity(R.ar1_bins(m, n, 0.95 if (m, n) == (130, 65) else 0.9))
        seen[(m, n)] = float(r['raw'])
        if n == 1:                                        # no pair of columns: lambda = 1 by definition
            assert r['lam'] == 1 and np.isnan(float(r['raw']))
            continue
        assert 0.0 < r['raw'] < 1.0 and r['lam'] == r['raw'], (m, n, float(r['raw']))
        assert 1.0 <= r['kappa'] < 8.0, (m, n, float(r['kappa']))
    print(seen)
    # more bins, less shrinkage
    assert seen[(2000, 8)] < seen[(130, 65)] < seen[(24, 40)]


def test_the_formula_with_the_explicit_sums():
    """Var(r_ij) as the sum over the bins it is defined by, not the Gram matrices the reference and the device use"""
    bins = R.ar1_bins(12, 5)
    b = np.asarray(bins, dtype=LD)
    m, n = b.shape
    x = b - b.mean(axis=0)
    z = x / np.sqrt((x * x).sum(axis=0) / (m - 1))
    num = den = LD(0)
    for i in range(n):
        for j in range(n):
            if i != j:
                w = z[:, i] * z[:, j]
                num += LD(m) / LD(m - 1) ** 3 * ((w - w.mean()) ** 2).sum()
                den += (LD(m) / LD(m - 1) * w.mean()) ** 2
    ref = R.intensity(bins)
    assert abs(num - ref['num']) <= 1e-16 * num and abs(den - ref['den']) <= 1e-16 * den
    assert abs(num / den - ref['raw']) <= 1e-16 * ref['raw']


def test_constant_and_uncorrelated_columns():
    bins = R.ar1_bins(12, 5)
    bins[:, 2] = 0.75
    r = R.intensity(bins)
    assert r['used'].tolist() == [True, True, False, True, True]
    np.testing.assert_allclose(float(r['raw']), float(R.intensity(np.delete(bins, 2, axis=1))['raw']), rtol=1e-15)
    # two columns that are exactly uncorrelated: a zero denominator, lambda = 1
    b = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, -1.0]])
    r = R.intensity(b)
    assert r['den'] == 0 and r['lam'] == 1


# ---- the shrinkage argument ------------------------------------------------------------------------------------------
def test_shrinkage_argument():
    assert device.shrinkage_argument(None, 10) is None
    assert device.shrinkage_argument(0.0, 10) is None and device.shrinkage_argument(0, 10) is None
    assert device.shrinkage_argument('auto', 4) == -1.0
    assert device.shrinkage_argument(0.3, 2) == 0.3 and device.shrinkage_argument(1, 2) == 1.0
    assert device.shrinkage_argument(np.float64(0.25), 2) == 0.25
    for bad in (1.5, -0.1, float('nan'), 'bogus', 'Auto', True, [0.3], 0.3 + 0j):
        with pytest.raises(ValueError, match='shrinkage'):
            device.shrinkage_argument(bad, 10)
    with pytest.raises(ValueError, match='4 bins'):
        device.shrinkage_argument('auto', 3)


class _Touched(Exception):
    pass


def test_setters_refuse_the_argument_before_the_device_is_touched_and_stay_as_they_were(monkeypatch):
    def fake(*args, **kwargs):
        raise _Touched()
    monkeypatch.setattr(device, 'bins_eig', fake)
    monkeypatch.setattr(device, 'bins_eig_shrunk', fake)
    tau = np.linspace(0, 10, 12)
    iw = (2 * np.arange(6) + 1) * np.pi / 10
    rng = np.random.RandomState(0)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.set_G_tau_data(tau, -np.exp(-tau))
    tm.set_error(1e-3)
    G, err, K = np.array(tm.G), np.array(tm.err), tm.K
    for bad in (1.5, 'bogus', -0.5):
        with pytest.raises(ValueError, match='shrinkage'):
            tm.set_G_tau_bins(tau, rng.randn(8, 12), shrinkage=bad)
        with pytest.raises(ValueError, match='shrinkage'):
            tm.set_G_iw_bins(iw, rng.randn(8, 6) + 1j * rng.randn(8, 6), shrinkage=bad)
        with pytest.raises(ValueError, match='shrinkage'):
            tm.set_G_l_bins(rng.randn(8, 6), 10.0, shrinkage=bad)
    with pytest.raises(ValueError, match='4 bins'):
        tm.set_G_tau_bins(tau, rng.randn(3, 12), shrinkage='auto')
    assert tm.K is K and np.array_equal(tm.G, G) and np.array_equal(tm.err, err) and np.array_equal(tm.tau, tau)
    assert not hasattr(tm, 'bin_statistics')
    ew = mx.ElementwiseMaxEnt()
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    for bad in (1.5, 'bogus'):
        with pytest.raises(ValueError, match='shrinkage'):
            ew.set_G_tau_bins(tau, rng.randn(8, 2, 2, 12), shrinkage=bad)
        with pytest.raises(ValueError, match='shrinkage'):
            ew.set_G_iw_bins(iw, rng.randn(8, 2, 2, 6) + 0j, shrinkage=bad)
        with pytest.raises(ValueError, match='shrinkage'):
            ew.set_G_l_bins(rng.randn(8, 2, 2, 6), 10.0, shrinkage=bad)
    with pytest.raises(ValueError, match='4 bins'):
        ew.set_G_tau_bins(tau, rng.randn(3, 2, 2, 12), shrinkage='auto')
    assert not hasattr(ew, 'bin_statistics')
    with pytest.raises(ValueError, match='shrinkage'):
        mx.shrink_bins(rng.randn(8, 12), shrinkage='bogus')
    with pytest.raises(ValueError, match='shrinkage'):
        mx.shrink_bins(rng.randn(8, 12), shrinkage=None)
    with pytest.raises(ValueError, match='4 bins'):
        mx.shrink_bins(rng.randn(3, 12))
    # a valid argument reaches the device call, None and 0.0 the one of before
    monkeypatch.setattr(device, 'bins_eig', lambda *a, **k: (_ for _ in ()).throw(_Touched('plain')))
    monkeypatch.setattr(device, 'bins_eig_shrunk', lambda *a, **k: (_ for _ in ()).throw(_Touched('shrunk')))
    for arg, path in ((None, 'plain'), (0.0, 'plain'), ('auto', 'shrunk'), (0.3, 'shrunk'), (1.0, 'shrunk')):
        with pytest.raises(_Touched, match=path):
            tm.set_G_tau_bins(tau, rng.randn(8, 12), shrinkage=arg)
        with pytest.raises(_Touched, match=path):
            ew.set_G_tau_bins(tau, rng.randn(8, 2, 2, 12), shrinkage=arg)


def test_with_shrinkage_the_few_bins_warning_gives_way_to_a_message_naming_lambda(monkeypatch, capsys):
    def fake(bins, threshold, shrinkage, device=0, timing=None):
        n = bins.shape[-1]
        return dict(mean=np.zeros(n), sigma=np.ones(n), T=np.eye(n), rank=n, sweeps=1, shrinkage=0.4375,
                    shrinkage_raw=0.4375, variance=np.ones(n))
    monkeypatch.setattr(device, 'bins_eig_shrunk', fake)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Default)
    before = len(tm.logtaker._errors)
    st = tm._bins_eig(np.random.RandomState(2).randn(8, 12), 'auto')
    assert len(tm.logtaker._errors) == before                       # no direction is lost: no warning
    out = capsys.readouterr().out
    assert 'lambda = 0.4375' in out and '8 bins for 12 data values' in out
    assert set(st) == {'mean', 'sigma', 'T', 'rank', 'sweeps', 'n_bins', 'shrinkage', 'shrinkage_raw', 'variance'}


# ---- the C-ABI -------------------------------------------------------------------------------------------------------
def test_library_exports_mxe_bins_eig_shrunk_and_the_header_declares_it():
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert re.search(r'\bint\s+mxe_bins_eig_shrunk\s*\(int device, int n_sets, int n_bins, int n_data, const double\* bins, '
                     r'double threshold,\s*double lambda_in,', header)
    lib = device.load_library()
    assert hasattr(lib, 'mxe_bins_eig_shrunk')
    assert 'mxe_bins_eig_shrunk' in [name for name, _, _ in device.SYMBOLS]
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_bins_eig_shrunk(' in source and '#include "mxe_shrink.hip.h"' in source
    assert callable(mx.shrink_bins) and callable(device.bins_eig_shrunk)


def test_argument_refusals_of_the_library_need_no_device():
    lib = device.load_library()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)

    def call(bins, lambda_in, threshold=0.0, drop=None):
        s, m, n = bins.shape
        dbl = dict(mean=np.zeros((s, n)), var=np.zeros((s, n)), T=np.zeros((s, n, n)), lam=np.zeros(s), raw=np.zeros(s),
                   diag=np.zeros((s, n)))
        ptr = dict((k, v.ctypes.data_as(dp)) for k, v in dbl.items())
        if drop:
            ptr[drop] = None
        ints = [np.zeros(s, dtype=np.int32), np.zeros(s, dtype=np.int32)]
        return lib.mxe_bins_eig_shrunk(0, s, m, n, np.ascontiguousarray(bins).ctypes.data_as(dp), threshold, lambda_in,
                                       ptr['mean'], ptr['var'], ptr['T'], *[a.ctypes.data_as(ip) for a in ints],
                                       ptr['lam'], ptr['raw'], ptr['diag'], None)
    ok = np.ones((1, 5, 4))
    assert call(ok, 1.5) == -1 and call(ok, float('nan')) == -1 and call(ok, float('inf')) == -1
    assert call(np.ones((1, 3, 4)), -1.0) == -1                      # an estimate takes four bins
    assert call(np.ones((1, 1, 4)), 0.5) == -1
    assert call(np.ones((1, 5, 513)), 0.5) == -1
    assert call(ok, 0.5, threshold=-1.0) == -1 and call(ok, 0.5, threshold=float('nan')) == -1
    bad = np.ones((2, 5, 7))
    bad[1, 4, 6] = np.nan
    assert call(bad, -1.0) == -1
    for name in ('lam', 'raw', 'diag', 'mean'):
        assert call(ok, 0.5, drop=name) == -1
    if device.device_count() < 1:
        # what passes the checks gets as far as the device: without one MXE_ERR_NODEVICE, not MXE_ERR_ARG
        assert call(ok, 0.5) not in (0, -1) and call(np.ones((1, 3, 4)), 0.5) not in (0, -1)
        assert call(ok, -1.0) not in (0, -1) and call(ok, 0.0) not in (0, -1) and call(ok, 1.0) not in (0, -1)
        with pytest.raises(device.MaxEntDeviceError):
            mx.shrink_bins(np.random.RandomState(0).randn(8, 5))
