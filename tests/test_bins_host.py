"""Binned Monte Carlo data, host side (no GPU): the C-ABI of ``mxe_bins_eig``, the refusals of the setters, the unfolding
of Matsubara bins and the rule that selects the eigenvalues kept."""
import os
import re

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


def test_library_exports_mxe_bins_eig_and_the_header_declares_it():
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert re.search(r'\bint\s+mxe_bins_eig\s*\(int device, int n_sets, int n_bins, int n_data', header)
    lib = device.load_library()
    assert hasattr(lib, 'mxe_bins_eig')
    assert 'mxe_bins_eig' in [name for name, _, _ in device.SYMBOLS]
    assert device.BINS_MAX_DATA == 512


def test_argument_refusals_of_the_library_need_no_device():
    """n_bins < 2, n_data outside 1..512 and NaN / Inf are MXE_ERR_ARG before the device is looked at"""
    import ctypes
    lib = device.load_library()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)

    def call(bins, threshold=0.0):
        s, m, n = bins.shape
        out = [np.zeros((s, n)), np.zeros((s, n)), np.zeros((s, n, n))]
        ints = [np.zeros(s, dtype=np.int32), np.zeros(s, dtype=np.int32)]
        return lib.mxe_bins_eig(0, s, m, n, np.ascontiguousarray(bins).ctypes.data_as(dp), threshold,
                                *[a.ctypes.data_as(dp) for a in out], *[a.ctypes.data_as(ip) for a in ints])
    assert call(np.ones((1, 1, 4))) == -1
    assert call(np.ones((1, 3, 513))) == -1
    bad = np.ones((2, 5, 7))
    bad[1, 4, 6] = np.nan
    assert call(bad) == -1
    bad[1, 4, 6] = np.inf
    assert call(bad) == -1
    assert call(np.ones((1, 3, 4)), threshold=-1.0) == -1
    assert call(np.ones((1, 3, 4)), threshold=float('nan')) == -1


def test_setters_refuse_wrong_shapes_too_few_bins_and_values_that_are_not_finite():
    tau = np.linspace(0, 10, 12)
    iw = (2 * np.arange(6) + 1) * np.pi / 10
    rng = np.random.RandomState(0)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    with pytest.raises(AssertionError, match='last axis'):
        tm.set_G_tau_bins(tau, rng.randn(8, 11))
    with pytest.raises(AssertionError, match='at least two'):
        tm.set_G_tau_bins(tau, rng.randn(1, 12))
    with pytest.raises(AssertionError, match=r'\(n_bins, n_tau\)'):
        tm.set_G_tau_bins(tau, rng.randn(8, 2, 2, 12))
    with pytest.raises(AssertionError, match='real'):
        tm.set_G_tau_bins(tau, rng.randn(8, 12) + 1j)
    b = rng.randn(8, 12)
    b[3, 4] = np.nan
    with pytest.raises(AssertionError, match='not finite'):
        tm.set_G_tau_bins(tau, b)
    with pytest.raises(AssertionError, match='last axis'):
        tm.set_G_iw_bins(iw, rng.randn(8, 12) + 0j)
    with pytest.raises(AssertionError, match='at most 512'):
        tm.set_G_iw_bins(np.arange(257.0), np.zeros((4, 257), dtype=complex))
    zb = rng.randn(8, 6) + 1j * rng.randn(8, 6)
    zb[0, 0] = np.inf
    with pytest.raises(AssertionError, match='not finite'):
        tm.set_G_iw_bins(iw, zb)
    ew = mx.ElementwiseMaxEnt()
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    with pytest.raises(AssertionError, match=r'\(n_bins, M, N, n_tau\)'):
        ew.set_G_tau_bins(tau, rng.randn(8, 12))
    with pytest.raises(AssertionError, match='at least two'):
        ew.set_G_tau_bins(tau, rng.randn(1, 2, 2, 12))
    with pytest.raises(AssertionError, match='use_complex'):
        ew.set_G_tau_bins(tau, rng.randn(8, 2, 2, 12) + 1j)
    with pytest.raises(AssertionError, match=r'\(n_bins, M, M, n_iw\)'):
        ew.set_G_iw_bins(iw, rng.randn(8, 2, 3, 6) + 0j)
    b4 = rng.randn(8, 2, 2, 12)
    b4[1, 1, 0, 2] = -np.inf
    with pytest.raises(AssertionError, match='not finite'):
        ew.set_G_tau_bins(tau, b4)
    with pytest.raises(ValueError):
        device.bins_eig(rng.randn(1, 5), 0.0)
    with pytest.raises(ValueError):
        device.bins_eig(rng.randn(5), 0.0)


def test_refused_bins_leave_the_object_as_it_was(monkeypatch):
    def fake(bins, threshold, device=0):
        raise device_error('refused')
    device_error = device.MaxEntDeviceError
    monkeypatch.setattr(device, 'bins_eig', fake)
    tau = np.linspace(0, 10, 12)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.set_G_tau_data(tau, -np.exp(-tau))
    tm.set_error(1e-3)
    G, err, K = np.array(tm.G), np.array(tm.err), tm.K
    with pytest.raises(device.MaxEntDeviceError):
        tm.set_G_iw_bins((2 * np.arange(6) + 1) * np.pi / 10, np.ones((8, 6), dtype=complex))
    assert tm.K is K and np.array_equal(tm.G, G) and np.array_equal(tm.err, err) and np.array_equal(tm.tau, tau)
    assert not hasattr(tm, 'bin_statistics')


class _Stop(Exception):
    pass


def test_matsubara_bins_go_down_as_the_unfolding_of_every_bin(monkeypatch):
    seen = {}

    def fake(bins, threshold, device=0):
        seen['bins'], seen['threshold'] = np.array(bins), threshold
        raise _Stop()
    monkeypatch.setattr(device, 'bins_eig', fake)
    iw = (2 * np.arange(6) + 1) * np.pi / 10
    rng = np.random.RandomState(1)
    zb = rng.randn(9, 6) + 1j * rng.randn(9, 6)
    tm = mx.TauMaxEnt(cov_threshold=3e-13)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    with pytest.raises(_Stop):
        tm.set_G_iw_bins(iw, zb)
    assert seen['threshold'] == 3e-13
    K = mx.IOmegaKernel(iw, mx.HyperbolicOmegaMesh())
    assert seen['bins'].shape == (9, 12)
    for k in range(9):
        np.testing.assert_array_equal(seen['bins'][k], K.unfold(zb[k]))
    # element-wise: every bin split like set_G_iw_data splits the data, only i <= j with hermiticity, one call
    z4 = rng.randn(9, 2, 2, 6) + 1j * rng.randn(9, 2, 2, 6)
    ew = mx.ElementwiseMaxEnt(use_hermiticity=True, use_complex=True)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    with pytest.raises(_Stop):
        ew.set_G_iw_bins(iw, z4)
    assert seen['bins'].shape == (4, 9, 12)              # (0,0), (0,1) real part, (0,1) imaginary part, (1,1)
    for k in range(9):
        np.testing.assert_array_equal(seen['bins'][0, k], K.unfold(z4[k, 0, 0]))
        np.testing.assert_array_equal(seen['bins'][1, k], K.unfold(0.5 * (z4[k, 0, 1] + z4[k, 1, 0])))
        np.testing.assert_array_equal(seen['bins'][2, k], K.unfold((z4[k, 0, 1] - z4[k, 1, 0]) / 2j))
        np.testing.assert_array_equal(seen['bins'][3, k], K.unfold(z4[k, 1, 1]))


def test_few_bins_log_one_warning(monkeypatch):
    def fake(bins, threshold, device=0):
        raise _Stop()
    monkeypatch.setattr(device, 'bins_eig', fake)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    before = len(tm.logtaker._errors)
    with pytest.raises(_Stop):
        tm.set_G_tau_bins(np.linspace(0, 1, 12), np.random.RandomState(2).randn(12, 12))
    assert len(tm.logtaker._errors) == before + 1 and 'rank-deficient' in tm.logtaker._errors[-1]
    with pytest.raises(_Stop):
        tm.set_G_tau_bins(np.linspace(0, 1, 12), np.random.RandomState(2).randn(13, 12))
    assert len(tm.logtaker._errors) == before + 1


def test_selection_rule_on_a_hand_made_spectrum():
    n_bins, n_data = 1000, 200
    floor = (1000 * EPS) ** 2                      # 4.93e-26: the noise floor of lambda / lambda_max
    lam = np.array([0.0, 1e-40, 0.9 * floor, 1.1 * floor, 1e-20, 0.99e-14, 1e-14, 3e-9, 1.0])
    np.testing.assert_array_equal(device.bins_keep(lam, 1e-14, n_bins, n_data),
                                  [False, False, False, False, False, False, True, True, True])
    # without a threshold the noise floor alone decides; it scales with lambda_max and with the larger dimension
    np.testing.assert_array_equal(device.bins_keep(lam, 0.0, n_bins, n_data),
                                  [False, False, False, True, True, True, True, True, True])
    np.testing.assert_array_equal(device.bins_keep(lam * 1e-6, 0.0, n_bins, n_data),
                                  [False, False, False, True, True, True, True, True, True])
    np.testing.assert_array_equal(device.bins_keep(lam, 0.0, 100, 2000),
                                  [False, False, False, False, True, True, True, True, True])
    assert not device.bins_keep(np.zeros(3), 0.0, 10, 3).any() and device.bins_keep([], 0.0, 10, 3).shape == (0,)
