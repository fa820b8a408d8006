"""Resampling error bars, the part that needs no GPU: the two entry points are declared, the tables of multiplicities,
and the refusals of ``resample_errors`` that come before the device is touched."""
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device, resampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_entry_points_are_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    for name in ('mxe_bins_resample', 'mxe_resample_reduce'):
        assert name in names
        assert ('int  %s(' % name) in header
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_bins_resample(' in source and 'extern "C" int mxe_resample_reduce(' in source
    assert 'mxe_resample.hip.h' in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')).read()


def test_jackknife_counts():
    c = resampling.jackknife_counts(37, 1)
    assert c.shape == (37, 37) and c.dtype == np.int32
    assert np.all(c.sum(axis=1) == 36) and np.all(np.diag(c) == 0) and np.all(c + np.eye(37, dtype=int) == 1)
    c = resampling.jackknife_counts(37, 4)
    assert c.shape == (9, 37)
    assert np.all(c[:, 36] == 1)                        # the trailing bin stays in every resample
    assert np.all(c.sum(axis=1) == 33)
    for r in range(9):
        assert np.all(c[r, 4 * r:4 * r + 4] == 0) and c[r].sum() == 33
    assert np.all(c[:, :36].sum(axis=0) == 8)           # every bin of a block is left out exactly once
    for block in (19, 20, 37, 38):
        with pytest.raises(ValueError):
            resampling.jackknife_counts(37, block)
    assert resampling.jackknife_counts(37, 18).shape == (2, 37)
    with pytest.raises(ValueError):
        resampling.jackknife_counts(37, 0)


def test_bootstrap_counts():
    a = resampling.bootstrap_counts(41, 13, seed=5)
    assert a.shape == (13, 41) and a.dtype == np.int32 and np.all(a >= 0)
    assert np.all(a.sum(axis=1) == 41)
    np.testing.assert_array_equal(a, resampling.bootstrap_counts(41, 13, seed=5))
    assert not np.array_equal(a, resampling.bootstrap_counts(41, 13, seed=6))
    np.testing.assert_array_equal(a, np.random.default_rng(5).multinomial(41, np.ones(41) / 41, size=13))
    with pytest.raises(ValueError, match='seed'):
        resampling.bootstrap_counts(41, 13, seed=None)
    with pytest.raises(ValueError, match='seed'):
        resampling.resample_counts('bootstrap', 41, n_resamples=13)


def test_the_full_sample_leads_the_table():
    for c in (resampling.resample_counts('jackknife', 12, block=3), resampling.resample_counts('bootstrap', 12, n_resamples=5, seed=1)):
        assert np.all(c[0] == 1) and c.dtype == np.int32
    assert resampling.resample_counts('jackknife', 12, block=3).shape == (5, 12)
    with pytest.raises(ValueError):
        resampling.resample_counts('subsample', 12)


def test_scales_and_alpha_choice():
    assert resampling.spread_scale('jackknife', 16) == 15.0 / 16.0
    assert resampling.spread_scale('bootstrap', 16) == 1.0 / 15.0
    tm = mx.TauMaxEnt()
    assert resampling.choose_slot(None, tm.analyzers, 8) == (resampling.SLOTS.index(tm.analyzers[0].name), None)
    assert resampling.choose_slot('Chi2Curvature', tm.analyzers, 8) == (1, None)
    assert resampling.choose_slot('EntropyAnalyzer', tm.analyzers, 8) == (2, None)
    assert resampling.choose_slot(-1, tm.analyzers, 8) == (None, 7)
    for bad in ('BryanAnalyzer', 'bryan', 8, [1, 2]):
        with pytest.raises(ValueError):
            resampling.choose_slot(bad, tm.analyzers, 8)


def _fail_if_the_device_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(device, 'bins_resample', boom)
    monkeypatch.setattr(device, 'load_library', boom)


def test_refusals_come_before_the_device(monkeypatch):
    _fail_if_the_device_is_touched(monkeypatch)
    bins = np.random.RandomState(0).randn(32, 10)
    tm = mx.TauMaxEnt()
    with pytest.raises(ValueError, match='set_G_tau_bins'):
        tm.resample_errors(bins)
    # an object that holds the statistics of 32 bins of 10 values: bins of another shape are refused
    st = dict(mean=bins.mean(axis=0), sigma=np.ones(10), T=np.eye(10), rank=10, n_bins=32, sweeps=1)
    object.__setattr__(tm, 'bin_statistics', st)
    for other in (bins[:31], bins[:, :9], bins[None], bins.T):
        with pytest.raises(ValueError, match='shape'):
            tm.resample_errors(other)
    with pytest.raises(ValueError, match='real'):
        tm.resample_errors(bins + 0j)

    class Mine(object):
        def minimize(self, function, v0):
            return v0
    tm.minimizer = Mine()
    with pytest.raises(NotImplementedError, match='Minimizer'):
        tm.resample_errors(bins)
    ew = mx.ElementwiseMaxEnt()
    with pytest.raises(ValueError, match='set_G_tau_bins'):
        ew.resample_errors(np.zeros((32, 2, 2, 10)))
    pm = mx.PoormanMaxEnt()
    with pytest.raises(NotImplementedError, match='default model'):
        pm.resample_errors(np.zeros((32, 2, 2, 10)))
