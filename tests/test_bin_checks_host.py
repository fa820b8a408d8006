"""Bin checks, the part that needs no GPU: the entry point is declared, ``summarize`` and its plateau rule on reference
ladders of AR(1) bins, ``rebin_bins``, and the refusals that come before the device is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import bin_checks, device
import bin_checks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11


def _summary(bins, **kw):
    lad = R.ladder_ref(bins, **kw)
    return bin_checks.summarize(np.asarray(lad['err2'], dtype=float), np.asarray(lad['skew'], dtype=float),
                                np.asarray(lad['kurt'], dtype=float), len(bins))


def _not_on_a_knife_edge(s):
    """the step of the ladder is clear of the criterion's threshold at k* and at k* - 1 (every eligible level where there
    is no k*): rounding cannot move the outcome"""
    Rk, nb = s['R'], s['n_blocks']
    k = s['plateau_level']
    if k is None:
        ks = [j for j in range(len(Rk) - 1) if nb[j + 1] >= bin_checks.MIN_BLOCKS]
    else:
        ks = [j for j in (k - 1, k) if j >= 0]
    for j in ks:
        margin = Rk[j + 1] - Rk[j] - Rk[j + 1] * np.sqrt(2.0 / (nb[j + 1] - 1.0))
        assert abs(margin) > 1e-6 * Rk[j + 1], (j, margin)


def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert 'mxe_bins_check' in names and 'int  mxe_bins_check(' in header
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_bins_check(' in source
    assert 'mxe_bincheck.hip.h' in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')).read()
    assert mx.check_bins is bin_checks.check_bins and mx.rebin_bins is bin_checks.rebin_bins
    for cls in (mx.TauMaxEnt, mx.ElementwiseMaxEnt, mx.DiagonalMaxEnt, mx.PoormanMaxEnt):
        assert callable(getattr(cls, 'check_bins'))


@pytest.mark.parametrize('m,n', [(300, 40), (1000, 40), (4096, 65)])
def test_white_noise_needs_no_rebinning(m, n):
    s = _summary(R.ar1_bins(m, n, 0.0, SEED))
    _not_on_a_knife_edge(s)
    assert s['plateau_level'] == 0 and s['recommended_block'] == 1
    assert s['R'][0] == 1.0
    assert np.all(s['frac_non_normal'][:3] < 0.1)


def test_rho_05_plateau():
    s = _summary(R.ar1_bins(4096, 40, 0.5, SEED))
    _not_on_a_knife_edge(s)
    assert s['recommended_block'] in (8, 16)
    assert s['recommended_block'] == 1 << s['plateau_level']
    assert 2.5 <= s['R'][s['plateau_level']] <= 2.8                 # (exact 2 tau_int = (1 + rho) / (1 - rho) = 3)


def test_rho_09_plateau():
    s = _summary(R.ar1_bins(16384, 40, 0.9, SEED))
    _not_on_a_knife_edge(s)
    assert s['recommended_block'] == 64 and s['plateau_level'] == 6
    assert 15.4 <= s['R'][6] <= 16.5                                # (exact 19, less the finite-block bias)


def test_rho_099_is_beyond_what_1000_bins_resolve():
    s = _summary(R.ar1_bins(1000, 40, 0.99, SEED))
    _not_on_a_knife_edge(s)
    assert s['plateau_level'] is None and s['recommended_block'] is None


def test_rebin_bins():
    rng = np.random.RandomState(3)
    b = rng.randn(37, 5)
    assert bin_checks.rebin_bins(b, 1) is b
    r = bin_checks.rebin_bins(b, 4)
    assert r.shape == (9, 5)
    np.testing.assert_allclose(r[2], b[8:12].mean(axis=0), rtol=1e-15)
    np.testing.assert_allclose(r[8], b[32:36].mean(axis=0), rtol=1e-15)          # (bin 36 is dropped)
    c = rng.randn(16, 2, 3, 7) + 1j * rng.randn(16, 2, 3, 7)
    rc = bin_checks.rebin_bins(c, 8)
    assert rc.shape == (2, 2, 3, 7) and np.iscomplexobj(rc)
    np.testing.assert_allclose(rc[1], c[8:].mean(axis=0), rtol=1e-14)
    assert bin_checks.rebin_bins(list(map(list, b)), 37).shape == (1, 5)
    for bad in (0, -1, 38):
        with pytest.raises(ValueError):
            bin_checks.rebin_bins(b, bad)


def test_ladder_level_is_level_0_of_the_rebinned_bins():
    b = R.ar1_bins(203, 6, 0.6, 5)
    full = R.ladder_ref(b)
    for k in range(R.n_levels(203)):
        lev0 = R.ladder_ref(bin_checks.rebin_bins(b, 1 << k))
        for name, tol in (('err2', 1e-12), ('skew', 1e-11), ('kurt', 1e-11)):
            # (rebin_bins works in binary64 around an offset of 3000 sigma: that sets the tolerance)
            np.testing.assert_allclose(np.asarray(lev0[name][0], dtype=float), np.asarray(full[name][k], dtype=float),
                                       rtol=tol * 3000, atol=tol * 3000 if name != 'err2' else 0)


@pytest.mark.parametrize('m,L,blocks', [(2, 1, [2]), (3, 1, [3]), (4, 2, [4, 2]),
                                        (1000, 9, [1000, 500, 250, 125, 62, 31, 15, 7, 3])])
def test_levels_blocks_and_block_counts(m, L, blocks):
    assert R.n_levels(m) == L
    s = _summary(np.random.RandomState(1).randn(m, 2))
    assert list(s['n_blocks']) == blocks
    assert list(s['block']) == [1 << k for k in range(L)]
    assert s['err2'].shape == (L, 2) and len(s['R']) == L and len(s['frac_non_normal']) == L
    with pytest.raises(ValueError):
        bin_checks.summarize(np.ones((L + 1, 2)), np.ones((L + 1, 2)), np.ones((L + 1, 2)), m)


def test_a_constant_column_is_nan_and_leaves_the_others_alone():
    b = np.random.RandomState(2).randn(64, 3)
    alone = _summary(b[:, [0, 2]])
    b[:, 1] = 0.25
    s = _summary(b)
    assert np.all(s['err2'][:, 1] == 0.0)
    for name in ('skew', 'kurt', 'inefficiency', 'skew_z', 'kurt_z'):
        assert np.all(np.isnan(s[name][:, 1])), name
        np.testing.assert_array_equal(s[name][:, [0, 2]], alone[name])
    np.testing.assert_array_equal(s['R'], alone['R'])
    np.testing.assert_array_equal(s['frac_non_normal'], alone['frac_non_normal'])
    assert s['plateau_level'] == alone['plateau_level']
    # nothing but constant columns: NaN throughout, no plateau
    z = bin_checks.summarize(np.zeros((6, 2)), np.full((6, 2), np.nan), np.full((6, 2), np.nan), 64)
    assert np.all(np.isnan(z['R'])) and np.all(np.isnan(z['frac_non_normal'])) and z['recommended_block'] is None


def test_z_scores_and_fraction_by_hand():
    # 96 bins: levels of 96, 48, 24, 12, 6, 3 blocks
    L = 6
    err2 = np.ones((L, 4)) * np.array([1.0, 1.5, 1.6, 1.6, 1.6, 1.6])[:, None]
    skew = np.zeros((L, 4))
    kurt = np.zeros((L, 4))
    skew[0] = [0.0, 0.74, 0.76, np.nan]            # 0.75 sqrt(96 / 6) = 3
    kurt[1] = [2.2, -2.0, 0.0, np.nan]             # 2.2 sqrt(48 / 24) = 3.11, -2 sqrt 2 = -2.83
    s = bin_checks.summarize(err2, skew, kurt, 96)
    np.testing.assert_allclose(s['skew_z'][0, :3], np.array([0.0, 0.74, 0.76]) * 4.0, rtol=1e-15)
    np.testing.assert_allclose(s['kurt_z'][1, :3], np.array([2.2, -2.0, 0.0]) * np.sqrt(2.0), rtol=1e-15)
    np.testing.assert_allclose(s['frac_non_normal'], [1 / 3.0, 1 / 3.0, 0, 0, 0, 0], rtol=1e-15)
    np.testing.assert_allclose(s['R'], [1.0, 1.5, 1.6, 1.6, 1.6, 1.6], rtol=1e-15)
    np.testing.assert_allclose(s['inefficiency'][1], 1.5, rtol=1e-15)
    # eligible: 96 and 48 blocks only.  k = 0: 0.5 <= 1.5 sqrt(2 / 47) = 0.309 fails; k = 1 has no eligible successor
    assert s['plateau_level'] is None and s['recommended_block'] is None
    err2[1] = 1.2                                   # 0.2 <= 1.2 sqrt(2 / 47) = 0.2475 holds
    s = bin_checks.summarize(err2, skew, kurt, 96)
    assert s['plateau_level'] == 0 and s['recommended_block'] == 1


def _fail_if_the_device_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(device, 'load_library', boom)
    monkeypatch.setattr(device, 'device_count', boom)


def test_argument_errors_come_before_the_library(monkeypatch):
    _fail_if_the_device_is_touched(monkeypatch)
    b = np.random.RandomState(0).randn(32, 10)
    for bad in (b[0], b[None, None], b + 0j, b[:1], np.zeros((4, 513)), np.zeros((4, 0)), np.zeros((0, 4, 4))):
        with pytest.raises(ValueError, match='bins_check'):
            device.bins_check(bad)
    with pytest.raises(ValueError, match='come together'):
        device.bins_check(b, T=np.eye(10))
    with pytest.raises(ValueError, match='come together'):
        device.bins_check(b, rank=10)
    with pytest.raises(ValueError, match='rank'):
        device.bins_check(b, T=np.eye(10), rank=11)
    with pytest.raises(ValueError, match='rank'):
        device.bins_check(b, T=np.eye(10), rank=-1)
    with pytest.raises(ValueError, match='do not fit'):
        device.bins_check(b, T=np.eye(9), rank=9)
    with pytest.raises(ValueError, match='basis'):
        bin_checks.check_bins(b, basis='tau')
    with pytest.raises(ValueError, match='needs T and rank'):
        bin_checks.check_bins(b, basis='eigen')
    with pytest.raises(ValueError, match='shape'):
        bin_checks.check_bins(b[None])


def test_refusals_of_the_methods_come_before_the_device(monkeypatch):
    _fail_if_the_device_is_touched(monkeypatch)

    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(device, 'bins_check', boom)
    bins = np.random.RandomState(0).randn(32, 10)
    tm = mx.TauMaxEnt()
    with pytest.raises(ValueError, match='set_G_tau_bins'):
        tm.check_bins(bins)
    with pytest.raises(ValueError, match='basis'):
        tm.check_bins(bins, basis='tau')
    with pytest.raises(ValueError, match='shape'):
        tm.check_bins(bins[None], basis='data')
    # an object that holds the statistics of 32 bins of 10 values: bins of another shape are refused in both bases
    st = dict(mean=bins.mean(axis=0), sigma=np.ones(10), T=np.eye(10), rank=10, n_bins=32, sweeps=1)
    object.__setattr__(tm, 'bin_statistics', st)
    for basis in ('eigen', 'data'):
        for other in (bins[:31], bins[:, :9], bins[None], bins.T):
            with pytest.raises(ValueError, match='shape'):
                tm.check_bins(other, basis=basis)
        with pytest.raises(ValueError, match='real'):
            tm.check_bins(bins + 0j, basis=basis)
    for cls in (mx.ElementwiseMaxEnt, mx.DiagonalMaxEnt, mx.PoormanMaxEnt):
        with pytest.raises(ValueError, match='set_G_tau_bins'):
            cls().check_bins(np.zeros((32, 2, 2, 10)))
