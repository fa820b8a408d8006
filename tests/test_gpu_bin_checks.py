"""Bin checks on the device: ``mxe_bins_check`` against its longdouble restatement (tests/bin_checks_ref.py), and
``check_bins`` of the facades end to end.

The gates are those of the sums, not what was measured.  err2 is a recursive sum of <= m non-negative terms: about
m 2^-53 = 1.8e-12 at the largest m used (16384), and forming the deviations costs below 1e-11 with |mean| / sigma <= 1e4:
|d err2| <= 1e-10 err2.  Skewness and kurtosis are sums of signed powers, m eps E|z|^p: |d skew| <= 1e-9, |d kurt| <=
1e-9 (1 + |kurt|), absolute in the standardised variable.  In the eigen basis, against the reference applied to the same
T, err2 gets the absolute term 4 n_data^1.5 eps sigma_max sqrt(err2): the rounding of an inner product of n_data terms,
with tr C <= n_data sigma_max^2.

Measured on an MI355X (largest error over all levels and columns; err2 relative, skew and kurt absolute; every test
prints its own): data basis 4096 x 512: 5.2e-16, 9.2e-16, 3.5e-15; eigen basis 1000 x 65: 2.7e-15, 4.5e-15, 6.3e-15;
Matsubara bins in the eigen basis, the worst: 1.8e-14, 3.7e-14, 1.0e-13.  The table is in DESIGN.md, section 4t."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import bin_checks, device, resampling
import bin_checks_ref as R
from bin_checks_ref import EPS, LD

pytestmark = pytest.mark.gpu

_REF = {}


def _case(m, n, rho, seed):
    """bins and their longdouble ladder in the data basis, computed once per shape"""
    key = (m, n, rho, seed)
    if key not in _REF:
        bins = R.ar1_bins(m, n, rho, seed)
        _REF[key] = (bins, R.ladder_ref(bins))
    return _REF[key]


def _assert_gates(got, ref, what, err2_abs=0.0):
    worst, plain = R.gates(got, ref, err2_abs)
    print('%s: err2 rel %.2e, skew abs %.2e, kurt abs %.2e' % (what, plain['err2'], plain['skew'], plain['kurt']))
    assert worst['err2'] <= 1.0 and worst['skew'] <= 1.0 and worst['kurt'] <= 1.0, (what, worst, plain)


def _eigen_abs(ref_err2, n_data, sigma_max):
    return 4 * n_data ** 1.5 * EPS * sigma_max * np.sqrt(np.asarray(ref_err2, dtype=float))


@pytest.mark.parametrize('m,L', [(2, 1), (3, 1), (4, 2)])
def test_the_shortest_ladders(m, L):
    bins = 3.0 + 1e-3 * np.random.RandomState(m).randn(m, 1)
    got = device.bins_check(bins)
    assert got['levels'] == L and got['err2'].shape == (L, 1)
    _assert_gates(got, R.ladder_ref(bins), 'm = %d' % m)
    if m in (2, 4):                                  # the last level has two blocks: exact opposites
        assert got['skew'][-1, 0] == 0.0 and got['kurt'][-1, 0] == -2.0
        assert got['err2'][-1, 0] > 0.0


@pytest.mark.parametrize('m,n', [(1000, 65), (4096, 512), (16384, 8)])
def test_data_basis_against_longdouble(m, n):
    bins, ref = _case(m, n, 0.5, 7)
    got = device.bins_check(bins)
    assert got['levels'] == R.n_levels(m) and got['err2'].shape == (R.n_levels(m), n)
    _assert_gates(got, ref, '%d x %d' % (m, n))
    # level 0 is the diagonal of the covariance of the mean
    b = np.asarray(bins, dtype=LD)
    X = (b - b.mean(axis=0)) / np.sqrt(LD(m) * (m - 1))
    np.testing.assert_allclose(got['err2'][0], np.asarray((X * X).sum(axis=0), dtype=float), rtol=1e-10)


def test_sets_do_not_see_each_other_and_calls_repeat():
    sets = np.stack([R.ar1_bins(1000, 40, rho, seed) for rho, seed in ((0.0, 1), (0.5, 2), (0.9, 3))])
    t = {}
    got = device.bins_check(sets, timing=t)
    assert t['ms'] > 0.0
    again = device.bins_check(sets)
    for name in ('mean', 'err2', 'skew', 'kurt'):
        assert got[name].tobytes() == again[name].tobytes(), name
    for s in range(3):
        alone = device.bins_check(sets[s])
        for name in ('mean', 'err2', 'skew', 'kurt'):
            assert alone[name].tobytes() == got[name][s].tobytes(), (s, name)
        _assert_gates(dict((k, got[k][s]) for k in ('err2', 'skew', 'kurt')), R.ladder_ref(sets[s]), 'set %d of 3' % s)
    # the same in the eigen basis
    st = device.bins_eig(sets, 0.0)
    T = np.stack([resampling.padded_T(x, 40) for x in st])
    rank = [x['rank'] for x in st]
    got = device.bins_check(sets, T, rank)
    for s in range(3):
        alone = device.bins_check(sets[s], T[s], rank[s])
        for name in ('mean', 'err2', 'skew', 'kurt'):
            assert alone[name].tobytes() == got[name][s].tobytes(), (s, name)


def test_a_constant_column():
    bins, _ = _case(1000, 65, 0.5, 7)
    bins = bins.copy()
    bins[:, 17] = 0.3
    got = device.bins_check(bins)
    assert np.all(got['err2'][:, 17] == 0.0)
    assert np.all(np.isnan(got['skew'][:, 17])) and np.all(np.isnan(got['kurt'][:, 17]))
    assert got['mean'][17] == 0.3
    _assert_gates(got, R.ladder_ref(bins), 'a constant column')
    plain = device.bins_check(_case(1000, 65, 0.5, 7)[0])
    others = np.arange(65) != 17
    for name in ('err2', 'skew', 'kurt'):
        assert got[name][:, others].tobytes() == plain[name][:, others].tobytes(), name


def test_eigen_basis_against_longdouble():
    m, n = 1000, 65
    bins, _ = _case(m, n, 0.5, 7)
    st = device.bins_eig(bins, 0.0)
    assert st['rank'] == n
    T = resampling.padded_T(st, n)
    got = device.bins_check(bins, T, st['rank'])
    assert got['mean'].tobytes() == st['mean'].tobytes()
    assert device.bins_check(bins)['mean'].tobytes() == st['mean'].tobytes()
    smax = float(st['sigma'].max())
    # level 0 reproduces the eigenvalues
    d = np.abs(np.sqrt(got['err2'][0]) - st['sigma'])
    print('level 0 against the eigenvalues: worst |d sigma| / sigma %.2e' % float(np.max(d / st['sigma'])))
    assert np.all(d <= 1e-10 * st['sigma'] + 4 * n ** 1.5 * EPS * smax)
    ref = R.ladder_ref(bins, T, st['rank'])
    _assert_gates(got, ref, 'eigen basis %d x %d' % (m, n), _eigen_abs(ref['err2'], n, smax))


def test_fewer_bins_than_data_values():
    m, n = 30, 40
    bins = R.ar1_bins(m, n, 0.3, 5)
    # (the cut any user of such bins sets: centring an offset of 500 sigma leaves the null direction at ~1e-26 lambda_max)
    st = device.bins_eig(bins, 1e-20)
    assert st['rank'] == 29
    T = resampling.padded_T(st, n)
    got = device.bins_check(bins, T, st['rank'])
    assert got['levels'] == 4
    assert np.all(got['err2'][:, 29:] == 0.0)
    assert np.all(np.isnan(got['skew'][:, 29:])) and np.all(np.isnan(got['kurt'][:, 29:]))
    assert np.all(got['err2'][:, :29] > 0.0)
    ref = R.ladder_ref(bins, T, st['rank'])
    _assert_gates(got, ref, 'rank 29 of 40', _eigen_abs(ref['err2'], n, float(st['sigma'].max())))


def test_refusals_launch_nothing():
    good = R.ar1_bins(32, 10, 0.0, 1)
    bad = good.copy()
    bad[5, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        device.bins_check(bad)
    with pytest.raises(ValueError, match='not finite'):
        device.bins_check(good, np.full((10, 10), np.inf), 10)
    for refused in (np.zeros((4, 513)), good[:1]):
        with pytest.raises((ValueError, mx.MaxEntDeviceError)):
            device.bins_check(refused)
    with pytest.raises((ValueError, mx.MaxEntDeviceError)):
        device.bins_check(good, T=np.eye(10))
    # the library itself: MXE_ERR_ARG, and no output is written
    lib = device.load_library()
    DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)

    def raw(n_bins, n_data, bins, T, rank):
        outs = [np.full(4 * 513, -7.0) for _ in range(4)]
        lev = np.full(1, -7, dtype=np.int32)
        rc = lib.mxe_bins_check(0, 1, n_bins, n_data, bins.ctypes.data_as(DP),
                                None if T is None else T.ctypes.data_as(DP), None if rank is None else rank.ctypes.data_as(IP),
                                *([o.ctypes.data_as(DP) for o in outs] + [lev.ctypes.data_as(IP), None]))
        assert all(np.all(o == -7.0) for o in outs) and lev[0] == -7
        return rc

    eye, r10 = np.ascontiguousarray(np.eye(10)), np.array([10], dtype=np.int32)
    z = np.zeros(4 * 513)
    assert raw(32, 10, np.ascontiguousarray(bad), None, None) == device._MXE_ERR_ARG
    assert raw(4, 513, z, None, None) == device._MXE_ERR_ARG
    assert raw(1, 10, z, None, None) == device._MXE_ERR_ARG
    assert raw(32, 10, good, eye, None) == device._MXE_ERR_ARG
    assert raw(32, 10, good, None, r10) == device._MXE_ERR_ARG
    assert raw(32, 10, good, eye, np.array([11], dtype=np.int32)) == device._MXE_ERR_ARG
    assert raw(32, 10, good, eye * np.nan, r10) == device._MXE_ERR_ARG


def _tm():
    tm = mx.TauMaxEnt(cov_threshold=1e-24)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    return tm


def _summary(lad, m):
    return bin_checks.summarize(*[np.asarray(lad[k], dtype=float) for k in ('err2', 'skew', 'kurt')], n_bins=m)


def _clear_of_the_threshold(s):
    Rk, nb, k = s['R'], s['n_blocks'], s['plateau_level']
    for j in ([j for j in (k - 1, k) if j >= 0] if k is not None else []):
        margin = Rk[j + 1] - Rk[j] - Rk[j + 1] * np.sqrt(2.0 / (nb[j + 1] - 1.0))
        assert abs(margin) > 1e-6 * Rk[j + 1], (j, margin)


def test_end_to_end_tau():
    m, n = 16384, 40
    beta = 10.0
    tau = np.linspace(0.0, beta, n)
    G = -0.5 * (np.exp(-tau * 1.0) + np.exp(-(beta - tau) * 1.0)) / (1.0 + np.exp(-beta))     # a pole at +-1
    bins = G[None, :] + R.ar1_bins(m, n, 0.9, 11, offset=0.0)
    tm = _tm()
    tm.set_G_tau_bins(tau, bins)
    st = tm.bin_statistics
    assert st['rank'] == n
    ref = _summary(R.ladder_ref(bins, resampling.padded_T(st, n), st['rank']), m)
    _clear_of_the_threshold(ref)
    block = ref['recommended_block']
    assert block is not None and block > 1
    tm.logtaker.clear_error_messages()
    out = tm.check_bins(bins)
    assert out['recommended_block'] == block and out['basis'] == 'eigen'
    said = [t for t in tm.logtaker.get_error_messages() if 'rebin_bins' in t]
    assert len(said) == 1 and 'rebin_bins(bins, %d)' % block in said[0] and ('%.3g' % out['R'][out['plateau_level']]) in said[0]
    tm.logtaker.clear_error_messages()
    ref_data = _summary(R.ladder_ref(bins), m)
    _clear_of_the_threshold(ref_data)
    data = tm.check_bins(bins, basis='data')
    assert data['recommended_block'] == ref_data['recommended_block'] == block
    assert len([t for t in tm.logtaker.get_error_messages() if 'rebin_bins' in t]) == 1
    # the object is as it was, and a fresh one checks the data basis without any setter
    assert tm.bin_statistics is st
    assert _tm().check_bins(bins, basis='data')['err2'].tobytes() == data['err2'].tobytes()
    # the ladder at the plateau IS the covariance of the rebinned bins
    k = out['plateau_level']
    t2 = _tm()
    t2.set_G_tau_bins(tau, mx.rebin_bins(bins, block))
    ratio = np.sum(t2.bin_statistics['sigma'] ** 2) / np.sum(st['sigma'] ** 2)
    for o in (out, data):
        mine = np.sum(o['err2'][k]) / np.sum(o['err2'][0])
        print('tr C(rebinned) / tr C(raw) = %.12g, from the ladder %.12g' % (ratio, mine))
        assert abs(mine - ratio) <= 1e-9 * ratio
    # other bins than those that were set are refused
    with pytest.raises(ValueError, match='mean differs'):
        tm.check_bins(bins[::-1] * (1 + 1e-9))
    with pytest.raises(ValueError, match='shape'):
        tm.check_bins(bins[:-1])


def test_matsubara_bins():
    m, n_iw = 1000, 20
    beta = 10.0
    iomega = (2 * np.arange(n_iw) + 1) * np.pi / beta
    G = 0.5 / (1j * iomega - 1.0) + 0.5 / (1j * iomega + 1.0)
    noise = R.ar1_bins(m, 2 * n_iw, 0.5, 4, offset=0.0)
    bins = G[None, :] + noise[:, :n_iw] + 1j * noise[:, n_iw:]
    tm = _tm()
    tm.set_G_iw_bins(iomega, bins, beta=beta)
    st = tm.bin_statistics
    stacked = np.concatenate([bins.real, bins.imag], axis=-1)
    assert stacked.shape == (m, 40) and len(st['mean']) == 40
    out = tm.check_bins(bins)
    ref = R.ladder_ref(stacked, resampling.padded_T(st, 40), st['rank'])
    _assert_gates(out, ref, 'Matsubara, eigen basis', _eigen_abs(ref['err2'], 40, float(st['sigma'].max())))
    data = tm.check_bins(bins, basis='data')
    _assert_gates(data, R.ladder_ref(stacked), 'Matsubara, data basis')
    assert out['mean'].tobytes() == data['mean'].tobytes() == np.asarray(st['mean']).tobytes()


def test_elementwise(monkeypatch):
    m, n = 4096, 20
    beta = 10.0
    tau = np.linspace(0.0, beta, n)
    G = -0.5 * (np.exp(-tau) + np.exp(-(beta - tau))) / (1.0 + np.exp(-beta))
    bins = np.empty((m, 2, 2, n))
    bins[:, 0, 0] = G + R.ar1_bins(m, n, 0.0, 21, offset=0.0)
    bins[:, 1, 1] = G + R.ar1_bins(m, n, 0.5, 22, offset=0.0)
    bins[:, 0, 1] = bins[:, 1, 0] = 0.3 * G + R.ar1_bins(m, n, 0.5, 23, offset=0.0)
    ew = mx.ElementwiseMaxEnt(use_hermiticity=True, use_complex=False, cov_threshold=1e-24)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    ew.set_G_tau_bins(tau, bins)
    calls = []
    real = device.bins_check

    def counted(*a, **k):
        calls.append(np.shape(a[0]))
        return real(*a, **k)
    monkeypatch.setattr(device, 'bins_check', counted)
    log = ew.maxent_diagonal.logtaker
    log.clear_error_messages()
    out = ew.check_bins(bins)
    assert calls == [(3, m, n)]
    assert set(out) == set(ew.bin_statistics) | {'recommended_block'}
    blocks = []
    for key, st in ew.bin_statistics.items():
        ref = R.ladder_ref(bins[:, key[0], key[1], :], resampling.padded_T(st, n), st['rank'])
        _assert_gates(out[key], ref, 'element %s' % (key,), _eigen_abs(ref['err2'], n, float(st['sigma'].max())))
        s = _summary(ref, m)
        _clear_of_the_threshold(s)
        assert out[key]['recommended_block'] == s['recommended_block']
        blocks.append(s['recommended_block'])
    assert out[(0, 0)]['recommended_block'] == 1 and max(blocks) > 1
    assert out['recommended_block'] == max(blocks)
    assert len([t for t in log.get_error_messages() if 'rebin_bins' in t]) == 1
    data = ew.check_bins(bins, basis='data')
    assert calls == [(3, m, n)] * 2
    for key in ew.bin_statistics:
        _assert_gates(data[key], R.ladder_ref(bins[:, key[0], key[1], :]), 'element %s, data basis' % (key,))
