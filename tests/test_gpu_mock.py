"""Parametric bootstrap on the device: ``mxe_mock_data`` against its numpy mirror (``mock.mock_rows``) with the derivable
bound of its product, ``mxe_resample_quantiles`` against ``numpy.quantile``, and ``parametric_bootstrap`` end to end
against a loop of ``run()`` calls over the same mock data.  Fixture of the bootstrap test: tests/golden/bins.npz.

The gates.  (1) generator: per entry |G_dev - G_mirror| <= (n_omega + 2) eps (|K| |H0|)_i + err_i 1e-13 + eps |G| -- both
sides form K H0 with at most n_omega roundings of half an eps each, the normals agree to the project's gate of
``mxe_normals`` against its mirror, the last term is the rounding of the sum; with a rotation the first term is carried
through |T| and the ``4 n_data eps |T| |m|`` of ``bins_resample_ref`` is added.  (3) quantiles: the bits of the order
statistic where (n - 1) q is an integer, else 2 eps max(|x_lo|, |x_hi|): a rounding each of the difference, the product
and the sum."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, mock, posterior, resampling, synthetic
from resample_ref import reduce_ref, EPS, LD

pytestmark = pytest.mark.gpu

GATE = 1e-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
UP = ctypes.POINTER(ctypes.c_uint64)
Q5 = (0.0, 0.16, 0.5, 0.84, 1.0)
Q3 = (0.16, 0.5, 0.84)
WINDOWS = [(-3.0, 0.0), (0.0, 3.0)]


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


# ---- 1. the generator against the mirror ----------------------------------------------------------------------------------
def _sets(shape, with_T):
    n_sets, n_data, n_omega, n_mock = shape
    rng = np.random.RandomState(n_data + 7 * n_omega + with_T)
    K = np.ascontiguousarray(rng.randn(n_data, n_omega))
    H0 = np.ascontiguousarray(rng.rand(n_sets, n_omega) / n_omega)
    err = np.ascontiguousarray(0.01 * (1.0 + rng.rand(n_sets, n_data)))
    streams = [3 * s + 1 + (2 ** 40 if s == 0 else 0) for s in range(n_sets)]         # (one above 32 bits)
    T = rank = None
    if with_T:
        T = np.stack([np.linalg.qr(rng.randn(n_data, n_data))[0].T for _ in range(n_sets)])
        rank = np.full(n_sets, n_data, dtype=np.int32)
        rank[-1] = n_data // 2                              # a rank below n_data
        T[-1, rank[-1]:] = 0.0
    return K, H0, err, streams, T, rank


@pytest.mark.parametrize('with_T', [False, True])
@pytest.mark.parametrize('shape', [(3, 37, 70, 5), (1, 1, 1, 2), (2, 64, 128, 17)])
def test_generator_against_the_mirror(shape, with_T):
    n_sets, n_data, n_omega, n_mock = shape
    K, H0, err, streams, T, rank = _sets(shape, with_T)
    seed = 20261019
    t = {}
    got = device.mock_data(K, H0, err, seed, streams, n_mock, T=T, rank=rank, timing=t)
    again = device.mock_data(K, H0, err, seed, streams, n_mock, T=T, rank=rank)
    assert t['ms'] > 0.0
    assert got['G'].shape == (n_sets, n_mock, n_data) and got['model'].shape == (n_sets, n_data)
    worst = 0.0
    for s in range(n_sets):
        first = (n_omega + 2) * EPS * (np.abs(K) @ np.abs(H0[s]))
        m = np.asarray(K, dtype=LD) @ np.asarray(H0[s], dtype=LD)
        r = n_data
        if with_T:
            r = int(rank[s])
            first = np.abs(T[s]) @ first + 4 * n_data * EPS * (np.abs(T[s]) @ np.asarray(np.abs(m), dtype=float))
            m = np.asarray(T[s], dtype=LD) @ m
            assert not np.any(got['G'][s][:, r:]) and not np.any(got['model'][s][r:])         # rows >= rank: exact zeros
        assert np.all(np.abs(np.asarray(got['model'][s] - m, dtype=float)) <= first), s
        mirror = mock.mock_rows(K, H0[s], err[s], seed, streams[s], n_mock, T=None if T is None else T[s],
                                rank=None if T is None else r)
        bound = first[None, :] + err[s][None, :] * 1e-13 + EPS * np.abs(mirror)
        diff = np.abs(got['G'][s] - mirror)
        with np.errstate(all='ignore'):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, diff / bound, 0.0))))
        assert np.all(diff <= bound), s
        # the noise is the generator's: (G - model) / err against the normals of the stream
        z = posterior.sample_normals(seed, streams[s], n_mock, n_data)
        assert np.all(np.abs((got['G'][s] - got['model'][s])[:, :r] - (err[s] * z)[:, :r]) <= err[s][:r] * 1e-13 + 2 * EPS * np.abs(mirror[:, :r]))
    for k in ('model', 'G'):
        assert got[k].tobytes() == again[k].tobytes(), k                  # two calls: the same bits
    # a set alone: the bits it has in the batch; fewer mocks: a prefix
    s = n_sets - 1
    alone = device.mock_data(K, H0[s], err[s], seed, [streams[s]], n_mock, T=None if T is None else T[s:s + 1],
                             rank=None if T is None else rank[s:s + 1])
    assert alone['G'].tobytes() == got['G'][s].tobytes() and alone['model'].tobytes() == got['model'][s].tobytes()
    fewer = device.mock_data(K, H0, err, seed, streams, n_mock - 1, T=T, rank=rank)
    assert fewer['G'].tobytes() == np.ascontiguousarray(got['G'][:, :n_mock - 1]).tobytes()
    print('shape %s, T %s: worst error / bound = %.3f, %.3f ms' % (shape, with_T, worst, t['ms']))


def test_generator_chunks_of_mocks_agree():
    """more mocks than one workgroup writes: every chunk forms the model again, and forms the same bits"""
    K, H0, err, streams, T, rank = _sets((2, 20, 33, 0), True)
    got = device.mock_data(K, H0, err, 5, streams, 41, T=T, rank=rank)
    few = device.mock_data(K, H0, err, 5, streams, 3, T=T, rank=rank)
    assert few['model'].tobytes() == got['model'].tobytes()
    assert few['G'].tobytes() == np.ascontiguousarray(got['G'][:, :3]).tobytes()
    for s in range(2):
        mirror = mock.mock_rows(K, H0[s], err[s], 5, streams[s], 41, T=T[s], rank=rank[s])
        first = np.abs(T[s]) @ ((33 + 2) * EPS * (np.abs(K) @ np.abs(H0[s]))) + 4 * 20 * EPS * (np.abs(T[s]) @ np.abs(K @ H0[s]))
        assert np.all(np.abs(got['G'][s] - mirror) <= first[None, :] + err[s][None, :] * 1e-13 + EPS * np.abs(mirror))


# ---- 2. refusals write nothing ----------------------------------------------------------------------------------------------
def _raw_mock(n_sets, n_mock, n_data, n_omega, K, H0, err, T, rank, streams, outs):
    lib = device.load_library()
    st = np.ascontiguousarray(streams, dtype=np.uint64)
    return lib.mxe_mock_data(0, n_sets, n_mock, n_data, n_omega, K.ctypes.data_as(DP), H0.ctypes.data_as(DP),
                             err.ctypes.data_as(DP), None if T is None else T.ctypes.data_as(DP),
                             None if rank is None else rank.ctypes.data_as(IP), 9, st.ctypes.data_as(UP),
                             outs[0].ctypes.data_as(DP), outs[1].ctypes.data_as(DP), None)


def test_mock_data_refuses_bad_arguments_and_touches_nothing():
    n_sets, n_data, n_omega, n_mock = 2, 5, 9, 4
    K, H0, err, streams, T, rank = _sets((n_sets, n_data, n_omega, n_mock), True)

    def outs():
        return [np.full((n_sets, n_data), 7.0), np.full((n_sets, n_mock, n_data), 7.0)]

    def refused(rc, o):
        return rc == -1 and all(np.all(a == 7.0) for a in o)
    o = outs()
    assert _raw_mock(n_sets, n_mock, n_data, n_omega, K, H0, err, T, rank, streams, o) == 0 and not np.any(o[1][0] == 7.0)
    cases = {}
    for v in (np.nan, np.inf):
        for name, a, at in (('K', K, (1, 2)), ('H0', H0, (1, 3)), ('err', err, (0, 4)), ('T', T, (0, 1, 1))):
            b = a.copy(); b[at] = v
            cases['%s in %s' % (v, name)] = {name: b}
    for v in (0.0, -1e-3):
        e = err.copy(); e[1, 2] = v
        cases['err = %g' % v] = dict(err=e)
    for bad in (-1, n_data + 1):
        r = rank.copy(); r[1] = bad
        cases['rank %d' % bad] = dict(rank=r)
    cases['T without rank'] = dict(rank=None)
    for name, kw in cases.items():
        a = dict(K=K, H0=H0, err=err, T=T, rank=rank)
        a.update(kw)
        o = outs()
        assert refused(_raw_mock(n_sets, n_mock, n_data, n_omega, a['K'], a['H0'], a['err'], a['T'], a['rank'], streams, o), o), name
    o = outs()
    assert refused(_raw_mock(n_sets, 0, n_data, n_omega, K, H0, err, T, rank, streams, o), o)              # n_mock < 1
    assert refused(_raw_mock(0, n_mock, n_data, n_omega, K, H0, err, T, rank, streams, o), o)              # sizes below 1
    assert refused(_raw_mock(n_sets, n_mock, 0, n_omega, K, H0, err, T, rank, streams, o), o)
    assert refused(_raw_mock(n_sets, n_mock, n_data, 0, K, H0, err, T, rank, streams, o), o)
    # the wrapper refuses the same before the library is asked
    for kw in (dict(K=cases['nan in K']['K']), dict(H0=cases['inf in H0']['H0']), dict(err=cases['err = 0']['err']), dict(n_mock=0)):
        a = dict(K=K, H0=H0, err=err, seed=9, streams=streams, n_mock=n_mock, T=T, rank=rank)
        a.update(kw)
        with pytest.raises((ValueError, device.MaxEntDeviceError)):
            device.mock_data(**a)


# ---- 3. quantiles against numpy ------------------------------------------------------------------------------------------------
def _ctx(n_omega):
    n_s = min(n_omega, 4)
    rng = np.random.RandomState(n_omega)
    return device.DeviceContext(rng.randn(6, n_s), np.linspace(1.0, 0.1, n_s), np.linalg.qr(rng.randn(n_omega, n_s))[0])


def _check_quantiles(got, rows, q, scale=None, slack=0.0):
    """``got`` (n_q, n) against the type-7 quantiles of the finite rows of ``rows``, both divided by ``scale`` (one more
    rounding): equal bits where (n - 1) q is an integer, else gate 3 (+ ``slack`` |x_hi - x_lo|)"""
    v = rows[np.all(np.isfinite(rows), axis=1)]
    if len(v) == 0:
        assert np.all(np.isnan(got))
        return
    x = np.sort(v, axis=0)
    n = len(x)
    ref = np.quantile(v, q, axis=0)
    divided = scale is not None
    scale = np.asarray(scale, dtype=float) if divided else 1.0
    for iq, qq in enumerate(q):
        h = (n - 1) * qq
        lo = int(np.floor(h))
        if h == lo and slack == 0.0:
            assert (x[lo] / scale).tobytes() == np.ascontiguousarray(got[iq]).tobytes(), (n, qq)
            assert (ref[iq] / scale).tobytes() == np.ascontiguousarray(got[iq]).tobytes(), (n, qq)
        else:
            hi = min(lo + 1, n - 1)
            bound = (2 * EPS * np.maximum(np.abs(x[lo]), np.abs(x[hi])) + slack * np.abs(x[hi] - x[lo])) / scale
            if divided:
                bound = bound + EPS * np.abs(ref[iq] / scale)
            assert np.all(np.abs(got[iq] - ref[iq] / scale) <= bound), (n, qq)


@pytest.mark.parametrize('n_omega', [1, 63, 130])
def test_quantiles_against_numpy(n_omega):
    rng = np.random.RandomState(11 + n_omega)
    cap = device.QUANTILE_MAX_ROWS
    sizes = [1, 2, 3, 64, 65, 0, 257, 2, cap]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    H = np.ascontiguousarray(rng.randn(int(off[-1]), n_omega) * np.linspace(1.0, 1e-3, n_omega)[None, :])
    H[off[3]:off[4]] = np.round(H[off[3]:off[4]], 1) + 0.0  # duplicated values (the tail columns are all 0; + 0.0: no -0.0)
    H[off[6] + 5] = H[off[6] + 9]                           # a duplicated row
    H[off[4] + 3, n_omega // 2] = np.nan                    # rows that are left out
    H[off[4] + 64, 0] = np.inf
    H[off[6] + 200, n_omega - 1] = -np.inf
    H[off[7], 0] = np.nan                                   # a group with no finite row
    H[off[7] + 1, n_omega - 1] = np.inf
    ctx = _ctx(n_omega)
    try:
        t = {}
        got = ctx.resample_quantiles(off, Q5, H=H, timing=t)
        assert got['q'].shape == (len(sizes), 5, n_omega) and t['ms'] > 0.0
        red = ctx.resample_reduce(off, np.ones(len(sizes)), H=H, want=())
        assert got['used'].tolist() == red['used'].tolist() == [1, 2, 3, 64, 63, 0, 256, 0, cap]
        for gi in range(len(sizes)):
            _check_quantiles(got['q'][gi], H[off[gi]:off[gi + 1]], Q5)
        assert np.all(np.isnan(got['q'][5])) and np.all(np.isnan(got['q'][7]))
        again = ctx.resample_quantiles(off, Q5, H=H)
        assert got['q'].tobytes() == again['q'].tobytes() and got['used'].tobytes() == again['used'].tobytes()
        # a group alone, and among other groups: the same bits
        for gi in (2, 4, 6):
            sub = ctx.resample_quantiles([0, sizes[gi]], Q5, H=H[off[gi]:off[gi + 1]])
            assert sub['q'][0].tobytes() == got['q'][gi].tobytes() and sub['used'][0] == got['used'][gi]
        # one probability, not sorted ones
        one = ctx.resample_quantiles(off[:5], [0.84, 0.16], H=H[:off[4]])
        assert one['q'][:, 0].tobytes() == np.ascontiguousarray(got['q'][:4, 3]).tobytes()
        assert one['q'][:, 1].tobytes() == np.ascontiguousarray(got['q'][:4, 1]).tobytes()
        # one row more than the cap: refused, nothing written
        big = np.ascontiguousarray(rng.randn(cap + 1, n_omega))
        with pytest.raises(device.MaxEntDeviceError, match='limit|LIMIT|exceed'):
            ctx.resample_quantiles([0, cap + 1], Q5, H=big)
        out_q, out_used = np.full((1, 5, n_omega), 7.0), np.full(1, 7, dtype=np.int32)
        o2 = np.array([0, cap + 1], dtype=np.int32)
        qq = np.array(Q5)
        rc = ctx._lib.mxe_resample_quantiles(ctx._h, 1, o2.ctypes.data_as(IP), big.ctypes.data_as(DP), None, 5, qq.ctypes.data_as(DP),
                                             out_q.ctypes.data_as(DP), out_used.ctypes.data_as(IP), None)
        assert rc == -5 and np.all(out_q == 7.0) and out_used[0] == 7
        bad = np.array([0.5, 1.5])
        rc = ctx._lib.mxe_resample_quantiles(ctx._h, 1, np.array([0, 2], dtype=np.int32).ctypes.data_as(IP), big.ctypes.data_as(DP), None, 2,
                                             bad.ctypes.data_as(DP), out_q.ctypes.data_as(DP), out_used.ctypes.data_as(IP), None)
        assert rc == -1 and np.all(out_q == 7.0) and out_used[0] == 7
        # without a launch there are no rows on the device to read
        with pytest.raises(device.MaxEntDeviceError, match='call order'):
            ctx.resample_quantiles([0, 2], [0.5], problem_index=[0, 1])
        with pytest.raises(ValueError):
            ctx.resample_quantiles([0, 2], [1.5], H=H[:2])
        with pytest.raises(ValueError):
            ctx.resample_quantiles([1, 2], [0.5], H=H[:2])
    finally:
        ctx.close()
    print('n_omega %d: %d rows in %d groups, %.3f ms' % (n_omega, off[-1], len(sizes), t['ms']))


# ---- 4. one element equals a loop of run() calls ---------------------------------------------------------------------------
def _single(**kw):
    tm = mx.TauMaxEnt(**kw)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    return tm


def _check_against_own_samples(out, delta, rowsH, n_win, n_fun, q=Q3):
    """A_mean, A_err, window_*, functional_* against the longdouble reduction of the samples of the same call, the bands
    against numpy's quantiles of them"""
    Hs = out['samples']['H']
    n = Hs.shape[0]
    assert out['n_used'] == n
    ref = reduce_ref(Hs, [0, n], [resampling.spread_scale('parametric', n)], rowsH)
    d = np.asarray(delta, dtype=LD)
    A_mean, A_var = ref['mean'][0] / d, ref['var'][0] / d ** 2
    assert np.all(np.abs(np.asarray(out['A_mean'] - A_mean, dtype=float)) <= ref['mean_bound'][0] / delta + EPS * np.abs(out['A_mean']))
    assert np.all(np.abs(np.asarray(out['A_err'] ** 2 - A_var, dtype=float)) <= ref['var_bound'][0] / delta ** 2 + 4 * EPS * out['A_err'] ** 2)
    val = np.concatenate([out['window_weight'], out['functional_value']])
    err = np.concatenate([out['window_err'], out['functional_err']])
    assert np.all(np.abs(np.asarray(val - ref['fmean'][0], dtype=float)) <= ref['fmean_bound'][0])
    var_ref = np.asarray(np.diagonal(ref['fcov'][0]), dtype=float)
    assert np.all(np.abs(err ** 2 - var_ref) <= np.diagonal(ref['fcov_bound'][0]) + 4 * EPS * var_ref)
    assert np.all(np.abs(np.asarray(out['samples']['functional'] - ref['fval'], dtype=float)) <= ref['fval_bound'])
    assert np.all(err > 0) and np.all(out['A_err'] > 0)
    np.testing.assert_array_equal(out['quantiles'], q)
    _check_quantiles(out['A_quantiles'], Hs, q, scale=delta)
    fq = np.quantile(out['samples']['functional'], q, axis=0)
    np.testing.assert_array_equal(np.concatenate([out['window_quantiles'], out['functional_quantiles']], axis=1), fq)
    np.testing.assert_array_equal(out['A_bias'], out['A_mean'] - out['A'])
    assert out['chi2_p_value'] == mock.chi2_p_value(out['chi2'], out['chi2_samples'])
    assert 0.0 < out['chi2_p_value'] <= 1.0


@pytest.fixture(scope='module')
def single_job():
    """the TauMaxEnt of test 4, its result and its parametric bootstrap: made once, shared, left unchanged"""
    tau, omega, K, G = synthetic.single_G(40, 60)
    tm = _single()
    tm.set_G_tau_data(tau, G)
    tm.set_error(synthetic.SIGMA)
    res = tm.run()
    w = np.asarray(tm.omega)
    F = np.stack([w, w ** 2])
    G_before, err_before = np.array(tm.G), np.array(tm.err)
    out = tm.parametric_bootstrap(res, n_mock=6, seed=7, windows=WINDOWS, functionals=F, keep_samples=True, keep_data=True)
    assert np.array_equal(G_before, tm.G) and np.array_equal(err_before, tm.err)        # the object is as it was
    return dict(tau=tau, G=G, tm=tm, res=res, F=F, out=out)


def test_single_element_equals_a_loop_of_runs(single_job):
    tau, tm, res, F, out = (single_job[k] for k in ('tau', 'tm', 'res', 'F', 'out'))
    name = tm.analyzers[0].name
    assert out['method'] == 'parametric' and out['n_mock'] == 6 and out['seed'] == 7 and out['n_used'] == 6
    assert out['info']['left_out'] == [] and out['info']['audit_max'] < GATE and out['info']['launches'] == 1
    assert out['samples']['H'].shape == (6, 60) and out['G_mock'].shape == (6, 40) and out['A_quantiles'].shape == (3, 60)
    pick0 = int(res.analyzer_results[name]['alpha_index'])
    assert out['alpha_index'] == pick0
    # the mocks: drawn from the row of the result at that pick
    H0 = np.asarray(res.H)[pick0]
    Kj, err = np.asarray(tm.K.K), np.asarray(tm.err)
    mirror = mock.mock_rows(Kj, H0, err, 7, 0, 6)
    first = (60 + 2) * EPS * (np.abs(Kj) @ np.abs(H0))
    assert np.all(np.abs(out['G_mock'] - mirror) <= first[None, :] + err[None, :] * 1e-13 + EPS * np.abs(mirror))
    assert rel_l2(out['A'] * tm.omega.delta, H0) < GATE                  # chain 0 is the run() of the object itself
    assert out['chi2'] == pytest.approx(float(np.asarray(res.chi2)[pick0]), rel=1e-6)
    # the reference loop: one fresh object per mock
    worst = 0.0
    for k in range(6):
        th = _single()
        th.set_G_tau_data(tau, out['G_mock'][k])
        th.set_error(synthetic.SIGMA)
        r = th.run()
        pick = int(r.analyzer_results[name]['alpha_index'])
        assert np.all(r.converged) and th.last_launch['audit_max'] < GATE
        assert out['alpha_index_samples'][k] == pick, k
        e = float(rel_l2(out['samples']['H'][k], np.asarray(r.H)[pick]))
        worst = max(worst, e)
        assert e < GATE, (k, e)
        assert out['chi2_samples'][k] == pytest.approx(float(np.asarray(r.chi2)[pick]), rel=1e-6)
    print('mocks vs loop of run(): worst rel. L2 %.2e, audit of the launch %.2e, p = %.3f' %
          (worst, out['info']['audit_max'], out['chi2_p_value']))
    rowsH = np.concatenate([resampling.window_rows(tm.omega, WINDOWS), F])
    _check_against_own_samples(out, tm.omega.delta, rowsH, 2, 2)


def test_single_element_modes_and_refusals(single_job):
    tau, G, tm, res, out = (single_job[k] for k in ('tau', 'G', 'tm', 'res', 'out'))
    fx = tm.parametric_bootstrap(res, n_mock=6, seed=7, alpha_mode='fixed', keep_data=True, quantiles=None)
    assert np.all(fx['alpha_index_samples'] == fx['alpha_index']) and fx['alpha_index'] == out['alpha_index']
    assert fx['G_mock'].tobytes() == out['G_mock'].tobytes()              # the same seed: the same mocks
    assert 'A_quantiles' not in fx and 'quantiles' not in fx and 'A_bias' in fx
    a3 = tm.parametric_bootstrap(res, n_mock=4, seed=7, alpha=3, windows=WINDOWS)
    assert a3['alpha_index'] == 3 and np.all(a3['alpha_index_samples'] == 3) and a3['n_used'] == 4
    assert a3['alpha'] == pytest.approx(float(res.alpha[3]), rel=1e-13)
    assert a3['window_quantiles'].shape == (3, 2)
    # without a result: run() first -- the same job, the same mocks to the gate of the solver
    own = tm.parametric_bootstrap(n_mock=6, seed=7, keep_data=True, pointwise=False, windows=WINDOWS)
    assert 'A_mean' not in own and 'A_bias' not in own and np.max(rel_l2(own['G_mock'], out['G_mock'])) < GATE
    # a result of another job (data changed since) is refused before anything is launched
    other = _single()
    other.set_G_tau_data(tau, G)
    other.set_error(synthetic.SIGMA)
    old = other.run()
    launch = other.last_launch
    other.set_G_tau_data(tau, G + 1e-7)
    other.set_error(synthetic.SIGMA)
    with pytest.raises(ValueError, match='data'):
        other.parametric_bootstrap(old, n_mock=4, seed=1)
    assert other.last_launch is launch
    other.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=7)
    with pytest.raises(ValueError, match='alphas'):
        other.parametric_bootstrap(old, n_mock=4, seed=1)


# ---- 5. a covariance (rotated kernel) and a preblur -------------------------------------------------------------------------
def test_covariance_draws_in_the_eigenbasis():
    tau, omega, K, G = synthetic.single_G(40, 60)
    i = np.arange(40)
    cov = synthetic.SIGMA ** 2 * 0.5 ** np.abs(i[:, None] - i[None, :])
    tm = _single()
    tm.set_G_tau_data(tau, G)
    tm.set_cov(cov)
    res = tm.run()
    G_before = np.array(tm.G)
    out = tm.parametric_bootstrap(res, n_mock=5, seed=3, keep_samples=True, keep_data=True, windows=WINDOWS)
    assert np.array_equal(G_before, tm.G) and out['n_used'] == 5 and out['info']['audit_max'] < GATE
    Kj, err = np.asarray(tm.K.K), np.asarray(tm.err)                     # the rotated kernel, the roots of the eigenvalues
    assert tm.K.rotation is not None and Kj.shape == (len(err), 60) and out['G_mock'].shape == (5, len(err))
    H0 = np.asarray(res.H)[out['alpha_index']]
    mirror = mock.mock_rows(Kj, H0, err, 3, 0, 5)
    first = (60 + 2) * EPS * (np.abs(Kj) @ np.abs(H0))
    assert np.all(np.abs(out['G_mock'] - mirror) <= first[None, :] + err[None, :] * 1e-13 + EPS * np.abs(mirror))
    _check_quantiles(out['A_quantiles'], out['samples']['H'], Q3, scale=tm.omega.delta)
    # the mocks scatter about the rotated data like the data's own noise: chi2 of a mock against the model ~ n_data
    z = (out['G_mock'] - Kj @ H0) / err
    assert 0.3 < np.mean(z ** 2) < 3.0


def test_preblur_refers_to_A():
    tau, omega, K, G = synthetic.single_G(40, 60)
    tm = _single()
    tm.A_of_H = mx.PreblurA_of_H(b=0.2, omega=tm.omega)
    tm.K = mx.PreblurKernel(K=tm.K, b=0.2)
    tm.set_G_tau_data(tau, G)
    tm.set_error(synthetic.SIGMA)
    res = tm.run()
    out = tm.parametric_bootstrap(res, n_mock=8, seed=4, windows=WINDOWS, keep_samples=True, keep_data=True)
    assert out['n_used'] == 8
    # the hidden image is what the mocks are drawn from: the job's kernel contains B
    H0 = np.asarray(res.H)[out['alpha_index']]
    Kj, err = np.asarray(tm.K.K), np.asarray(tm.err)
    mirror = mock.mock_rows(Kj, H0, err, 4, 0, 8)
    first = (60 + 2) * EPS * (np.abs(Kj) @ np.abs(H0))
    assert np.all(np.abs(out['G_mock'] - mirror) <= first[None, :] + err[None, :] * 1e-13 + EPS * np.abs(mirror))
    B = np.asarray(tm.maxent_loop.A_of_H.matrix())
    A_s = out['samples']['H'] @ B.T
    np.testing.assert_allclose(out['A_mean'], A_s.mean(axis=0), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(out['A_err'], np.sqrt(((A_s - A_s.mean(axis=0)) ** 2).sum(axis=0) / 7.0), rtol=1e-8, atol=1e-13)
    np.testing.assert_allclose(out['A_quantiles'], np.quantile(A_s, Q3, axis=0), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(out['A'], B @ H0, rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(out['A_bias'], out['A_mean'] - out['A'])
    inside = resampling.window_rows(tm.omega, WINDOWS)
    w_s = (A_s * tm.omega.delta) @ inside.T
    np.testing.assert_allclose(out['window_weight'], w_s.mean(axis=0), rtol=1e-10)
    np.testing.assert_allclose(out['window_quantiles'], np.quantile(w_s, Q3, axis=0), rtol=1e-10)


# ---- 6. ElementwiseMaxEnt ---------------------------------------------------------------------------------------------------
def _ew(Gmat, tau, cls=None, **kw):
    ew = (cls or mx.ElementwiseMaxEnt)(**kw)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    ew.set_error(synthetic.SIGMA)
    return ew


def test_elementwise_matrix_and_its_partners():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 40, 60)
    ew = _ew(Gmat, tau)
    res = ew.run()
    out = ew.parametric_bootstrap(res, n_mock=6, seed=7, windows=WINDOWS, keep_samples=True, keep_data=True)
    info = out['info']
    assert out['method'] == 'parametric' and out['n_mock'] == 6 and info['audit_max'] < GATE
    assert info['n_elements'] == [2, 1] and info['mock_calls'] == 1 and info['launches'] == 2
    assert out['A_quantiles'].shape == (2, 2, 3, 60) and out['window_quantiles'].shape == (2, 2, 3, 2)
    assert out['samples']['H'].shape == (2, 2, 6, 60) and out['G_mock'].shape == (2, 2, 6, 40)
    assert out['chi2_samples'].shape == (2, 2, 6) and out['chi2_p_value'].shape == (2, 2) and np.all(out['n_used'] == 6)
    for k in ('A', 'A_err', 'A_mean', 'A_bias', 'A_quantiles', 'window_weight', 'window_quantiles', 'alpha_index', 'chi2',
              'chi2_samples', 'G_mock'):
        np.testing.assert_array_equal(out[k][1, 0], out[k][0, 1])       # the partner from hermiticity
    delta = ew.omega.delta
    for (i, j) in ((0, 0), (0, 1), (1, 1)):
        _check_quantiles(out['A_quantiles'][i, j], out['samples']['H'][i, j], Q3, scale=delta)
        np.testing.assert_array_equal(out['A_bias'][i, j], out['A_mean'][i, j] - out['A'][i, j])
        assert out['chi2_p_value'][i, j] == mock.chi2_p_value(out['chi2'][i, j], out['chi2_samples'][i, j])
        # every element draws from its own stream
        H0 = np.asarray(res.H)[i, j][out['alpha_index'][i, j]]
        Kj = np.asarray(ew.maxent_diagonal.K.K)
        mirror = mock.mock_rows(Kj, H0, synthetic.SIGMA, 7, posterior.stream_id(2 * i + j, 0, 1, 0), 6)
        first = (60 + 2) * EPS * (np.abs(Kj) @ np.abs(H0))
        assert np.all(np.abs(out['G_mock'][i, j] - mirror) <= first[None, :] + synthetic.SIGMA * 1e-13 + EPS * np.abs(mirror)), (i, j)
    # element (0, 0) alone: the same mocks, the same outputs
    tm = _single()
    tm.set_G_tau_data(tau, Gmat[0, 0])
    tm.set_error(synthetic.SIGMA)
    r1 = tm.run()
    one = tm.parametric_bootstrap(r1, n_mock=6, seed=7, windows=WINDOWS, keep_samples=True, keep_data=True)
    dH0 = np.abs(np.asarray(r1.H)[one['alpha_index']] - np.asarray(res.H)[0, 0][out['alpha_index'][0, 0]])
    Kj = np.asarray(tm.K.K)
    print('element (0, 0) alone and in the matrix: largest difference of the hidden images %.2e' % dH0.max())
    # (the same normals; the models differ by K times the difference of the two hidden images, two solves of one problem)
    assert np.all(np.abs(one['G_mock'] - out['G_mock'][0, 0]) <= (np.abs(Kj) @ dH0)[None, :] + 4 * EPS * np.abs(one['G_mock']))
    assert one['alpha_index'] == out['alpha_index'][0, 0]
    np.testing.assert_array_equal(one['alpha_index_samples'], out['alpha_index_samples'][0, 0])
    assert np.all(rel_l2(one['samples']['H'], out['samples']['H'][0, 0]) < GATE)
    assert rel_l2(one['A_mean'], out['A_mean'][0, 0]) < GATE
    assert np.all(rel_l2(one['A_quantiles'], out['A_quantiles'][0, 0]) < GATE)
    # the diagonal driver: the same diagonal, nothing off it; Poorman refuses
    dg = _ew(Gmat, tau, cls=mx.DiagonalMaxEnt)
    od = dg.parametric_bootstrap(n_mock=6, seed=7, quantiles=None)
    assert od['info']['n_elements'] == [2] and np.all(np.isnan(od['A_err'][0, 1])) and 'A_quantiles' not in od
    for i in range(2):
        assert rel_l2(od['A_mean'][i, i], out['A_mean'][i, i]) < GATE
        np.testing.assert_array_equal(od['alpha_index_samples'][i, i], out['alpha_index_samples'][i, i])
    pm = _ew(Gmat, tau, cls=mx.PoormanMaxEnt)
    with pytest.raises(NotImplementedError, match='default model'):
        pm.parametric_bootstrap(n_mock=6, seed=7)


def test_elementwise_complex_partners_reverse_the_quantiles():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 40, 60)
    Gc = Gmat.astype(complex)
    Gc[0, 1] = Gmat[0, 1] + 0.5j * Gmat[0, 0]
    Gc[1, 0] = np.conj(Gc[0, 1])
    ew = _ew(Gc, tau, use_complex=True)
    q = (0.1, 0.5, 0.75)                                                  # (not symmetric about 1/2)
    out = ew.parametric_bootstrap(n_mock=6, seed=7, windows=WINDOWS, keep_samples=True, quantiles=q)
    assert out['A_quantiles'].shape == (2, 2, 2, 3, 60) and out['samples']['H'].shape == (2, 2, 2, 6, 60)
    np.testing.assert_array_equal(out['quantiles'], q)
    assert out['info']['n_elements'] == [2, 2] and out['info']['audit_max'] < GATE
    delta = ew.omega.delta
    # the real part's partner is a copy, the imaginary part's has the other sign
    for k in ('A', 'A_mean', 'A_bias', 'A_quantiles', 'window_weight', 'window_quantiles'):
        np.testing.assert_array_equal(out[k][1, 0, 0], out[k][0, 1, 0])
    for k in ('A', 'A_mean', 'A_bias', 'window_weight'):
        np.testing.assert_array_equal(out[k][1, 0, 1], -out[k][0, 1, 1])
    for k in ('A_err', 'window_err', 'alpha_index_samples', 'chi2_samples'):
        np.testing.assert_array_equal(out[k][1, 0, 1], out[k][0, 1, 1])
    np.testing.assert_array_equal(out['samples']['H'][1, 0, 1], -out['samples']['H'][0, 1, 1])
    assert np.any(out['A_quantiles'][1, 0, 1] != -out['A_quantiles'][0, 1, 1])         # not a blind copy with a sign
    # ... and its quantiles are the quantiles of ITS samples: minus the partner's at 1 - q (1 - q is rounded once: a slack of
    # (n - 1) eps on the interpolation weight)
    _check_quantiles(out['A_quantiles'][0, 1, 1], out['samples']['H'][0, 1, 1], q, scale=delta)
    _check_quantiles(out['A_quantiles'][1, 0, 1], out['samples']['H'][1, 0, 1], q, scale=delta, slack=5 * EPS)
    fq = np.quantile(out['samples']['functional'][1, 0, 1], q, axis=0)
    np.testing.assert_allclose(out['window_quantiles'][1, 0, 1], fq, rtol=1e-13, atol=1e-16)
    assert np.all(np.isnan(out['A_mean'][0, 0, 1])) or np.all(out['A_mean'][0, 0, 1] == 0.0)      # no imaginary part on the diagonal


def test_elementwise_covariances_of_their_own():
    """after ``set_G_tau_bins`` every element has its own eigenbasis: the sets of the one ``mxe_mock_data`` call share the
    unrotated kernel and carry T and rank"""
    g = np.load(os.path.join(GOLD, 'bins.npz'))
    bins, tau = g['e_bins'], g['e_tau']
    ew = mx.ElementwiseMaxEnt(cov_threshold=float(g['cov_threshold']))
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    ew.set_G_tau_bins(tau, bins)
    res = ew.run()
    out = ew.parametric_bootstrap(res, n_mock=4, seed=11, keep_samples=True, keep_data=True)
    info = out['info']
    assert info['mock_calls'] == 1 and info['n_elements'] == [2, 1] and info['audit_max'] < GATE and np.all(out['n_used'] == 4)
    th = _single()                                                       # the unrotated kernel, from an object of its own
    th.set_G_tau_data(tau, bins[:, 0, 0].mean(axis=0))
    Ku = np.asarray(th.K.K)
    n = len(tau)
    assert th.K.rotation is None and Ku.shape == (n, 60)
    for (i, j) in ((0, 0), (0, 1), (1, 1)):
        st = ew.error[(i, j)][0]
        r = int(st['rank'])
        T = resampling.padded_T(st, n)
        err = np.ones(n)
        err[:r] = st['sigma']
        H0 = np.asarray(res.H)[i, j][out['alpha_index'][i, j]]
        mirror = mock.mock_rows(Ku, H0, err, 11, posterior.stream_id(2 * i + j, 0, 1, 0), 4, T=T, rank=r)
        first = np.abs(T) @ ((60 + 2) * EPS * (np.abs(Ku) @ np.abs(H0))) + 4 * n * EPS * (np.abs(T) @ np.abs(Ku @ H0))
        G = out['G_mock'][i, j][:, :r]
        assert np.all(np.isfinite(G)) and np.all(np.isnan(out['G_mock'][i, j][:, r:]))
        assert np.all(np.abs(G - mirror[:, :r]) <= first[None, :r] + err[None, :r] * 1e-13 + EPS * np.abs(mirror[:, :r])), (i, j)
        _check_quantiles(out['A_quantiles'][i, j], out['samples']['H'][i, j], Q3, scale=ew.omega.delta)
    np.testing.assert_array_equal(out['G_mock'][1, 0], out['G_mock'][0, 1])


# ---- 7. percentile intervals of the bootstrap over bins ---------------------------------------------------------------------
def test_bootstrap_of_bins_returns_percentile_intervals():
    g = np.load(os.path.join(GOLD, 'bins.npz'))
    bins, tau = g['s_bins'], g['s_tau']
    tm = _single(cov_threshold=float(g['cov_threshold']))
    tm.set_G_tau_bins(tau, bins)
    w = np.asarray(tm.omega)
    F = np.stack([w, w ** 2])
    kw = dict(method='bootstrap', n_resamples=8, seed=2, windows=WINDOWS, functionals=F, keep_samples=True)
    plain = tm.resample_errors(bins, **kw)
    bs = tm.resample_errors(bins, quantiles=Q5, **kw)
    extra = {'quantiles', 'A_quantiles', 'window_quantiles', 'functional_quantiles'}
    assert set(bs) - set(plain) == extra and not extra & set(plain) and set(plain) <= set(bs)      # the keys without: unchanged
    for k in ('A', 'A_mean', 'A_err', 'window_weight', 'window_err', 'functional_cov', 'alpha_index_samples'):
        assert np.asarray(plain[k]).tobytes() == np.asarray(bs[k]).tobytes(), k
    np.testing.assert_array_equal(bs['quantiles'], Q5)
    _check_quantiles(bs['A_quantiles'], bs['samples']['H'], Q5, scale=tm.omega.delta)
    fq = np.quantile(bs['samples']['functional'], Q5, axis=0)
    np.testing.assert_array_equal(np.concatenate([bs['window_quantiles'], bs['functional_quantiles']], axis=1), fq)
    with pytest.raises(ValueError, match='jackknife'):
        tm.resample_errors(bins, block=16, quantiles=Q3)
