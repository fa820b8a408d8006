"""Legendre-basis continuation on the GPU: the device fill (mxe_kernel_svd_legendre) against 40-digit truth, its
decomposition, TauMaxEnt / ElementwiseMaxEnt on Legendre coefficients G_l against the extended-precision fixed point of
the reference's iterates (tests/golden/make_golden_legendre.py), bins, error bars and the preblur scan.

Gate as everywhere (test_gpu_api.py, test_gpu_boson.py): 1e-6 relative L2 against the truth (oracle/hp_truth.py).
"""
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GATE = 1e-6
EPS = 2.0 ** -52
SVD_MAX_SWEEPS = 40
GRIDS = ['w200', 'w201z', 'wmid', 'wwide', 'wsmall', 'even', 'shuffled', 'l0']


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def load(name):
    with np.load(os.path.join(GOLD, name + '.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def kk():
    return load('legendre_kernels')


@pytest.fixture(scope='module')
def c(kk):
    """the single-scan fixture with its (40-digit) kernel"""
    g = load('legendre')
    g['K'] = kk['K_w200']
    return g


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _delta(w):
    return mx.DataOmegaMesh(w).delta


# ---- the device fill --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GRIDS)
def test_device_fill_against_the_truth(kk, name):
    """the bound of tests/test_legendre_host.py: relative error <= (8 + l) 2^-52 where |truth| >= 2^-1000, |K| < 2^-990
    elsewhere, exact values at omega = 0; one row (l0), 2, 81 and 201 columns: grids that are no multiple of the block"""
    l, w, truth = kk['l_' + name], kk['w_' + name], kk['K_' + name]
    got = device.kernel_svd_legendre(l, w, _delta(w), float(kk['beta']), want_K=True)[0]['K']
    assert got.shape == truth.shape and np.all(np.isfinite(got))
    big = np.abs(truth) >= 2.0 ** -1000
    bound = (8.0 + l)[:, None] * EPS * np.abs(truth)
    err = np.abs(got - truth)
    host = np.asarray(mx.LegendreKernel(l, mx.DataOmegaMesh(w), beta=float(kk['beta'])).K)
    print('device fill %s: worst error %.3f of the bound; %d of %d entries differ from the host fill'
          % (name, (err[big] / bound[big]).max(), int((got != host).sum()), got.size))
    assert np.all(err[big] <= bound[big])
    assert np.all(np.abs(got[~big]) < 2.0 ** -990)
    zero = w == 0.0
    if zero.any():
        assert np.all(got[l == 0][:, zero] == -float(kk['beta']) / 2) and np.all(got[l != 0][:, zero] == 0.0)


def test_refused_arguments_raise_before_any_launch(kk):
    """the refusals are on the host side of the C-ABI: nothing is launched"""
    w = kk['w_w200']
    for l, beta in (([0, -1, 2], 40.0), ([0, 0.5, 2], 40.0), ([0, 1, 2], 0.0), ([0, 1, 5000], 40.0), ([0, 1, 2], -1.0),
                    ([0, 1, 1], 40.0), ([0, 1, 2], 1e7)):
        with pytest.raises(device.MaxEntDeviceError, match='mxe_kernel_svd_legendre'):
            device.kernel_svd_legendre(l, w, _delta(w), beta)


# ---- the decomposition ------------------------------------------------------------------------------------------
def check_svd(r, Kh, what):
    """the assertions and constants of test_gpu_boson.py::check_svd, and: every singular value above 1e-14 within
    1e-12 S_0 of numpy's"""
    nrm = np.linalg.norm(Kh, 2)
    Sl = np.linalg.svd(Kh, compute_uv=False)
    U, S, V = r['U'], r['S'], r['V']
    k = int((Sl >= 1e-12 * Sl[0]).sum())
    lead = int((Sl >= 1e-4 * Sl[0]).sum())
    k14 = min(int((Sl >= 1e-14).sum()), len(S))
    d_abs = np.max(np.abs(S[:k] - Sl[:k])) / Sl[0]
    d_rel = np.max(np.abs(S[:lead] - Sl[:lead]) / Sl[:lead])
    print('%s: n_s=%d (LAPACK %d above 1e-14) qr_rank=%d sweeps=%d %.3f ms; |dS|/S_0 %.1e, leading %d values relative %.1e'
          % (what, len(S), int((Sl >= 1e-14).sum()), r['qr_rank'], r['sweeps'], r['ms'], d_abs, lead, d_rel))
    assert 0 < r['sweeps'] < SVD_MAX_SWEEPS
    assert abs(len(S) - int((Sl >= 1e-14).sum())) <= 1             # (a value may lie within rounding of the cut)
    assert np.max(np.abs(S[:k14] - Sl[:k14])) <= 1e-12 * Sl[0]
    assert len(S) >= k and d_abs < 1e-12 and d_rel < 1e-12
    assert np.abs((U * S) @ V.T - Kh).max() < 1e-13 * nrm
    assert np.abs(U.T @ U - np.eye(len(S))).max() < 1e-12
    assert np.abs(V.T @ V - np.eye(len(S))).max() < 1e-12


def test_device_svd_of_the_kernel_and_of_the_same_matrix_as_a_callers(kk):
    l, w, Kt = kk['l_w200'], kk['w_w200'], kk['K_w200']
    omega = mx.DataOmegaMesh(w)
    bs = [0.0, 0.1]
    K = mx.LegendreKernel(l, omega, beta=float(kk['beta']))
    res = device.kernel_svd_legendre(l, w, omega.delta, float(kk['beta']), bs, want_K=True)
    res_d = device.kernel_svd_data(Kt, w, omega.delta, bs, want_K=True)
    for b, r, rd in zip(bs, res, res_d):
        Kh = np.array(K.K) if b <= 0 else np.array(mx.PreblurKernel(K=K, b=b).K)
        if b > 0:
            assert np.abs(r['K'] - Kh).max() <= 1e-14 * np.linalg.norm(Kh, 2)
        check_svd(r, np.array(r['K']) if b <= 0 else Kh, 'fill + SVD b=%g' % b)
        Kd = Kt if b <= 0 else np.array(mx.PreblurKernel(K=mx.DataKernel(None, omega, Kt), b=b).K)
        assert np.abs(rd['K'] - Kd).max() <= 1e-14 * np.linalg.norm(Kd, 2)
        check_svd(rd, Kd, 'mxe_kernel_svd_data b=%g' % b)


def test_preblur_scan_of_the_legendre_kernel(kk):
    omega = mx.DataOmegaMesh(kk['w_w200'])
    beta = float(kk['beta'])
    K = mx.LegendreKernel(kk['l_w200'], omega, beta=beta, svd_backend='device')
    widths = [0.05, 0.2]
    scan = mx.PreblurKernel.scan(K, widths)
    for Kb, b in zip(scan, widths):
        assert Kb.b == b and Kb.S.min() >= 1e-14
        one = mx.PreblurKernel(K=mx.LegendreKernel(kk['l_w200'], omega, beta=beta, svd_backend='device'), b=b)
        Kh = np.array(mx.PreblurKernel(K=mx.LegendreKernel(kk['l_w200'], omega, beta=beta), b=b).K)
        nrm = np.linalg.norm(Kh, 2)
        assert np.abs((Kb.U * Kb.S) @ Kb.V.T - Kh).max() < 1e-12 * nrm
        assert np.abs((one.U * one.S) @ one.V.T - Kh).max() < 1e-12 * nrm
        k = len(Kb.S)
        np.testing.assert_allclose(one.S[:k], Kb.S, rtol=0, atol=1e-12 * Kb.S[0])


# ---- single scan ------------------------------------------------------------------------------------------------
def facade(c, svd_backend='host'):
    tm = mx.TauMaxEnt(svd_backend=svd_backend)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.DataOmegaMesh(c['omega'])
    tm.set_G_l_data(c['data'], float(c['beta']), l=c['l'])
    tm.set_error(float(c['err'][0]))
    tm.alpha_mesh = mx.DataAlphaMesh(c['alpha'] / len(c['err']))
    return tm


@pytest.fixture(scope='module')
def facade_run(c):
    tm = facade(c)
    return tm, tm.run()


def test_single_scan_matches_the_reference_fixed_point(c, facade_run):
    assert np.all(c['converged_ref']) and len(c['converged_ref']) == len(c['alpha']) == 30
    tm, res = facade_run
    assert type(tm.K) is mx.LegendreKernel
    assert abs(len(tm.K.S) - len(c['S'])) <= 1
    assert np.all(res.converged)
    np.testing.assert_allclose(np.asarray(res.alpha), c['alpha'], rtol=1e-14)
    eA, eH = rel_l2(np.asarray(res.A), c['A_truth']).max(), rel_l2(np.asarray(res.H), c['H_truth']).max()
    print('legendre: A %.2e H %.2e audit %.2e' % (eA, eH, tm.last_launch['audit_max']))
    assert eA < GATE and eH < GATE
    assert tm.last_launch['audit_max'] < GATE, tm.last_launch['audit_max']
    assert np.array_equal(res.data_variable, c['l'])
    G_rec = np.asarray(res.G_rec)
    assert np.asarray(res.G).dtype == float and np.array_equal(res.G, c['data']) and G_rec.shape == (30, 30)
    assert res.analyzer_results['LineFitAnalyzer']['alpha_index'] == int(c['linefit_alpha_index'])


def test_maxent_loop_with_a_data_kernel_of_the_truth_equals_the_facade(c, facade_run):
    """the way a user had to do it before: MaxEntLoop + DataKernel of the (40-digit) matrix"""
    omega = mx.DataOmegaMesh(c['omega'])
    loop = mx.MaxEntLoop(alpha_mesh=mx.DataAlphaMesh(c['alpha'] / len(c['err'])))
    loop.set_verbosity(mx.VerbosityFlags.Quiet)
    loop.K = mx.DataKernel(c['l'], omega, c['K'])
    loop.D = mx.FlatDefaultModel(omega)
    loop.G = c['data']
    loop.err = c['err']
    res = loop.run()
    ref = facade_run[1]
    assert np.all(res.converged) and np.all(ref.converged)
    e = rel_l2(np.asarray(res.H), np.asarray(ref.H)).max()
    print('hand-built vs facade %.2e' % e)
    assert e < GATE
    assert rel_l2(np.asarray(res.H), c['H_truth']).max() < GATE


def test_device_backend_end_to_end(c):
    tm = facade(c, svd_backend='device')
    out = tm.run()
    assert tm.K.svd_backend == 'device' and np.all(out.converged)
    e = rel_l2(np.asarray(out.A), c['A_truth']).max()
    print('device backend: %.2e' % e)
    assert e < GATE and tm.last_launch['audit_max'] < GATE
    Kb = mx.PreblurKernel(K=mx.LegendreKernel(c['l'], tm.omega, beta=float(c['beta']), svd_backend='device'), b=0.1)
    assert Kb.svd_backend == 'device'
    assert np.abs((Kb.U * Kb.S) @ Kb.V.T - Kb.K).max() < 1e-13 * np.linalg.norm(Kb.K, 2)


# ---- element-wise -----------------------------------------------------------------------------------------------
def _ew(g, G_l, herm=True):
    ew = mx.ElementwiseMaxEnt(use_hermiticity=herm)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.DataOmegaMesh(g['omega'])
    ew.alpha_mesh = mx.DataAlphaMesh(g['alpha_mesh'])
    ew.set_G_l_data(G_l, float(g['beta']), l=g['l'])
    ew.set_error(float(g['err']))
    return ew


def test_elementwise_fixture_and_run_many_returns_the_same_bits():
    g = load('legendre_elementwise')
    ew = _ew(g, g['G_l'])
    res = ew.run()
    assert type(ew.maxent_diagonal.K) is mx.LegendreKernel and type(ew.maxent_offdiagonal.K) is mx.LegendreKernel
    assert np.array_equal(ew.maxent_diagonal.K.V, ew.maxent_offdiagonal.K.V)      # one decomposition for all elements
    assert all(info['audit_max'] < GATE for info in ew.last_launches) and ew.last_launches
    H = np.asarray(res.H)
    assert H.shape == g['H_truth'].shape
    for i in range(2):
        for j in range(2):
            e = rel_l2(H[i, j], g['H_truth'][i, j])
            print('element-wise (%d, %d): %.2e' % (i, j, e.max()))
            assert np.all(np.isfinite(e)) and e.max() < GATE, (i, j, e.max())
    jobs = [_ew(g, g['G_l']), _ew(g, 0.5 * g['G_l'])]
    seq = [np.asarray(job.run().H).copy() for job in jobs]
    many = mx.run_many(jobs)
    for s, r in zip(seq, many):
        assert np.array_equal(np.asarray(r.H), s, equal_nan=True)
    assert np.array_equal(seq[0], H, equal_nan=True)


# ---- bins and error bars ----------------------------------------------------------------------------------------
def cov_longdouble(bins):
    b = np.asarray(bins, dtype=np.longdouble)
    nb = b.shape[0]
    X = (b - b.mean(axis=0)) / np.sqrt(np.longdouble(nb) * (nb - 1))
    return np.asarray(X.T @ X, dtype=float), np.asarray(b.mean(axis=0), dtype=float)


def _single(b, **kw):
    tm = mx.TauMaxEnt(**kw)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.DataOmegaMesh(b['omega'])
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    return tm


def test_bins_equal_the_host_path_and_carry_error_bars():
    """set_G_l_bins is set_G_l_data(mean) + set_cov(C) on a fresh object (the comparison of
    test_gpu_bins.py::test_single_element_bins_match_truth_reference_and_host_path); 24 bins of 30 coefficients: the
    covariance of the mean has 23 directions"""
    b = load('legendre_bins')
    beta = float(b['beta'])
    tm = _single(b)
    tm.set_G_l_bins(b['s_bins'], beta)
    st = tm.bin_statistics
    assert type(tm.K) is mx.LegendreKernel and np.array_equal(tm.tau, b['s_l'])
    assert st['rank'] == 23 and st['n_bins'] == 24 and len(tm.err) == 23
    C, mean = cov_longdouble(b['s_bins'])
    np.testing.assert_allclose(st['mean'], mean, rtol=0, atol=2 * EPS * np.abs(b['s_bins']).max())
    res = tm.run()
    assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE
    th = _single(b)
    th.set_G_l_data(mean, beta)
    th.set_cov(C)
    rh = th.run()
    assert len(th.err) == 23
    eh = rel_l2(np.asarray(res.H), np.asarray(rh.H))
    print('bins path vs host path: %.2e' % eh.max())
    assert eh.max() < GATE
    np.testing.assert_allclose(res.G_orig, st['mean'], rtol=0, atol=0)
    jk = tm.resample_errors(b['s_bins'], method='jackknife')
    assert jk['n_used'] == 24 and jk['A_err'].shape == (200,) and np.all(np.isfinite(jk['A_err'])) and np.any(jk['A_err'] > 0)
    pe = tm.posterior_errors(res, windows=[(-1, 1)])
    print('window weight %.4f +- %.2e (prior %.2e)' % (pe['window_weight'][0], pe['window_err'][0], pe['prior_err'][0]))
    assert np.isfinite(pe['window_err'][0]) and 0 < pe['window_err'][0] < pe['prior_err'][0]


def test_elementwise_bins_equal_the_host_path():
    b = load('legendre_bins')
    beta = float(b['beta'])
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.DataOmegaMesh(b['omega'])
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    ew.set_G_l_bins(b['e_bins'], beta, l=b['e_l'])
    assert sorted(ew.bin_statistics) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert all(st['rank'] == 11 and st['n_bins'] == 12 for st in ew.bin_statistics.values())
    res = ew.run()
    assert all(info['audit_max'] < GATE for info in ew.last_launches) and ew.last_launches
    for i in range(2):
        for j in range(2):
            C, mean = cov_longdouble(b['e_bins'][:, i, j, :])
            th = mx.TauMaxEnt(**({} if i == j else dict(cost_function='plusminus')))
            th.set_verbosity(mx.VerbosityFlags.Quiet)
            th.omega = mx.DataOmegaMesh(b['omega'])
            th.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
            th.set_G_l_data(mean, beta, l=b['e_l'])
            th.set_cov(C)
            rh = th.run()
            assert len(th.err) == 11
            e = rel_l2(np.asarray(res.H[i, j]), np.asarray(rh.H)).max()
            print('element-wise bins (%d, %d) vs host path: %.2e' % (i, j, e))
            assert e < GATE, (i, j)
    jk = ew.resample_errors(b['e_bins'], method='jackknife')
    assert np.all(jk['n_used'] == 12) and np.all(np.isfinite(jk['A_err']))
