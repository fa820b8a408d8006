"""Bosonic continuation, host side: BosonicTauKernel / BosonicIOmegaKernel against 40-digit truth, the setters, the
element-wise split, get_chi_w_from_A_w's argument handling, the C-ABI entries.

The fixtures tests/golden/boson_*.npz come from tests/golden/make_golden_boson.py (mpmath and the reference).
"""
import ctypes
import os
import pickle

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import kernels, maxent_util

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def load(name):
    with np.load(os.path.join(GOLD, name + '.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def kk():
    return load('boson_kernels')


def check_fill(got, truth, tau_abs_omega):
    """relative error <= (8 + tau |omega|) 2^-52 where the truth is above 1e-300 (the tau |omega| term: the rounding of
    the argument of exp; 8: the few roundings around it), exact 0 where the truth is below the smallest binary64
    number; nothing infinite or NaN.  Returns the largest error in units of the bound."""
    assert got.shape == truth.shape
    assert np.all(np.isfinite(got))
    big = np.abs(truth) > 1e-300
    rel = np.abs(got[big] - truth[big]) / np.abs(truth[big])
    bound = ((8 + tau_abs_omega) * EPS * np.ones(truth.shape))[big]
    worst = float((rel / bound).max()) if big.any() else 0.0
    print('fill: max rel %.2e (%.2f of the bound), %d entries, %d exact zeros'
          % (rel.max() if big.any() else 0.0, worst, big.sum(), (truth == 0).sum()))
    assert np.all(rel <= bound)
    assert np.all(got[truth == 0.0] == 0.0)
    return worst


TAU_MESHES = ['w200', 'w201z', 'wmid', 'wwide']


@pytest.mark.parametrize('name', TAU_MESHES)
def test_tau_fill_against_the_truth(kk, name):
    w = kk[name]
    K = mx.BosonicTauKernel(kk['tau'], mx.DataOmegaMesh(w), beta=float(kk['beta']))
    assert K.K.shape == (len(kk['tau']), len(w))
    check_fill(np.asarray(K.K), kk['K_tau_' + name], kk['tau'][:, None] * np.abs(w)[None, :])
    if name == 'w201z':
        assert w[100] == 0.0 and np.array_equal(K.K[:, 100], np.full(len(kk['tau']), 1.0 / float(kk['beta'])))
    if name == 'wmid':
        assert np.all(np.abs(w) < 2e-15) and np.all(w != 0)
    if name == 'w200':
        # beta omega = -400 and tau = 0, beta are in the grid
        assert w[0] == -10.0 and kk['tau'][0] == 0.0 and kk['tau'][-1] == float(kk['beta'])
    if name == 'wwide':
        assert (kk['K_tau_wwide'] == 0).any()               # (below the underflow line)
    assert np.array_equal(K.K_delta, K.K * K.omega.delta[None, :])
    assert np.array_equal(K.data_variable, kk['tau'])


def test_tau_fill_symmetric_against_the_truth(kk):
    w = kk['whalf']
    K = mx.BosonicTauKernel(kk['tau'], mx.DataOmegaMesh(w), beta=float(kk['beta']), symmetric=True)
    check_fill(np.asarray(K.K), kk['K_tau_whalf'], kk['tau'][:, None] * np.abs(w)[None, :])
    assert w[0] == 0.0 and np.array_equal(K.K[:, 0], np.full(len(kk['tau']), 2.0 / float(kk['beta'])))


def test_tau_beta_defaults_to_the_last_tau(kk):
    om = mx.DataOmegaMesh(kk['w200'])
    assert np.array_equal(mx.BosonicTauKernel(kk['tau'], om).K, mx.BosonicTauKernel(kk['tau'], om, beta=40.0).K)
    assert not np.array_equal(mx.BosonicTauKernel(kk['tau'], om, beta=41.0).K, mx.BosonicTauKernel(kk['tau'], om).K)


@pytest.mark.parametrize('name', ['w200', 'w201z', 'wmid'])
def test_matsubara_fill_is_the_stacked_closed_form_bit_for_bit(kk, name):
    w, nu = kk[name], kk['nu']
    K = mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(w))
    n = len(nu)
    assert K.K.shape == (2 * n, len(w)) and K.n_iw == n
    d = nu[:, None] * nu[:, None] + w[None, :] * w[None, :]
    with np.errstate(invalid='ignore', divide='ignore'):
        re = np.where(d > 0, (w * w)[None, :] / d, 1.0)
        im = np.where(d > 0, w[None, :] * nu[:, None] / d, 0.0)
    assert np.array_equal(K.K, np.concatenate([re, im]))
    assert np.array_equal(K.K_complex, re + 1j * im)
    assert np.array_equal(K.K[n], np.zeros(len(w)))               # the row Im K(i nu_0 = 0) is kept
    check_fill(np.asarray(K.K), kk['K_nu_' + name], 0.0)
    if name == 'w201z':
        assert K.K[0, 100] == 1.0 and K.K[n, 100] == 0.0            # omega = nu_n = 0
    assert K.beta == pytest.approx(float(kk['beta']), rel=1e-14)
    assert mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(w), beta=10.0).beta == 10.0
    assert np.array_equal(K.data_variable, nu)


def test_matsubara_fill_symmetric(kk):
    w, nu = kk['whalf'], kk['nu']
    K = mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(w), symmetric=True)
    assert K.K.shape == (len(nu), len(w)) and K.K[0, 0] == 2.0
    check_fill(np.asarray(K.K), kk['K_nu_whalf'], 0.0)
    assert np.iscomplexobj(K.K_complex) and np.array_equal(K.K_complex.real, K.K) and not K.K_complex.imag.any()


def test_fold_and_unfold_round_trip(kk):
    nu = kk['nu']
    K = mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(kk['w200']))
    rng = np.random.RandomState(1)
    z = rng.randn(len(nu)) + 1j * rng.randn(len(nu))
    x = K.unfold(z)
    assert x.dtype == float and x.shape == (2 * len(nu),)
    assert np.array_equal(K.fold(K.unfold(z)), z)
    arr = np.stack([x, 2 * x])
    assert np.array_equal(K.unfold(K.fold(arr)), arr)
    with pytest.raises(ValueError):
        K.fold(x[:-1])
    assert np.array_equal(mx.PreblurKernel(K=K, b=0.1).fold(x), z)
    Ks = mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(kk['whalf']), symmetric=True)
    y = rng.randn(len(nu))
    assert Ks.fold(y) is y and Ks.unfold(y) is y
    assert np.array_equal(Ks.unfold(y + 1j), y) and Ks.unfold(y + 1j).dtype == float


def test_symmetric_is_the_sum_of_the_two_half_axes(kk):
    w, tau, nu, beta = kk['whalf'], kk['tau'], kk['nu'], float(kk['beta'])
    for cls, grid, kw in ((mx.BosonicTauKernel, tau, dict(beta=beta)), (mx.BosonicIOmegaKernel, nu, {})):
        Kp = np.asarray(cls(grid, mx.DataOmegaMesh(w), **kw).K)
        Km = np.asarray(cls(grid, mx.DataOmegaMesh(-w[::-1]), **kw).K)[:, ::-1]
        Ks = np.asarray(cls(grid, mx.DataOmegaMesh(w), symmetric=True, **kw).K)
        two = Kp + Km
        if cls is mx.BosonicIOmegaKernel:
            n = len(nu)
            assert np.abs(two[n:]).max() <= 2 * EPS            # the imaginary parts cancel
            two = two[:n]
        assert np.all(np.abs(Ks - two) <= 2 * np.spacing(np.abs(two)))


def test_a_symmetric_kernel_on_a_two_sided_mesh_raises(kk):
    om = mx.DataOmegaMesh(kk['w200'])
    with pytest.raises(ValueError, match='omega >= 0'):
        mx.BosonicTauKernel(kk['tau'], om, symmetric=True)
    with pytest.raises(ValueError, match='omega >= 0'):
        mx.BosonicIOmegaKernel(kk['nu'], om, symmetric=True)
    tm = mx.TauMaxEnt()                                         # (its default mesh is two-sided)
    with pytest.raises(ValueError):
        tm.set_chi_tau_data(kk['tau'], np.ones(len(kk['tau'])), symmetric=True)


def test_kinds_are_kept_apart_in_the_fill_cache():
    grid = np.linspace(0.0, 5.0, 20)
    omega = mx.DataOmegaMesh(np.linspace(0.0, 10.0, 60))
    made = {}
    for rnd in range(2):                                        # (the second round finds every fill in the cache)
        now = dict(tau=mx.TauKernel(grid, omega, beta=5.0).K, iw=mx.IOmegaKernel(grid + 0.1, omega).K,
                   btau=mx.BosonicTauKernel(grid, omega, beta=5.0).K,
                   btau_s=mx.BosonicTauKernel(grid, omega, beta=5.0, symmetric=True).K,
                   biw=mx.BosonicIOmegaKernel(grid, omega).K, biw_s=mx.BosonicIOmegaKernel(grid, omega, symmetric=True).K)
        if rnd == 0:
            made = now
        else:
            for k in now:
                assert np.array_equal(now[k], made[k]), k
    assert made['btau'].shape == (20, 60) and made['biw'].shape == (40, 60) and made['biw_s'].shape == (20, 60)
    assert np.all(made['btau'] > 0) and np.all(made['tau'] < 0)
    assert not np.array_equal(made['btau'], made['btau_s'])
    assert not np.array_equal(made['biw'][:20], made['biw_s'])
    with pytest.raises(ValueError):
        made['btau'][0, 0] = 1.0                                 # shared and frozen, as TauKernel's


def test_reduce_singular_space_and_transform(kk):
    K = mx.BosonicTauKernel(kk['tau'], mx.DataOmegaMesh(kk['w200']), beta=float(kk['beta']))
    Km = np.array(K.K)
    assert np.abs((K.U * K.S) @ K.V.T - Km).max() < 1e-13 * np.linalg.norm(Km, 2)
    K.reduce_singular_space(1e-14)
    assert 30 < len(K.S) <= 64 and K.S.min() >= 1e-14
    T, _ = np.linalg.qr(np.random.RandomState(3).randn(len(kk['tau']), len(kk['tau'])))
    U0 = np.array(K.U)
    K.transform(T)
    assert np.allclose(K.K, T @ Km, rtol=0, atol=1e-15) and np.allclose(K.U, T @ U0, rtol=0, atol=1e-15)
    assert np.array_equal(K.K_delta, Km * K.omega.delta[None, :])        # never rotated
    K.transform(None)
    assert np.allclose(K.K, Km, rtol=0, atol=1e-14)


def test_preblur_of_the_bosonic_kernels_on_the_host(kk):
    om = mx.DataOmegaMesh(kk['w200'])
    B = mx.get_preblur(om, 0.1)
    for K in (mx.BosonicTauKernel(kk['tau'], om, beta=float(kk['beta'])), mx.BosonicIOmegaKernel(kk['nu'], om)):
        Kb = mx.PreblurKernel(K=K, b=0.1)
        assert np.allclose(Kb.K, np.array(K.K) @ (B * om.delta[:, None]), rtol=0, atol=1e-15)
        assert np.abs((Kb.U * Kb.S) @ Kb.V.T - Kb.K).max() < 1e-13 * np.linalg.norm(Kb.K, 2)
        assert Kb.K_delta is K.K_delta


# ---- the setters ---------------------------------------------------------------------------------------------
def test_set_chi_tau_data(kk):
    g = load('boson_tau')
    n = len(g['grid'])
    tm = mx.TauMaxEnt()
    tm.omega = mx.DataOmegaMesh(g['omega'])
    tm.set_chi_tau_data(g['grid'], g['data'], beta=float(g['beta']))
    assert type(tm.K) is mx.BosonicTauKernel and not tm.K.symmetric and tm.K.omega is tm.omega
    assert np.array_equal(tm.G, g['data']) and np.array_equal(tm.tau, g['grid'])
    assert tm.maxent_loop._alpha_scale() == n
    tm.set_error(1e-4)
    assert np.array_equal(tm.err, 1e-4 * np.ones(n))
    e = 1e-4 * (1 + np.arange(n) / n)
    tm.set_error(e)
    assert np.array_equal(tm.err, e)
    with pytest.raises(Exception):
        tm.set_error(np.ones(n + 1))
    with pytest.raises(AssertionError):
        tm.set_chi_tau_data(g['grid'], g['data'][:-1])
    with pytest.raises(AssertionError):
        tm.set_chi_tau_data(g['grid'], g['data'] + 0j)
    # the symmetric form on the half-axis mesh; the same object, a new kernel
    tm.omega = mx.DataOmegaMesh(g['omega_sym'])
    tm.set_chi_tau_data(g['grid'], g['data_sym'], beta=float(g['beta']), symmetric=True)
    assert type(tm.K) is mx.BosonicTauKernel and tm.K.symmetric and tm.K.K.shape == (n, len(g['omega_sym']))
    # back to fermionic data: a TauKernel again
    tm.set_G_tau_data(g['grid'], -g['data_sym'])
    assert type(tm.K) is mx.TauKernel


def test_set_chi_iw_data_shapes_errors_and_the_ndata_scale():
    g = load('boson_iw')
    nu, chi = g['grid'], g['chi_iw']
    n = len(nu)
    tm = mx.TauMaxEnt()
    tm.omega = mx.DataOmegaMesh(g['omega'])
    tm.set_chi_iw_data(nu, chi)
    assert type(tm.K) is mx.BosonicIOmegaKernel and tm.K.svd_backend == 'host' and tm.K.omega is tm.omega
    assert tm.G.shape == (2 * n,) and np.array_equal(tm.G, np.concatenate([chi.real, chi.imag]))
    assert np.array_equal(tm.G, g['data'])
    assert tm.maxent_loop._alpha_scale() == 2 * n
    tm.set_error(1e-4)
    assert np.array_equal(tm.err, 1e-4 * np.ones(2 * n))
    e = 1e-4 * (1 + np.arange(n) / n)
    tm.set_error(e)
    assert np.array_equal(tm.err, np.concatenate([e, e]))
    e2 = 1e-4 * (1 + np.arange(2 * n) / n)
    tm.set_error(e2)
    assert np.array_equal(tm.err, e2)
    with pytest.raises(Exception):
        tm.set_error(np.ones(n + 1))
    tm.set_cov(np.diag(e2 ** 2))
    assert np.allclose(np.sort(tm.err), np.sort(e2))
    with pytest.raises(AssertionError):
        tm.set_chi_iw_data(nu, chi[:-1])
    # symmetric: n real values
    tm.omega = mx.DataOmegaMesh(g['omega_sym'])
    tm.set_chi_iw_data(nu, g['data_sym'] + 0j, symmetric=True)
    assert tm.K.symmetric and tm.G.shape == (n,) and tm.G.dtype == float and np.array_equal(tm.G, g['data_sym'])
    assert tm.maxent_loop._alpha_scale() == n
    tm.set_error(e)
    assert np.array_equal(tm.err, e)
    with pytest.raises(Exception):
        tm.set_error(e2)
    # fermionic Matsubara data afterwards: an IOmegaKernel, not the bosonic one; the object's SVD backend is kept
    tm = mx.TauMaxEnt(svd_backend='device')
    tm.omega = mx.DataOmegaMesh(g['omega'])
    tm.set_chi_iw_data(nu, chi)
    assert type(tm.K) is mx.BosonicIOmegaKernel and tm.K.svd_backend == 'device'
    tm.set_G_iw_data(nu + np.pi / float(g['beta']), chi)
    assert type(tm.K) is mx.IOmegaKernel and tm.K.svd_backend == 'device'
    tm.set_chi_iw_data(nu, chi)
    assert type(tm.K) is mx.BosonicIOmegaKernel and tm.K.svd_backend == 'device'


def _rotated_2x2(w):
    mu, s = np.array([-1.0, 1.2]), np.array([0.4, 0.6])
    A_diag = np.exp(-(w[None, :] - mu[:, None]) ** 2 / (2 * s[:, None] ** 2))
    A_diag /= np.trapezoid(A_diag, w, axis=1)[:, None]
    U, _ = np.linalg.qr(np.random.RandomState(7).randn(2, 2) + 1j * np.random.RandomState(8).randn(2, 2))
    return np.einsum('ik,kw,jk->ijw', U, A_diag, U.conj())


def test_elementwise_hermitian_split(kk):
    w, nu = kk['w200'], kk['nu']
    omega = mx.DataOmegaMesh(w)
    K = mx.BosonicIOmegaKernel(nu, omega)
    A = _rotated_2x2(w)
    assert np.abs(A.imag).max() > 0.01
    Kd = np.array(K.K_delta)
    chi = np.einsum('nw,ijw->ijn', K.K_complex * omega.delta[None, :], A)
    ew = mx.ElementwiseMaxEnt(use_complex=True)
    ew.omega = omega
    ew.set_chi_iw_data(nu, chi)
    ew.set_error(1e-4 * np.ones(len(nu)))
    assert ew.shape == (2, 2)
    for i in range(2):
        for j in range(2):
            for re, part in ((True, A[i, j].real), (False, A[i, j].imag)):
                worker = ew._worker_for((i, j))
                ew._load_element(worker, (i, j), re)
                assert type(worker.K) is mx.BosonicIOmegaKernel
                want = Kd @ (part if (re or i != j) else A[i, j].real)
                assert np.abs(np.asarray(worker.G) - want).max() < 1e-14 * np.abs(Kd @ A[i, i].real).max()
                assert worker.err.shape == (2 * len(nu),)
    with pytest.raises(AssertionError):
        ew.set_chi_iw_data(nu, chi[:, :, :-1])
    # chi(tau): the real part of an element, as for G(tau)
    tau = kk['tau']
    Kt = mx.BosonicTauKernel(tau, omega, beta=float(kk['beta']))
    chi_tau = np.einsum('tw,ijw->ijt', np.array(Kt.K_delta), A.real)
    ew = mx.ElementwiseMaxEnt()
    ew.omega = omega
    ew.set_chi_tau_data(tau, chi_tau, beta=float(kk['beta']))
    ew.set_error(1e-4)
    worker = ew._worker_for((0, 1))
    ew._load_element(worker, (0, 1), True)
    assert type(worker.K) is mx.BosonicTauKernel and np.array_equal(worker.G, chi_tau[0, 1])
    assert ew.get_error((0, 1)) == 1e-4
    with pytest.raises(AssertionError):
        ew.set_chi_tau_data(tau, chi_tau[:, :, :-1])


def test_result_record_folds_and_pickles():
    """the data-space fields of a result in the form the data came in (complex for the stacked kernel, real
    otherwise), through pickle"""
    from maxent_amd import maxent_loop
    g = load('boson_iw')
    nu = g['grid']
    K = mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(g['omega']))
    A = g['A_truth'][:3]
    rec = maxent_loop.data_fields(K, g['data'], g['data'], A)
    assert rec['G'].dtype == complex and np.array_equal(rec['G'], g['chi_iw']) and np.array_equal(rec['G_orig'], g['chi_iw'])
    G_rec = np.asarray(rec['G_rec'])
    assert G_rec.dtype == complex and G_rec.shape == (3, len(nu))
    np.testing.assert_allclose(G_rec, A @ (K.K_complex * g['delta'][None, :]).T, rtol=0, atol=1e-13)
    back = pickle.loads(pickle.dumps(dict(G=rec['G'], G_rec=G_rec)))
    assert back['G'].dtype == complex and np.array_equal(back['G_rec'], G_rec)
    Ks = mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(g['omega_sym']), symmetric=True)
    rec = maxent_loop.data_fields(Ks, g['data_sym'], g['data_sym'], g['A_truth_sym'][:3])
    assert rec['G'].dtype == float and np.asarray(rec['G_rec']).dtype == float
    # the kernels themselves pickle (a result's plain-data form carries none, a user's script may)
    K2 = pickle.loads(pickle.dumps(K))
    assert np.array_equal(K2.K, K.K) and K2.symmetric is False


# ---- chi(omega) ------------------------------------------------------------------------------------------------
def test_get_chi_w_argument_checks_and_the_mirror():
    w = np.linspace(0.0, 5.0, 11)
    A = np.arange(11.0)
    Am, wm = maxent_util._mirror_half_axis(A, w)
    assert np.array_equal(wm, np.linspace(-5.0, 5.0, 21)) and np.array_equal(Am, np.abs(np.arange(-10.0, 11.0)))
    Am, wm = maxent_util._mirror_half_axis(A, w + 0.25)                    # no point at 0: every point is mirrored
    assert len(wm) == 22 and np.array_equal(wm, -wm[::-1]) and np.array_equal(Am, Am[::-1])
    Am3, _ = maxent_util._mirror_half_axis(np.stack([A, 2 * A]).reshape(1, 2, 11)[:, :1].repeat(1, 0), w)
    assert Am3.shape == (1, 1, 21)
    with pytest.raises(Exception, match='>= 0'):
        mx.get_chi_w_from_A_w(A, np.linspace(-1, 5, 11), symmetric=True)
    with pytest.raises(Exception, match='wrong shape'):
        mx.get_chi_w_from_A_w(np.ones((2, 3, 11)), w)
    with pytest.raises(Exception, match='w_min'):
        mx.get_chi_w_from_A_w(A, w, w_min=1, w_max=0)
    assert 'get_chi_w_from_A_w' in maxent_util.__all__


# ---- the library -------------------------------------------------------------------------------------------------
def test_library_exports_the_three_entries_and_the_header_declares_them():
    from maxent_amd import device
    lib = ctypes.CDLL(device.library_path())
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    for name in ('mxe_kernel_svd_boson', 'mxe_kernel_svd_boson_iw', 'mxe_kernel_svd_data'):
        assert hasattr(lib, name)
        assert getattr(device.load_library(), name).restype is ctypes.c_int
        assert ('int  %s(int device,' % name) in header
    for name in ('kernel_svd_boson', 'kernel_svd_boson_iw', 'kernel_svd_data'):
        assert hasattr(device, name)
    assert mx.DataKernel(np.arange(3.0), mx.DataOmegaMesh(np.linspace(0, 1, 4)), np.ones((3, 4)),
                         svd_backend='device').svd_backend == 'device'
