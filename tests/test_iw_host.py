"""Matsubara-axis continuation, host side: IOmegaKernel, folding, the element-wise split, errors, the C-ABI entry.

The fixture tests/golden/iw_single.npz comes from the reference (tests/golden/make_golden_iw.py).
"""
import ctypes
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import kernels

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    with np.load(os.path.join(GOLD, name + '.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def g():
    return load('iw_single')


def mesh(g):
    return mx.DataOmegaMesh(g['omega'])


def test_kernel_matches_the_reference_and_the_stacked_closed_form(g):
    K = mx.IOmegaKernel(g['iomega'], mesh(g))
    n = len(g['iomega'])
    assert np.abs(K.K_complex - g['K_ref']).max() <= 1e-15 * np.abs(g['K_ref']).max()
    wn, w = g['iomega'][:, None], g['omega'][None, :]
    d = wn * wn + w * w
    assert K.K.shape == (2 * n, len(g['omega']))
    assert np.array_equal(K.K, np.concatenate([-w / d, -wn / d]))
    assert np.array_equal(K.K_delta, K.K * g['delta'][None, :])
    assert K.beta == pytest.approx(float(g['beta']), rel=1e-14)          # 2 pi / (w_1 - w_0)
    assert mx.IOmegaKernel(g['iomega'], mesh(g), beta=10.0).beta == 10.0
    assert np.array_equal(K.data_variable, g['iomega'])


def test_host_svd_reconstructs_the_stacked_kernel(g):
    K = mx.IOmegaKernel(g['iomega'], mesh(g))
    U, S, V = K.U, K.S, K.V
    Km = np.array(K.K)
    assert np.abs((U * S) @ V.T - Km).max() < 1e-13 * np.linalg.norm(Km, 2)
    K.reduce_singular_space(1e-14)
    assert len(K.S) == len(g['S'])


def test_tau_and_iomega_kernels_on_equal_grids_are_kept_apart():
    grid = np.linspace(0.1, 5.0, 20)
    omega = mx.HyperbolicOmegaMesh(-10, 10, 60)
    Kt = mx.TauKernel(grid, omega, beta=5.0)
    Ki = mx.IOmegaKernel(grid, omega)
    assert Ki.K.shape == (40, 60) and Kt.K.shape == (20, 60)
    assert not np.array_equal(Ki.K[:20], Kt.K)
    # and again, now that both fills are in the cache
    assert not np.array_equal(mx.TauKernel(grid, omega, beta=5.0).K, mx.IOmegaKernel(grid, omega).K[:20])
    assert np.array_equal(mx.IOmegaKernel(grid, omega).K, Ki.K)


def test_fold_and_unfold_round_trip(g):
    K = mx.IOmegaKernel(g['iomega'], mesh(g))
    z = g['G_iw']
    x = K.unfold(z)
    assert x.dtype == float and x.shape == (2 * len(z),)
    assert np.array_equal(K.fold(x), z)
    arr = np.stack([x, 2 * x])
    assert np.array_equal(K.fold(arr), np.stack([z, 2 * z]))
    assert np.array_equal(K.unfold(K.fold(arr)), arr)
    with pytest.raises(ValueError):
        K.fold(x[:-1])
    # the base kernel folds nothing; a PreblurKernel folds as the kernel it blurs
    Kt = mx.TauKernel(np.linspace(0, 40, 10), mesh(g))
    assert Kt.fold(x) is x and Kt.unfold(x) is x
    assert np.array_equal(mx.PreblurKernel(K=K, b=0.1).fold(x), z)


def test_preblur_of_an_iomega_kernel_on_the_host(g):
    K = mx.IOmegaKernel(g['iomega'], mesh(g))
    Kb = mx.PreblurKernel(K=K, b=0.1)
    B = mx.get_preblur(mesh(g), 0.1)
    assert np.allclose(Kb.K, np.array(K.K) @ (B * g['delta'][:, None]), rtol=0, atol=1e-15)
    assert np.abs((Kb.U * Kb.S) @ Kb.V.T - Kb.K).max() < 1e-13 * np.linalg.norm(Kb.K, 2)


def _rotated_3x3(omega):
    """a hermitian A_ij(omega) with complex off-diagonal elements: U diag(A_k) U^H with a complex unitary U"""
    w = np.asarray(omega)
    mu, s = np.array([-1.5, 0.0, 1.5]), np.array([0.4, 0.5, 0.6])
    A_diag = np.exp(-(w[None, :] - mu[:, None]) ** 2 / (2 * s[:, None] ** 2))
    A_diag /= np.trapezoid(A_diag, w, axis=1)[:, None]
    rng = np.random.RandomState(7)
    U, _ = np.linalg.qr(rng.randn(3, 3) + 1j * rng.randn(3, 3))
    return np.einsum('ik,kw,jk->ijw', U, A_diag, U.conj())


def test_elementwise_hermitian_split(g):
    omega = mesh(g)
    K = mx.IOmegaKernel(g['iomega'], omega)
    A = _rotated_3x3(omega)
    assert np.abs(A.imag).max() > 0.01
    G_iw = np.einsum('nw,ijw->ijn', K.K_complex * g['delta'][None, :], A)
    ew = mx.ElementwiseMaxEnt(use_complex=True)
    ew.set_G_iw_data(g['iomega'], G_iw)
    ew.set_error(1e-4)
    Kd = np.array(K.K_delta)
    for i in range(3):
        for j in range(3):
            for re, part in ((True, A[i, j].real), (False, A[i, j].imag)):
                worker = ew._worker_for((i, j))
                ew._load_element(worker, (i, j), re)
                assert isinstance(worker.K, mx.IOmegaKernel)
                want = Kd @ (part if (re or i != j) else A[i, j].real)
                assert np.abs(np.asarray(worker.G) - want).max() < 1e-14 * np.abs(Kd @ A[i, i].real).max()
                assert worker.err.shape == (2 * len(g['iomega']),)


def test_set_error_shapes_and_the_ndata_scale(g):
    n = len(g['iomega'])
    tm = mx.TauMaxEnt()
    tm.set_G_iw_data(g['iomega'], g['G_iw'])
    assert isinstance(tm.K, mx.IOmegaKernel) and tm.K.omega is tm.omega
    assert tm.G.shape == (2 * n,) and np.array_equal(tm.G, np.concatenate([g['G_iw'].real, g['G_iw'].imag]))
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
    assert tm.maxent_loop._alpha_scale() == 2 * n
    tm.set_cov(np.diag(e2 ** 2))
    assert np.allclose(np.sort(tm.err), np.sort(e2))
    with pytest.raises(NotImplementedError):
        tm.set_G_iw()
    # back to tau data: a TauKernel again, with the object's SVD backend and omega mesh
    tmd = mx.TauMaxEnt(svd_backend='device')
    tmd.set_G_iw_data(g['iomega'], g['G_iw'])
    assert isinstance(tmd.K, mx.IOmegaKernel) and tmd.K.svd_backend == 'device'
    tau = np.linspace(0, 40, 30)
    tmd.set_G_tau_data(tau, np.ones(30))
    assert type(tmd.K) is mx.TauKernel and tmd.K.svd_backend == 'device' and np.array_equal(tmd.tau, tau)


def test_elementwise_errors_per_frequency_are_stacked(g):
    n = len(g['iomega'])
    G = np.stack([np.stack([g['G_iw'], 0.1 * g['G_iw']]), np.stack([0.1 * g['G_iw'], g['G_iw']])])
    ew = mx.ElementwiseMaxEnt()
    ew.set_G_iw_data(g['iomega'], G)
    e = 1e-4 * np.ones(n)
    ew.set_error(e)
    assert ew.get_error((0, 1)).shape == (2 * n,)
    ew.set_error(np.ones((2, 2, n)))
    assert ew.get_error((0, 1)).shape == (2 * n,)
    with pytest.raises(NotImplementedError):
        ew.set_G_iw()


def test_library_exports_the_iomega_entry():
    from maxent_amd import device
    lib = ctypes.CDLL(device.library_path())
    assert hasattr(lib, 'mxe_kernel_svd_iw')
    assert device.load_library().mxe_kernel_svd_iw.restype is ctypes.c_int
    assert hasattr(device, 'kernel_svd_iw')
