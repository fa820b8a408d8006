"""The device code every ordinary run goes through -- tau_kernel_fill, iomega_kernel_fill, the preblur chain
(preblur_rows, preblur_cols, preblur_matrix, preblur_product) and output_map_kernel -- against truth that shares no
formula with the host path: tests/golden/fermion_kernels.npz (mpmath at 40 digits on the stored grid values,
tests/golden/make_golden_fermion_kernels.py) and np.longdouble restatements held against that fixture.

tests/test_fermion_fill_host.py shows that the plain numpy path meets the same bounds and has their derivations.
EPS = 2^-52.  Every entry is checked: relative error where |truth| > 1e-300, |got| < 1e-290 elsewhere; the gates of
the products are absolute, term by term.  Every test prints its worst ratio to its bound (pytest -s).

  a. tau fill         (8 + x) EPS, x = tau |w| (w >= 0), (beta - tau) |w| (w < 0); -0.5 exactly at w = 0; the one-point
                      tau grid; device against host on 200 x 500 within 2 ulp of the entry
  b. Matsubara fill   the host fill bit for bit, 8 EPS of the truth
  c. blur matrix      K = unit rows e_i: K'[r][l] = fl(delta_i B[i][l]), against delta_i times truth,
                      (17 + n_omega/16 + 4 y) EPS, y = (w_l - w_i)^2 / (2 b^2); n_omega = 2, 3, 255, 257, 513 are a short
                      block, one under and one over the 256 threads of the reductions of preblur_rows / preblur_cols, and
                      two strides plus one; the hyperbolic meshes are where B is not symmetric
  d. blur product     K (300 rows: the strided loop of preblur_product; 1 row) times diag(delta) B, against longdouble,
                      |K' - truth|[i][l] <= sum_j |K_ij| delta_j B_jl ((n_omega/2 + 3) EPS + bound of (c) at (j, l)):
                      two interleaved fma chains of n_omega/2 terms on top of B's own error; odd n_omega takes the tail
  e. output map       a random signed non-symmetric matrix: (n_omega/2 + 2) EPS sum_k |B_jk H_k|; the blur matrix of the
                      mesh against PreblurA_of_H on the host, 1e-13 relative L2
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fermion_fill_host import (EPS, PB_MESHES, load, check_entries, tau_bound, blur_bound, blur_truth,   # noqa: E402
                                    blur_longdouble, check_blur_longdouble)
import maxent_amd as mx                                                                                       # noqa: E402
from maxent_amd import device, synthetic, hostprep                                                            # noqa: E402
from maxent_amd.preblur import get_preblur                                                                    # noqa: E402

pytestmark = pytest.mark.gpu

L = np.longdouble


@pytest.fixture(scope='module')
def fk():
    return load()


def _delta(w):
    return mx.DataOmegaMesh(w).delta


# ---- a. the fermionic tau fill --------------------------------------------------------------------------------------
@pytest.mark.parametrize('tname', ['tau', 'tau_one'])
@pytest.mark.parametrize('wname', ['hyp67', 'wide41', 'zero'])
def test_device_tau_fill_against_the_truth(fk, wname, tname):
    tau, w, beta = fk[tname], fk['w_' + wname], float(fk['beta'])
    r = device.kernel_svd(tau, w, _delta(w), beta, [0.0], want_K=True)[0]
    check_entries(r['K'], fk['K_%s_%s' % (tname, wname)], tau_bound(tau, w, beta),
                  'device tau fill %s x %s' % (tname, wname))
    if wname == 'zero':
        assert w[1] == 0.0 and np.all(r['K'][:, 1] == -0.5)


def test_device_tau_fill_is_within_two_ulp_of_the_host_fill():
    tau, omega = synthetic.grids(200, 500)
    w = np.asarray(omega)
    Kd = device.kernel_svd(tau, w, omega.delta, synthetic.BETA, [0.0], want_K=True)[0]['K']
    Kh = np.asarray(mx.TauKernel(tau, omega, beta=synthetic.BETA).K)
    ulps = np.abs(Kd - Kh) / np.spacing(np.abs(Kh))
    print('device against host tau fill 200 x 500: %d of %d entries differ, worst %.1f ulp (%.2f of the bound 2)'
          % ((ulps > 0).sum(), ulps.size, ulps.max(), ulps.max() / 2))
    assert np.all(np.isfinite(Kd)) and ulps.max() <= 2.0


# ---- b. the Matsubara fill ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wname', ['hyp67', 'zero'])
def test_device_matsubara_fill_is_the_host_fill_and_the_truth(fk, wname):
    iw, w = fk['iw'], fk['w_' + wname]
    r = device.kernel_svd_iw(iw, w, _delta(w), [0.0], want_K=True)[0]
    truth = fk['K_iw_' + wname]
    check_entries(r['K'], truth, 8 * EPS, 'device Matsubara fill ' + wname)
    assert np.all(r['K'][truth == 0.0] == 0.0)
    assert np.array_equal(r['K'], np.asarray(mx.IOmegaKernel(iw, mx.DataOmegaMesh(w)).K))


# ---- c. the blur matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PB_MESHES)
def test_device_blur_matrix_against_the_truth(fk, name):
    w, delta = fk['pb_w_' + name], fk['pb_delta_' + name]
    n = len(w)
    rows = fk['pb_rows_%d' % n]
    K = np.zeros((len(rows), n))
    K[np.arange(len(rows)), rows] = 1.0
    res = device.kernel_svd_data(K, w, delta, fk['pb_b'], want_K=True)
    for ib, b in enumerate(fk['pb_b']):
        truth = delta[rows].astype(L)[:, None] * blur_truth(fk, name, ib)
        check_entries(res[ib]['K'], truth, blur_bound(w, rows, float(b)), 'device blur matrix %s b=%g' % (name, b))


# ---- d. the blur product --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blur_L(name, ib):
    """the longdouble blur matrix on a fixture mesh, checked against the fixture's rows before it serves as truth"""
    fk = load()
    B = blur_longdouble(fk['pb_w_' + name], fk['pb_delta_' + name], float(fk['pb_b'][ib]))
    check_blur_longdouble(fk, name, ib, B)
    B.setflags(write=False)
    return B


@pytest.mark.parametrize('ib', [1, 2])                       # b = 0.05, 0.3
@pytest.mark.parametrize('n', [3, 255, 257])
def test_device_blur_product_against_longdouble(fk, n, ib):
    name = 'hyp%d' % n
    w, delta, b = fk['pb_w_' + name], fk['pb_delta_' + name], float(fk['pb_b'][ib])
    B = _blur_L(name, ib)
    dB = delta.astype(L)[:, None] * B                                        # delta_j B_jl
    term_bound = np.asarray(dB, dtype=float) * ((n / 2.0 + 3) * EPS + blur_bound(w, np.arange(n), b))
    rng = np.random.RandomState(4000 + 10 * n + ib)
    R1, R2 = rng.randn(300, 8), rng.randn(8, n)
    one = (0.1 + rng.rand(1, n)) * (-1.0) ** np.arange(n)                       # (signed whatever the seed gives)
    for what, K in (('300 rows', R1 @ R2), ('1 row', one)):
        assert (K < 0).any() and (K > 0).any()
        got = device.kernel_svd_data(K, w, delta, [b], want_K=True)[0]['K']
        assert got.shape == K.shape and np.all(np.isfinite(got))
        err = np.asarray(np.abs(got.astype(L) - K.astype(L) @ dB), dtype=float)
        gate = np.abs(K) @ term_bound
        print('device blur product %s b=%g, %s: worst ratio to the bound %.3f' % (name, b, what, (err / gate).max()))
        assert np.all(gate > 0) and np.all(err <= gate)


# ---- e. the output map ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _launched(n_tau, n_omega):
    """a small launched context -- two chains (normal, plus-minus) at three alphas on a problem of test_gpu_shapes.py --
    and what it gives for a random matrix and for the blur matrix of its mesh"""
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, n_tau, n_omega)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    alphas = np.array(synthetic.alpha_mesh(3)) * n_tau
    kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
    v0 = np.stack([hostprep.initial_v(K.V, D, omega.delta, k) for k in kinds])
    B_rand = np.random.RandomState(500 + n_omega).randn(n_omega, n_omega)
    B_blur = get_preblur(omega, 0.3)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    try:
        ds = ctx.add_dataset(synthetic.SIGMA * np.ones(n_tau))
        ctx.set_elements([ds] * 2, [Gmat[0, 0], Gmat[0, 1]], np.tile(D, (2, 1)), kinds)
        H = ctx.solve_chains(np.arange(2), alphas, v0)['H']
        return omega, H, B_rand, ctx.apply_output_map(B_rand), B_blur, ctx.apply_output_map(B_blur)
    finally:
        ctx.close()


@pytest.mark.parametrize('n_tau,n_omega', [(40, 33), (80, 257)])
def test_output_map_of_a_matrix_that_is_not_symmetric(n_tau, n_omega):
    omega, H, B, A, _, _ = _launched(n_tau, n_omega)
    assert H.shape == A.shape == (2, 3, n_omega) and np.all(np.isfinite(H)) and np.all(np.isfinite(A))
    assert (H < 0).any() and (B < 0).any() and not np.allclose(B, B.T)
    truth = H.astype(L) @ B.astype(L).T                                      # A_j = sum_k B_jk H_k
    gate = (n_omega / 2.0 + 2) * EPS * (np.abs(H) @ np.abs(B).T)
    err = np.asarray(np.abs(A.astype(L) - truth), dtype=float)
    print('output map n_omega=%d: worst ratio to the bound %.3f' % (n_omega, (err / gate).max()))
    assert np.all(err <= gate)
    # the transposed matrix gives something else: the gate tells B from B^T
    wrong = np.asarray(np.abs(H.astype(L) @ B.astype(L) - truth), dtype=float)
    assert np.all(wrong.max(axis=-1) > 1e6 * gate.max(axis=-1))


@pytest.mark.parametrize('n_tau,n_omega', [(40, 33), (80, 257)])
def test_output_map_of_the_blur_matrix_is_preblur_a_of_h(n_tau, n_omega):
    omega, H, _, _, B, A = _launched(n_tau, n_omega)
    assert np.abs(B - B.T).max() > 1e-3 * np.abs(B).max()                     # (the hyperbolic mesh: not symmetric)
    f = mx.PreblurA_of_H(b=0.3, omega=omega)
    assert np.array_equal(f.matrix(), B)
    want = np.stack([[f.f(h) for h in Hc] for Hc in H])
    rel = np.linalg.norm(A - want, axis=-1) / np.linalg.norm(want, axis=-1)
    print('output map of the blur matrix n_omega=%d: worst rel L2 %.2e (%.3f of the bound 1e-13)'
          % (n_omega, rel.max(), rel.max() / 1e-13))
    assert np.all(rel <= 1e-13)
