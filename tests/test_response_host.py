"""Host side of the linear response: the extended-precision truth the GPU tests compare against (``response_ref``), pinned
against a 50-digit solve, against its own identities and against finite differences of the re-solved fit; the summaries
and argument checks of ``maxent_amd.response``; the binary64 prototype of the kernel's formula on the GPU tests' shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_posterior_errors_host import LD, small_problem                            # noqa: E402
from test_fit_diagnostics_host import truth_hat                                      # noqa: E402
from response_ref import GATE, truth_response, weights, prototype, rhs_rows, worst_rel    # noqa: E402
import maxent_amd as mx                                                              # noqa: E402
from maxent_amd import response, synthetic, hostprep, device, kernels               # noqa: E402
from oracle import sform as SF                                                       # noqa: E402

# the steps of the finite-difference tests (see their docstrings): the largest whitened data perturbation of (a), the
# factor on the direction of ln D of (b)
FD_STEP_DATA = 1e-2
FD_STEP_MODEL = 1e-3
# the error of the difference quotient of (b) the truth showed at FD_STEP_MODEL (measured, see the test's docstring): the GPU
# test of default_model_response against two run() calls gates at 10 x these
FD_MODEL_ERROR = {'normal': 1.22e-9, 'plusminus': 1.85e-7}


def test_longdouble_truth_against_50_digit_solve():
    import mpmath as mp
    mp.mp.dps = 50
    omega, K, H, err = small_problem()
    n_tau, n = K.shape
    for alpha in (2.0, 2.0e3):
        R, Dm = truth_response(K, err, H, alpha)
        Km = mp.matrix(K.tolist())
        sig = [mp.mpf(float(e)) for e in err]
        M = mp.zeros(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.fsum(Km[t, i] * Km[t, j] / sig[t] ** 2 for t in range(n_tau))
        hess = M.copy()
        for i in range(n):
            hess[i, i] += mp.mpf(alpha) / mp.mpf(float(H[i]))
        inv = mp.inverse(hess)
        Rm = inv * M
        Kw = mp.matrix(n, n_tau)
        for i in range(n):
            for t in range(n_tau):
                Kw[i, t] = Km[t, i] / sig[t]
        Dmm = inv * Kw
        top_R = max(abs(Rm[i, j]) for i in range(n) for j in range(n))
        top_D = max(abs(Dmm[i, t]) for i in range(n) for t in range(n_tau))
        for i in range(n):
            for j in range(n):
                assert abs(mp.mpf(float(R[i, j])) - Rm[i, j]) < 1e-12 * top_R, (alpha, i, j)
            for t in range(n_tau):
                assert abs(mp.mpf(float(Dm[i, t])) - Dmm[i, t]) < 1e-12 * top_D, (alpha, i, t)


def test_identities_of_the_truth():
    omega, K, H, err = small_problem()
    G = K @ H
    f = np.cos(omega) * H
    for alpha in (2.0, 2.0e3):
        R, Dm = truth_response(K, err, H, alpha)
        _, ng, _ = truth_hat(K, err, H, alpha, H, G)
        assert abs(np.trace(R) - ng) <= 1e-12 * ng, (alpha, float(np.trace(R)), float(ng))
        RW = R * np.asarray(H, dtype=LD)[None, :]
        assert np.max(np.abs(RW - RW.T)) <= 1e-13 * np.max(np.abs(RW)), alpha
        lhs = np.dot(Dm, np.dot(np.asarray(K, dtype=LD), np.asarray(f, dtype=LD)) / np.asarray(err, dtype=LD))
        rhs = np.dot(R, np.asarray(f, dtype=LD))
        assert np.max(np.abs(lhs - rhs)) <= 1e-13 * np.max(np.abs(rhs)), alpha
        d = np.diag(R).astype(float)
        assert np.all(d >= 0) and np.all(d <= 1)
    # eta: only alpha / eta enters
    R1, D1 = truth_response(K, err, H, 30.0, eta=2.5)
    R2, D2 = truth_response(K, err, H, 12.0)
    assert np.array_equal(R1, R2) and np.array_equal(D1, D2)


def _fd_setup(entropy):
    n_tau, n_omega = 40, 64
    tau, omega, K, G = synthetic.single_G(n_tau, n_omega)
    K.reduce_singular_space(1e-14)
    Kk = np.array(K.K)
    D = synthetic.flat_D(omega)
    err = synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(n_tau))
    basis = SF.Basis(np.array(K.U), np.array(K.S), np.array(K.V), err)
    kind = device.ENTROPY_NORMAL if entropy == 'normal' else device.ENTROPY_PLUSMINUS
    opts = SF.KernelOptions(tol_h=1e-13, stop_estimate=False)
    alphas = np.array([100.0, 1.0])

    def fit(Gx, Dx):
        v0 = basis.from_v(hostprep.initial_v(K.V, Dx, omega.delta, kind))
        out = SF.alpha_chain(basis, SF.Element(basis, Gx, Dx, entropy), alphas, v0, opts)
        assert out['converged'].all()
        return out['H']
    return np.asarray(omega), Kk, G, D, err, alphas, fit


def fd_true_spectrum(entropy, step):
    """worst error (of a column's largest entry) of the central difference quotient of the re-solved fit under
    G +- eps K e_j against R_t e_j; eps so that the largest whitened data perturbation is ``step``"""
    w_mesh, Kk, G, D, err, alphas, fit = _fd_setup(entropy)
    H0 = fit(G, D)
    worst = 0.0
    for j in (3, 20, 33, 58):
        eps = step / np.max(np.abs(Kk[:, j] / err))
        Hp, Hm = fit(G + eps * Kk[:, j], D), fit(G - eps * Kk[:, j], D)
        for ia, alpha in enumerate(alphas):
            R, _ = truth_response(Kk, err, weights(H0[ia], D, entropy), alpha)
            col = R[:, j].astype(float)
            worst = max(worst, float(np.max(np.abs((Hp[ia] - Hm[ia]) / (2.0 * eps) - col)) / np.max(np.abs(col))))
    return worst


def dlogD_directions(w_mesh):
    return np.stack([np.exp(-(w_mesh - 1.0) ** 2 / 2.0), np.tanh(w_mesh / 3.0)])


def fd_default_model(entropy, step):
    """the same for D exp(+- step d) of two smooth directions d against (I - R_t)(H o d)"""
    w_mesh, Kk, G, D, err, alphas, fit = _fd_setup(entropy)
    H0 = fit(G, D)
    worst = 0.0
    for d in dlogD_directions(w_mesh):
        Hp, Hm = fit(G, D * np.exp(step * d)), fit(G, D * np.exp(-step * d))
        for ia, alpha in enumerate(alphas):
            R, _ = truth_response(Kk, err, weights(H0[ia], D, entropy), alpha)
            f = np.asarray(H0[ia] * d, dtype=LD)
            col = (f - np.dot(R, f)).astype(float)
            worst = max(worst, float(np.max(np.abs((Hp[ia] - Hm[ia]) / (2.0 * step) - col)) / np.max(np.abs(col))))
    return worst


@pytest.mark.parametrize('entropy', ['normal', 'plusminus'])
def test_resolution_operator_is_the_derivative_of_the_fit(entropy):
    """four columns of R_t against the central finite difference of the re-solved fit (tol_h = 1e-13, 40 x 64, per-tau
    errors, alpha = 100 and 1) under G +- eps K e_j, eps such that the largest whitened data perturbation is the step.
    Gate: 1e-6 of the column's largest entry.  Measured worst: step 1e-2: 5.7e-9 (normal), 4.0e-9 (plus-minus); step 1e-3:
    1.3e-8, 7.6e-8 (the noise of the re-solved fits takes over); 1e-4: 4.8e-7, 1.2e-7.  Both of the first two leave more
    than the factor 4 to the gate; 1e-2 is taken."""
    worst = fd_true_spectrum(entropy, FD_STEP_DATA)
    print('R_t against the finite difference of the fit (%s, step %.0e): worst %.2e of the largest entry of a column'
          % (entropy, FD_STEP_DATA, worst))
    assert worst <= GATE, (entropy, worst)


@pytest.mark.parametrize('entropy', ['normal', 'plusminus'])
def test_default_model_response_is_the_derivative_of_the_fit(entropy):
    """(I - R_t)(H o d) for two smooth directions d of ln D against the central finite difference of the re-solved fit
    under D exp(+- step d); same problem and gate.  Measured worst: step 1e-2: 2.7e-8 (normal), 1.8e-5 (plus-minus:
    truncation, it falls with the square of the step); step 1e-3: 1.22e-9, 1.85e-7 (FD_MODEL_ERROR); 1e-4: 1.7e-8, 1.8e-9.  Step 1e-3 leaves
    the factor 4 to the gate for both entropies (5.4 for plus-minus) and is taken."""
    worst = fd_default_model(entropy, FD_STEP_MODEL)
    print('(I - R_t)(H o d) against the finite difference of the fit (%s, step %.0e): worst %.2e of the largest entry'
          % (entropy, FD_STEP_MODEL, worst))
    assert worst <= GATE, (entropy, worst)


def test_summaries_of_a_gaussian_by_hand():
    """A Gaussian of sigma = 0.3 around omega0 = 0.4 on a linear mesh of spacing h = 0.01 over [-4, 4].  The sums are
    trapezoid rules of analytic functions that vanish (below 1e-40) at the ends: their quadrature error is far below the
    rounding of the sums, bound 1e-12.  fwhm interpolates a curve of curvature |p''| <= p_max / sigma^2 linearly inside
    one cell: the crossing moves by at most h^2 |p''| / (8 |p'|) with |p'| = 1.18 p_half / sigma ... at half maximum, i.e.
    by less than h^2 / (4 sigma) = 8.4e-5 per side; bound 2e-4."""
    h, sigma, x0 = 0.01, 0.3, 0.4
    w = np.linspace(-4.0, 4.0, 801)
    delta = np.full(801, h)
    p = np.exp(-(w - x0) ** 2 / (2 * sigma ** 2)) / (sigma * np.sqrt(2 * np.pi))
    j = int(np.argmin(np.abs(w - x0)))
    s = response.psf_summaries(w, delta, p[None, :], np.array([w[j]]))
    assert abs(s['weight'][0] - 1.0) < 1e-12
    assert abs(s['centroid'][0] - x0) < 1e-12 and abs(s['shift'][0] - (x0 - w[j])) < 1e-12
    assert abs(s['spread'][0] - sigma / np.sqrt(2.0)) < 1e-12
    assert abs(s['fwhm'][0] - 2.0 * np.sqrt(2.0 * np.log(2.0)) * sigma) < 2e-4
    assert s['peak'][0] == w[j] and s['height'][0] == p[j]
    # cut by the mesh edge: the left side never falls to half the maximum
    cut = w >= x0 - 0.2
    s2 = response.psf_summaries(w[cut], delta[cut], p[None, cut], np.array([w[j]]))
    assert np.isnan(s2['fwhm'][0]) and np.isfinite(s2['weight'][0]) and np.isfinite(s2['spread'][0])
    # negative side lobes leave the spread defined; a NaN column gives NaN
    q = p * np.cos(6.0 * (w - x0))
    assert np.isfinite(response.psf_summaries(w, delta, q[None, :], np.array([w[j]]))['spread'][0])
    assert np.isnan(response.fwhm(w, np.full(801, np.nan)))


def test_right_hand_sides():
    w = np.linspace(-2.0, 2.0, 9)
    assert list(response.snap_points(w, [0.1, -1.9, 2.0])) == [4, 0, 8]
    assert list(response.snap_points(w)) == list(range(9))
    with pytest.raises(ValueError):
        response.snap_points(w, [2.5])
    assert np.array_equal(response.unit_rows([2, 0], 3), [[0, 0, 1], [1, 0, 0]])
    delta = np.linspace(0.1, 0.9, 9)
    assert np.array_equal(response.spectrum_rows(np.ones((2, 9)), delta), np.tile(delta, (2, 1)))
    H = np.arange(18.0).reshape(2, 9)
    d = np.stack([np.ones(9), w])
    F = response.default_model_rows(H, d)
    assert F.shape == (2, 2, 9) and np.array_equal(F[1, 1], H[1] * w)
    # data rows: K_delta dA, rotated by T (rows: eigenvectors), divided by the errors of the rotated rows
    rng = np.random.RandomState(0)
    Kd, dA = rng.rand(5, 9), rng.rand(3, 9)
    T = np.linalg.qr(rng.rand(5, 5))[0][:4]
    err = 0.1 + rng.rand(4)
    got = response.data_rows(Kd, dA, T, err)
    assert got.shape == (3, 4)
    np.testing.assert_allclose(got, ((T @ (Kd @ dA.T)) / err[:, None]).T, rtol=1e-15)
    np.testing.assert_allclose(response.data_rows(Kd, dA, None, 0.5), (Kd @ dA.T).T / 0.5, rtol=1e-15)


def test_argument_errors_and_symbols():
    assert 'mxe_response' in [s[0] for s in device.SYMBOLS]
    with pytest.raises(ValueError, match='bryan'):
        response.choose_alpha('bryan', 5, None, None)
    assert response.choose_alpha('all', 3, None, None) == ([0, 1, 2], 'many')
    assert response.choose_alpha(1, 3, None, None) == ([1], 'one')
    with pytest.raises(ValueError, match='dlogD'):
        response.check_dlogD(np.ones(7), 7)
    with pytest.raises(ValueError, match='dlogD'):
        response.check_dlogD(np.ones((2, 6)), 7)
    with pytest.raises(ValueError, match='finite'):
        response.check_dlogD(np.full((1, 7), np.inf), 7)
    bad = np.ones((2, 7))
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match='finite'):
        response.spectrum_rows(bad, np.ones(7))
    with pytest.raises(ValueError, match='test'):
        response.spectrum_rows(np.ones((2, 6)), np.ones(7))
    for cls in (mx.TauMaxEnt, mx.ElementwiseMaxEnt, mx.DiagonalMaxEnt, mx.PoormanMaxEnt):
        assert callable(getattr(cls, 'resolution')) and callable(getattr(cls, 'default_model_response'))
    assert callable(device.DeviceContext.response)


def big_data_kernel():
    """n_s > 64: a DataKernel of a seeded Gaussian 80 x 96 matrix, error 0.05 everywhere, a positive H handed in"""
    omega = mx.LinearOmegaMesh(omega_min=-3.0, omega_max=3.0, n_points=96)
    w96 = np.asarray(omega)
    K = kernels.DataKernel(np.arange(80.0), omega, np.random.RandomState(5).randn(80, 96))
    K.reduce_singular_space(1e-14)
    return '80 x 96 gaussian', K, 0.05 * np.ones(80), (np.exp(-w96 ** 2) + 0.01) * omega.delta, None, w96


def rotated_problem():
    """the shape of the GPU test with covariances of differing rank: 60 x 100, rotated into 57 eigen-directions of a
    covariance (T: orthonormal rows), an error per direction; a signed H for the plus-minus entropy"""
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 60, 100)
    K.reduce_singular_space(1e-14)
    rng = np.random.RandomState(4)
    T = np.linalg.qr(rng.randn(60, 60))[0].T[:57]
    err = synthetic.SIGMA * np.sqrt(1.0 + rng.rand(57))
    w_mesh = np.asarray(omega)
    D = synthetic.flat_D(omega)
    return '60 x 100 rotated to 57 rows', _Rotated(K, T), err, D * np.sin(1.3 * w_mesh), D, w_mesh


class _Rotated(object):
    """U, S, V, K of a kernel whose rows are rotated by T"""

    def __init__(self, K, T):
        self.U, self.S, self.V, self.K = np.dot(T, np.array(K.U)), np.array(K.S), np.array(K.V), np.dot(T, np.array(K.K))


def gpu_shapes():
    """(label, kernel with U, S, V, K, err, H, D or None, omega values) of the shapes of the GPU tests; H is a stand-in
    (the formulas are identities for any H the entropy allows): positive for the normal entropy, signed for plus-minus"""
    out = []
    tau, omega, K, G = synthetic.single_G(40, 64)
    K.reduce_singular_space(1e-14)
    err = synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(40))
    D = synthetic.flat_D(omega)
    H = D * np.exp(np.sin(3.0 * np.asarray(omega)))
    out.append(('40 x 64', K, err, H, D, np.asarray(omega)))
    out.append(big_data_kernel())
    out.append(rotated_problem())
    return out


def test_float64_prototype_sits_100x_inside_the_gate():
    """the whitened formula in binary64 (numpy) against the truth on the shapes of the GPU tests: at least 100 x inside
    the 1e-6 gate, so the gate tests the kernel and not the formula"""
    for label, K, err, H, D, w_mesh in gpu_shapes():
        U, S, V, Kk = np.array(K.U), np.array(K.S), np.array(K.V), np.array(K.K)
        n_omega = Kk.shape[1]
        F = rhs_rows(n_omega, w_mesh)
        Fd = np.concatenate([np.eye(Kk.shape[0])[[0, 7, Kk.shape[0] - 1]], (Kk @ F[8:12].T).T / err[None, :]])
        for kind in ('normal', 'plusminus'):
            if (kind == 'plusminus' and D is None) or (kind == 'normal' and np.any(H <= 0)):
                continue
            w = weights(H, D, kind)
            for alpha in (1.0e2, 1.0, 1.0e-2):
                R, Dm = truth_response(Kk, err, w, alpha)
                Xm = np.dot(R, F.T.astype(LD)).T
                e1 = worst_rel(prototype(U, S, V, err, w, alpha, F), Xm)
                Xu = Xm / np.asarray(w, dtype=LD)[None, :]
                e2 = worst_rel(prototype(U, S, V, err, w, alpha, F, weighted=False), Xu)
                Xd = np.dot(Dm, Fd.T.astype(LD)).T
                e3 = worst_rel(prototype(U, S, V, err, w, alpha, Fd, space='data'), Xd)
                print('%s, %s, alpha %g: prototype off by %.1e (model), %.1e (unweighted), %.1e (data)'
                      % (label, kind, alpha, e1, e2, e3))
                assert max(e1, e2, e3) <= GATE / 100, (label, kind, alpha, e1, e2, e3)
