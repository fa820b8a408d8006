"""Host side of the fit diagnostics: the extended-precision truth the GPU tests compare against, pinned against a
50-digit solve and against the finite-difference derivative of the fit, and the formulas of ``maxent_amd.diagnostics``.

The truth is independent of the library and of the whitened form the kernel evaluates: with
``Y = diag(sqrt w) K^T Sigma^-1/2`` in ``np.longdouble`` the hat matrix is

    Hat = Y^T (a I + Y Y^T)^-1 Y,      a = alpha~ / eta,      a I + Y Y^T = L L^T

so the leverage h_i is the squared norm of column i of ``L^-1 Y``; ``r = Sigma^-1/2 (K H - G)``.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_posterior_errors_host import LD, cholesky_ld, forward_ld, small_problem      # noqa: E402
from maxent_amd import diagnostics, synthetic, hostprep, device                       # noqa: E402
from oracle import sform as SF                                                         # noqa: E402


def truth_hat(K, err, w, alpha, H, G, eta=1.0, full=False):
    """leverages, number of good data and whitened residuals of the fit H of the data G: K the kernel matrix of the
    problem (rows in the space where the errors ``err`` are independent), w the entropy weights at H, alpha the scaled alpha
    of Q = eta chi2 / 2 - alpha S.  Returns (h, N_g, r) as longdouble; ``full``: the whole hat matrix instead of h."""
    K = np.asarray(K, dtype=LD)
    err = np.asarray(err, dtype=LD) * np.ones(K.shape[0], dtype=LD)
    w = np.asarray(w, dtype=LD)
    a = LD(alpha) / LD(eta)
    Y = np.sqrt(w)[:, None] * (K / err[:, None]).T              # n_omega x n_data
    A = np.dot(Y, Y.T)
    A[np.diag_indices_from(A)] += a
    Z = forward_ld(cholesky_ld(A), Y)
    h = np.sum(Z * Z, axis=0)
    r = (np.dot(K, np.asarray(H, dtype=LD)) - np.asarray(G, dtype=LD)) / err
    return (np.dot(Z.T, Z) if full else h), np.sum(h), r


def test_longdouble_truth_against_50_digit_solve():
    import mpmath as mp
    mp.mp.dps = 50
    omega, K, H, err = small_problem()
    n_tau, n = K.shape
    G = K @ H + err * np.random.RandomState(5).randn(n_tau)
    for alpha in (2.0, 2.0e3):
        h, ng, r = truth_hat(K, err, H, alpha, H, G)
        Km = mp.matrix(K.tolist())
        sig = [mp.mpf(float(e)) for e in err]
        hess = mp.zeros(n, n)
        for i in range(n):
            for j in range(n):
                hess[i, j] = mp.fsum(Km[t, i] * Km[t, j] / sig[t] ** 2 for t in range(n_tau))
            hess[i, i] += mp.mpf(alpha) / mp.mpf(float(H[i]))
        inv = mp.inverse(hess)
        total = mp.mpf(0)
        for t in range(n_tau):
            row = [Km[t, i] / sig[t] for i in range(n)]
            exact = mp.fsum(row[i] * inv[i, j] * row[j] for i in range(n) for j in range(n))
            total += exact
            assert abs(mp.mpf(float(h[t])) / exact - 1) < 1e-12, (alpha, t, float(h[t]), exact)
            assert 0 < float(h[t]) < 1
            rt = (mp.fsum(Km[t, i] * mp.mpf(float(H[i])) for i in range(n)) - mp.mpf(float(G[t]))) / sig[t]
            assert abs(mp.mpf(float(r[t])) - rt) < 1e-12 * max(1, abs(rt)), (alpha, t)
        assert abs(mp.mpf(float(ng)) / total - 1) < 1e-12


def test_truth_with_chi2_factor_is_the_scaled_problem():
    omega, K, H, err = small_problem()
    G = K @ H
    h1, n1, _ = truth_hat(K, err, H, 30.0, H, G, eta=2.5)
    h2, n2, _ = truth_hat(K, err, H, 30.0 / 2.5, H, G)
    assert np.array_equal(h1, h2) and n1 == n2


@pytest.mark.parametrize('entropy', ['normal', 'plusminus'])
def test_hat_matrix_is_the_derivative_of_the_fit(entropy):
    """four columns of the truth's hat matrix against the central finite difference of the re-solved fit with respect to
    the data (perturbation 1e-2 sigma_j).  Gate 1e-6 of the column's largest entry.  Measured worst on these columns:
    2.5e-7 (normal), 9.4e-8 (plus-minus) -- the truncation error of the difference quotient: 2.1e-8 at 1e-3 sigma_j,
    where the noise of the re-solved fits (tol_h = 1e-13) takes over."""
    n_tau, n_omega = 40, 64
    tau, omega, K, G = synthetic.single_G(n_tau, n_omega)
    K.reduce_singular_space(1e-14)
    Kk = np.array(K.K)
    D = synthetic.flat_D(omega)
    err = synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(n_tau))
    basis = SF.Basis(np.array(K.U), np.array(K.S), np.array(K.V), err)
    kind = device.ENTROPY_NORMAL if entropy == 'normal' else device.ENTROPY_PLUSMINUS
    v0 = basis.from_v(hostprep.initial_v(K.V, D, omega.delta, kind))
    opts = SF.KernelOptions(tol_h=1e-13, stop_estimate=False)
    alphas = np.array([100.0, 1.0])

    def fit(Gx):
        out = SF.alpha_chain(basis, SF.Element(basis, Gx, D, entropy), alphas, v0, opts)
        assert out['converged'].all()
        return out['H']

    H0 = fit(G)
    eps = 1e-2
    worst = 0.0
    for j in (0, 7, 22, n_tau - 1):
        dG = np.zeros(n_tau)
        dG[j] = eps * err[j]
        Hp, Hm = fit(G + dG), fit(G - dG)
        for ia, alpha in enumerate(alphas):
            w = H0[ia] if entropy == 'normal' else np.sqrt(H0[ia] ** 2 + 4.0 * D ** 2)
            Hat, _, _ = truth_hat(Kk, err, w, alpha, H0[ia], G, full=True)
            col = (Kk @ (Hp[ia] - Hm[ia])) / err / (2.0 * eps)
            rel = float(np.max(np.abs(col - Hat[:, j].astype(float))) / np.max(np.abs(Hat[:, j].astype(float))))
            worst = max(worst, rel)
            assert rel <= 1e-6, (entropy, j, alpha, rel)
    print('hat matrix against the finite difference (%s): worst %.2e of the largest entry of a column' % (entropy, worst))


def test_studentized_gcv_ratio_and_autocorr_by_hand():
    r = np.array([[1.0, -2.0, 0.5], [np.nan, np.nan, np.nan]])
    h = np.array([[0.75, 0.0, 1.0 - 1e-13], [np.nan, np.nan, np.nan]])
    st = diagnostics.studentized(r, h)
    assert st[0, 0] == 2.0 and st[0, 1] == -2.0 and np.isnan(st[0, 2]) and np.all(np.isnan(st[1]))
    ac = diagnostics.autocorr(r)
    assert abs(ac[0] - (1.0 * -2.0 + -2.0 * 0.5) / (1.0 + 4.0 + 0.25)) < 1e-15 and np.isnan(ac[1])
    # NaN padding behind the rows of a shorter element is left out of both sums
    assert diagnostics.autocorr(np.array([1.0, -2.0, 0.5, np.nan]))[()] == ac[0]
    assert np.isnan(diagnostics.autocorr(np.array([3.0])))
    chi2, ng = np.array([12.0, 8.0, np.nan, 5.0]), np.array([2.0, 6.0, np.nan, 10.0])
    g = diagnostics.gcv(chi2, ng, 10)
    assert g[0] == 10 * 12.0 / 64.0 and g[1] == 10 * 8.0 / 16.0 and np.isnan(g[2]) and np.isnan(g[3])
    assert diagnostics.index_gcv(g) == 0
    ratio = diagnostics.good_data_ratio(np.array([4.0, 2.0, 1.0, 1.0]), np.array([-2.0, -1.0, np.nan, -3.0]), np.array([2.0, 5.0, 3.0, 0.0]))
    assert ratio[0] == 8.0 and ratio[1] == 0.8 and np.isnan(ratio[2]) and np.isnan(ratio[3])
    assert diagnostics.index_classic(ratio) == 1
    assert diagnostics.index_classic(np.array([np.nan, 0.1, -1.0, 7.0])) == 3      # |log 7| < |log 0.1|
    with pytest.raises(ValueError):
        diagnostics.index_gcv(np.array([np.nan, np.nan]))
    with pytest.raises(ValueError):
        diagnostics.index_classic(np.array([np.nan, -1.0, 0.0]))


def test_argument_errors():
    with pytest.raises(ValueError, match='no analyzer of this name'):
        diagnostics.choose_alpha('NoSuchAnalyzer', 5, {}, None)
    with pytest.raises(ValueError, match='bryan'):
        diagnostics.choose_alpha('bryan', 5, {}, None)
    with pytest.raises(ValueError, match='out of range'):
        diagnostics.choose_alpha(5, 5, {}, None)
    assert diagnostics.choose_alpha('all', 3, {}, None) == ([0, 1, 2], 'many')
    assert diagnostics.choose_alpha(-1, 3, {}, None) == ([2], 'one')
    # a result of another alpha mesh is refused before the device is touched
    import maxent_amd as mx
    tau, omega, K, G = synthetic.single_G(40, 64)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = omega
    tm.set_G_tau_data(tau, G)
    tm.set_error(synthetic.SIGMA)
    tm.alpha_mesh = synthetic.alpha_mesh(6)

    class Other(object):
        alpha = np.asarray(tm.maxent_loop.make_spec()['alpha'])[:5]
    with pytest.raises(ValueError, match='alphas of the result are not those of this object'):
        tm.fit_diagnostics(Other())
    Other.alpha = np.asarray(tm.maxent_loop.make_spec()['alpha']) * 2.0
    with pytest.raises(ValueError, match='alphas of the result are not those of this object'):
        tm.fit_diagnostics(Other())
