"""Host side of the posterior error bars: the extended-precision truth the GPU tests compare against, pinned against a
50-digit solve, and the glue of ``maxent_amd.posterior`` (windows, preblur rows, the Bryan mixture, argument errors).

The truth is independent of the library and of the Woodbury form the kernel evaluates: with
``Y = diag(sqrt w) K^T Sigma^-1/2`` in ``np.longdouble``,

    var(f^T H) = (sqrt w o f)^T (alpha~ I + Y Y^T)^-1 (sqrt w o f)

by a Cholesky solve of the n_omega x n_omega matrix, whose condition number is (alpha~ + lambda_max) / alpha~ (the raw
Hessian's 1/w diagonal spans twenty decades instead).
"""
import numpy as np
import pytest

from maxent_amd import posterior

LD = np.longdouble


def cholesky_ld(A):
    """lower Cholesky factor of a symmetric positive definite matrix in extended precision"""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    for j in range(n):
        d = np.sqrt(A[j, j])
        assert d > 0
        A[j, j] = d
        A[j + 1:, j] /= d
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def forward_ld(L, Bm):
    """L^-1 Bm, columns at once"""
    Z = np.array(Bm, dtype=LD)
    for k in range(L.shape[0]):
        Z[k] /= L[k, k]
        Z[k + 1:] -= np.outer(L[k + 1:, k], Z[k])
    return Z


def truth_var(K, err, w, alpha, F, eta=1.0):
    """variances of the functionals F (n_f, n_omega) on H: K the kernel matrix of the problem (rows in the space where
    the errors ``err`` are independent), w the entropy weights, alpha the scaled alpha of Q = eta chi2 / 2 - alpha S.
    Returns (var, prior) as longdouble arrays of n_f values."""
    K, err, w = np.asarray(K, dtype=LD), np.asarray(err, dtype=LD) * np.ones(np.shape(K)[0], dtype=LD), np.asarray(w, dtype=LD)
    a = LD(alpha) / LD(eta)
    sw = np.sqrt(w)
    Y = sw[:, None] * (K / err[:, None]).T                      # n_omega x n_data
    A = np.dot(Y, Y.T)
    A[np.diag_indices_from(A)] += a
    L = cholesky_ld(A)
    R = sw[:, None] * np.asarray(F, dtype=LD).T                 # n_omega x n_f
    Z = forward_ld(L, R)
    var = np.sum(Z * Z, axis=0) / LD(eta)
    prior = np.sum(w[None, :] * np.asarray(F, dtype=LD) ** 2, axis=1) / LD(alpha)
    return var, prior


def small_problem(n_tau=24, n_omega=36, sigma=1e-3, seed=3):
    rng = np.random.RandomState(seed)
    tau = np.linspace(0.0, 10.0, n_tau)
    omega = np.linspace(-4.0, 4.0, n_omega)
    K = np.exp(-np.outer(tau, omega)) / (1.0 + np.exp(-10.0 * omega))[None, :]
    H = np.exp(-(omega - 0.7) ** 2) * (omega[1] - omega[0]) * (1.0 + 0.1 * rng.rand(n_omega))
    err = sigma * (1.0 + rng.rand(n_tau))
    return omega, K, H, err


def test_longdouble_truth_against_50_digit_solve():
    import mpmath as mp
    mp.mp.dps = 50
    omega, K, H, err = small_problem()
    n = len(omega)
    F = np.stack([np.ones(n), omega, (np.abs(omega - 0.7) < 0.5).astype(float), np.eye(n)[n // 2]])
    for alpha in (2.0, 2.0e3):
        var, prior = truth_var(K, err, H, alpha, F)
        Km = mp.matrix(K.tolist())
        hess = mp.zeros(n, n)
        for i in range(n):
            for j in range(n):
                hess[i, j] = mp.fsum(Km[t, i] * Km[t, j] / mp.mpf(float(err[t])) ** 2 for t in range(K.shape[0]))
            hess[i, i] += mp.mpf(alpha) / mp.mpf(float(H[i]))
        for k in range(len(F)):
            f = mp.matrix(F[k].tolist())
            x = mp.lu_solve(hess, f)
            exact = mp.fsum(f[i] * x[i] for i in range(n))
            assert abs(mp.mpf(float(var[k])) / exact - 1) < 1e-12, (alpha, k, float(var[k]), exact)
            assert float(var[k]) <= float(prior[k])


def test_truth_with_chi2_factor_is_the_scaled_problem():
    omega, K, H, err = small_problem()
    F = np.ones((1, len(omega)))
    v1, p1 = truth_var(K, err, H, 30.0, F, eta=2.5)
    v2, p2 = truth_var(K, err, H, 30.0 / 2.5, F)
    assert abs(float(v1[0] / (v2[0] / LD(2.5))) - 1) < 1e-15 and abs(float(p1[0] / (p2[0] / LD(2.5))) - 1) < 1e-15


def test_window_rows_are_indicators():
    w = np.linspace(-2, 2, 9)
    rows = posterior.window_rows(w, [(-1.0, 1.0), (0.4, 2.0)])
    np.testing.assert_array_equal(rows[0], (np.abs(w) <= 1.0).astype(float))
    np.testing.assert_array_equal(rows[1], ((w >= 0.4) & (w <= 2.0)).astype(float))
    for bad in ([(-3.0, 0.0)], [(0.0, 2.5)], [(1.0, 0.5)], [(0.1, 0.2)], [(0.0,)], [(0.0, np.nan)]):
        with pytest.raises(ValueError):
            posterior.window_rows(w, bad)


def test_preblur_rows_are_B_transposed_f():
    rng = np.random.RandomState(0)
    n = 7
    B, delta, f, H = rng.rand(n, n), 0.1 + rng.rand(n), rng.randn(2, n), rng.rand(n)
    rows = posterior.rows_on_H(f, delta, B)
    A = B @ H
    np.testing.assert_allclose(rows @ H, (f * delta) @ A, rtol=1e-13)
    np.testing.assert_allclose(rows, (B.T @ (f * delta).T).T, rtol=1e-13)
    assert posterior.rows_on_H(f, delta, None) is not None and np.array_equal(posterior.rows_on_H(f, delta, None), f)
    # without a preblur A delta = H: the weight on H is f itself
    np.testing.assert_allclose(posterior.rows_on_H(f, delta) @ H, f @ ((H / delta) * delta), rtol=1e-13)


def test_bryan_mixture_three_alphas_by_hand():
    logp = np.array([-3.0, -1.0, -2.0])
    alpha = np.array([1.0, 10.0, 100.0])
    good, p = posterior.bryan_weights(logp, alpha)
    e = np.exp(np.array([-2.0, 0.0, -1.0]))
    np.testing.assert_allclose(p, e / e.sum(), rtol=1e-15)
    assert good.all()
    x = np.array([[1.0], [2.0], [4.0]])
    v = np.array([[0.1], [0.2], [0.3]])
    mean, var = posterior.bryan_mixture(p, x, v)
    m = p[0] * 1 + p[1] * 2 + p[2] * 4
    s2 = p[0] * (0.1 + (1 - m) ** 2) + p[1] * (0.2 + (2 - m) ** 2) + p[2] * (0.3 + (4 - m) ** 2)
    assert abs(mean[0] - m) < 1e-15 and abs(var[0] - s2) < 1e-15
    # by integration: the analyzer's own normalisation (trapezoid, then the alpha mesh's delta)
    from maxent_amd.analyzers import get_delta
    good, q = posterior.bryan_weights(logp, alpha, average_by_integration=True)
    ref = np.exp(logp - logp.max())
    ref = ref / np.trapezoid(ref, alpha) * get_delta(alpha)
    np.testing.assert_allclose(q, ref, rtol=1e-15)
    # a NaN probability drops its alpha; none at all is the analyzer's message
    good, p = posterior.bryan_weights(np.array([np.nan, -1.0, -2.0]), alpha)
    assert good.tolist() == [False, True, True] and abs(p.sum() - 1) < 1e-15
    with pytest.raises(ValueError, match='Probability not calculated. Cannot use BryanAnalyzer.'):
        posterior.bryan_weights(np.full(3, np.nan), alpha)


def test_choose_alpha_and_argument_errors():
    ana = {'LineFitAnalyzer': {'alpha_index': 4}, 'BryanAnalyzer': {'A_out': None}}
    assert posterior.choose_alpha(None, 10, ana, 'LineFitAnalyzer') == ([4], 'one')
    assert posterior.choose_alpha(None, 10, ana, None) == ([4], 'one')
    assert posterior.choose_alpha(3, 10, ana, None) == ([3], 'one')
    assert posterior.choose_alpha(-1, 10, ana, None) == ([9], 'one')
    assert posterior.choose_alpha([0, 9], 10, ana, None) == ([0, 9], 'many')
    assert posterior.choose_alpha('all', 3, ana, None) == ([0, 1, 2], 'many')
    assert posterior.choose_alpha('bryan', 3, ana, None)[1] == 'bryan'
    for bad in (10, [0, 11], [], 'NoSuchAnalyzer', 'BryanAnalyzer'):
        with pytest.raises(ValueError):
            posterior.choose_alpha(bad, 10, ana, None)
    with pytest.raises(ValueError):
        posterior.functional_rows(np.ones((2, 5)), 6)
    with pytest.raises(ValueError):
        posterior.functional_rows(np.array([[1.0, np.nan]]), 2)
    with pytest.raises(ValueError):
        posterior.check_alpha(dict(alpha=np.array([1.0, 2.0])), np.array([1.0, 3.0]))


def test_entropy_weights():
    from maxent_amd import device
    H, D = np.array([0.3, -0.2]), np.array([0.1, 0.05])
    np.testing.assert_array_equal(posterior.entropy_weights(H, D, device.ENTROPY_NORMAL), H)
    np.testing.assert_allclose(posterior.entropy_weights(H, D, device.ENTROPY_PLUSMINUS), np.sqrt(H ** 2 + 4 * D ** 2), rtol=1e-15)


def test_public_methods_exist_and_need_a_device():
    import maxent_amd as mx
    assert callable(mx.TauMaxEnt.posterior_errors) and callable(mx.ElementwiseMaxEnt.posterior_errors)
    assert callable(mx.DiagonalMaxEnt.posterior_errors) and callable(mx.PoormanMaxEnt.posterior_errors)
    from maxent_amd import device
    assert 'mxe_posterior_var' in [s[0] for s in device.SYMBOLS]
    assert callable(device.DeviceContext.posterior_var)
