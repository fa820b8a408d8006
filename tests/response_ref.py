"""Helpers of the response tests (``test_response_host.py``, ``test_gpu_response.py``): the extended-precision truth, a
binary64 prototype of the whitened formula the kernel evaluates, and the problems both files use.

The truth is independent of the library and of the whitened form: with ``Y = diag(sqrt w) K^T Sigma^-1/2`` in
``np.longdouble`` and ``a = alpha~ / eta``

    (eta K^T Sigma^-1 K + alpha~ diag(1/w))^-1 = (1/eta) diag(sqrt w) (a I + Y Y^T)^-1 diag(sqrt w)
    Dm  = Gamma eta K^T Sigma^-1/2 = diag(sqrt w) (a I + Y Y^T)^-1 Y              (the data-space map, n_omega x n_data)
    R_t = Dm Sigma^-1/2 K                                                       (n_omega x n_omega)

by a Cholesky solve of the n_omega x n_omega matrix ``a I + Y Y^T``, whose condition number is (a + lambda_max) / a; no
division by w anywhere.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_posterior_errors_host import LD, cholesky_ld, forward_ld      # noqa: E402

GATE = 1e-6


def backward_ld(L, Z):
    """L^-T Z, columns at once"""
    X = np.array(Z, dtype=LD)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] /= L[k, k]
        X[:k] -= np.outer(L[k, :k], X[k])
    return X


def truth_response(K, err, w, alpha, eta=1.0):
    """(R_t, Dm) as longdouble: the resolution operator (n_omega x n_omega) and the response of H to the whitened data
    (n_omega x n_data).  K: the kernel matrix of the problem (rows in the space where the errors ``err`` are independent),
    w the entropy weights, alpha the scaled alpha of Q = eta chi2 / 2 - alpha S."""
    K = np.asarray(K, dtype=LD)
    err = np.asarray(err, dtype=LD) * np.ones(K.shape[0], dtype=LD)
    w = np.asarray(w, dtype=LD)
    a = LD(alpha) / LD(eta)
    sw = np.sqrt(w)
    Kw = K / err[:, None]                                       # Sigma^-1/2 K
    Y = sw[:, None] * Kw.T
    A = np.dot(Y, Y.T)
    A[np.diag_indices_from(A)] += a
    L = cholesky_ld(A)
    Dm = sw[:, None] * backward_ld(L, forward_ld(L, Y))
    return np.dot(Dm, Kw), Dm


def weights(H, D, kind):
    return np.asarray(H) if kind == 'normal' else np.sqrt(np.asarray(H) ** 2 + 4.0 * np.asarray(D) ** 2)


def prototype(U, S, V, err, w, alpha, F, space='model', weighted=True, eta=1.0):
    """binary64 prototype of what ``response_kernel`` evaluates: with Sigma^-1/2 U S = U^ c Q^T (thin SVD), V' = V Q,
    B = c W c + a I = L L^T:  X = [diag(w)] V' c B^-1 y,  y = c o V'^T F^T (model) or U^^T F^T (data).  ``F``: (n, ld).
    Returns (n, n_omega)."""
    U, S, V = (np.asarray(x, dtype=float) for x in (U, S, V))
    err = np.asarray(err, dtype=float) * np.ones(U.shape[0])
    Uh, c, Qt = np.linalg.svd((U * S[None, :]) / err[:, None], full_matrices=False)
    Vp = V @ Qt.T
    a = float(alpha) / float(eta)
    w = np.asarray(w, dtype=float)
    B = c[:, None] * (Vp.T @ (w[:, None] * Vp)) * c[None, :] + a * np.eye(len(c))
    L = np.linalg.cholesky(B)
    F = np.atleast_2d(np.asarray(F, dtype=float))
    y = c[:, None] * (Vp.T @ F.T) if space == 'model' else Uh.T @ F[:, :U.shape[0]].T
    z = np.linalg.solve(L, y)
    x = np.linalg.solve(L.T, z)
    X = (Vp @ (c[:, None] * x)).T
    return X * w[None, :] if weighted else X


def rhs_rows(n_omega, omega, seed=11):
    """the 20 right-hand sides of the small model-space tests: 8 unit vectors, 12 smooth and oscillating rows"""
    x = np.asarray(omega, dtype=float)
    s = (x - x.min()) / (x.max() - x.min())
    units = np.eye(n_omega)[[0, 5, 17, 31, 32, 47, 62, n_omega - 1]]
    smooth = [np.ones(n_omega), s, np.exp(-(x - 1.0) ** 2), np.exp(-(x + 2.0) ** 2 / 4.0), s * (1 - s), 1.0 / (1.0 + x * x)]
    wavy = [np.cos(np.pi * k * s) for k in (1, 2, 5, 9)] + [np.sin(2 * np.pi * 3 * s) * np.exp(-x * x / 8.0), (-1.0) ** np.arange(n_omega)]
    return np.concatenate([units, np.array(smooth), np.array(wavy)])


def worst_rel(X, Xt):
    """max over the rows of max|X - X_t| / max|X_t| (rows: right-hand sides)"""
    X, Xt = np.asarray(X, dtype=LD), np.asarray(Xt, dtype=LD)
    return float(np.max(np.max(np.abs(X - Xt), axis=-1) / np.max(np.abs(Xt), axis=-1)))
