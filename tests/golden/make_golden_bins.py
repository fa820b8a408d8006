#!/usr/bin/env python3
"""Generate bins.npz: Monte Carlo bins of G(tau) and what the REAL reference makes of their mean and covariance.

Runs only where the reference checkout is (it imports it the way make_golden.py does).  The reference has no
setter for bins: it is given what a user computes from them today, ``set_G_tau_data(tau, mean)`` and ``set_cov(C)``
with ``C = X^T X``, ``X = (bins - mean) / sqrt(n_bins (n_bins - 1))``, mean and C formed in longdouble and rounded.

  s_*    one element: n_bins = 256, n_tau = 40
  e_*    2 x 2 elements (hermiticity off): n_bins = 200, n_tau = 30
The noise of a bin is an AR(1) process along tau (correlation 0.5 between neighbours) whose amplitude decays along tau
by a factor 5.  Per case: ``tau``, ``bins``, ``mean``, ``cov``, ``omega``, ``A_true`` (the spectrum the bins were made
from), the reference's ``alpha``, ``A``, ``H``, ``chi2``, ``A_out`` and ``H_truth``, every solve of the reference
polished in extended precision (make_golden.truth_rows).  The 2 x 2 case runs one fresh reference object per element.

Conditions on the input (asserted here): lambda_max / lambda_min of every covariance <= 1e8, nothing is cut by
cov_threshold = 1e-14 and no eigenvalue lies within a factor 2 of it -- at this conditioning eigh(C) is a valid
yardstick for the device's SVD of X.

Usage:  python tests/golden/make_golden_bins.py
"""

import os

import numpy as np

import make_golden as mg
from make_golden import (TauMaxEnt, HyperbolicOmegaMesh, LogAlphaMesh, TauKernel, VerbosityFlags,
                         R)

HERE = os.path.dirname(os.path.abspath(__file__))
COV_THRESHOLD = 1e-14


def ar1_bins(rng, G, n_bins, amp):
    n = len(G)
    z = np.empty((n_bins, n))
    z[:, 0] = rng.randn(n_bins)
    for t in range(1, n):
        z[:, t] = 0.5 * z[:, t - 1] + np.sqrt(0.75) * rng.randn(n_bins)
    return G[None, :] + amp * np.exp(-np.log(5.0) * np.arange(n) / (n - 1))[None, :] * z


def mean_and_cov(bins):
    b = np.asarray(bins, dtype=np.longdouble)
    nb = b.shape[0]
    mean = b.mean(axis=0)
    X = (b - mean) / np.sqrt(np.longdouble(nb) * (nb - 1))
    C = np.asarray(X.T @ X, dtype=float)
    lam = np.linalg.eigvalsh(C)
    assert lam.min() > 2 * COV_THRESHOLD and lam.max() / lam.min() <= 1e8, (lam.min(), lam.max())
    return np.asarray(mean, dtype=float), C, lam


def spectra(omega):
    w = np.array(omega)
    A0 = 0.6 * np.exp(-(w - 1.0) ** 2 / (2 * 0.5 ** 2)) + 0.4 * np.exp(-(w + 1.5) ** 2 / (2 * 0.8 ** 2))
    A0 /= np.trapezoid(A0, w)
    A1 = 0.5 * np.exp(-(w + 0.5) ** 2 / (2 * 0.6 ** 2)) + 0.5 * np.exp(-(w - 2.0) ** 2 / (2 * 0.7 ** 2))
    A1 /= np.trapezoid(A1, w)
    Aoff = 0.3 * (np.exp(-(w - 1.0) ** 2 / (2 * 0.5 ** 2)) - np.exp(-(w + 1.5) ** 2 / (2 * 0.8 ** 2)))
    return A0, A1, Aoff


def single_case(out):
    n_bins, n_tau, n_w, n_alpha, beta = 256, 40, 60, 8, 40.0
    rng = np.random.RandomState(3141)
    tau = np.linspace(0, beta, n_tau)
    omega = HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=n_w)
    K = TauKernel(tau=tau, omega=omega, beta=beta)
    A0 = spectra(omega)[0]
    bins = ar1_bins(rng, K.K_delta @ A0, n_bins, 2e-3)
    mean, C, lam = mean_and_cov(bins)
    tm = TauMaxEnt(cov_threshold=COV_THRESHOLD)
    tm.set_verbosity(VerbosityFlags.Quiet)
    tm.omega = omega
    tm.set_G_tau_data(tau, mean)
    tm.set_cov(C)
    tm.alpha_mesh = LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=n_alpha)
    vs, its, conv = mg.record_v(tm)
    res = tm.run()
    p = R.Problem(np.array(tm.K.K), tm.K.U, tm.K.S, tm.K.V, np.array(tm.G), np.array(tm.err), np.array(tm.D.D))
    mg.check_port(p, omega.delta, tm.alpha_mesh, res, its)
    Ht = mg.truth_rows(p, np.array(res.alpha), vs, 'normal', list(range(n_alpha)))
    e = np.linalg.norm(np.array(res.H) - Ht, axis=1) / np.linalg.norm(Ht, axis=1)
    print('single: lambda %.2e .. %.2e, rank %d, reference vs truth max %.2e' % (lam.min(), lam.max(), len(tm.err), e.max()))
    out.update(s_tau=tau, s_bins=bins, s_mean=mean, s_cov=C, s_omega=np.array(omega), s_A_true=A0, s_beta=beta,
               s_alpha=np.array(res.alpha), s_A=np.array(res.A), s_H=np.array(res.H), s_chi2=np.array(res.chi2),
               s_A_out=np.array(res.analyzer_results['LineFitAnalyzer']['A_out']), s_H_truth=Ht)


def elementwise_case(out):
    n_bins, n_tau, n_w, n_alpha, beta = 200, 30, 60, 6, 40.0
    rng = np.random.RandomState(2653)
    tau = np.linspace(0, beta, n_tau)
    omega = HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=n_w)
    K = TauKernel(tau=tau, omega=omega, beta=beta)
    A0, A1, Aoff = spectra(omega)
    Amat = [[A0, Aoff], [Aoff, A1]]
    bins = np.empty((n_bins, 2, 2, n_tau))
    mean = np.empty((2, 2, n_tau))
    cov = np.empty((2, 2, n_tau, n_tau))
    for i in range(2):
        for j in range(2):
            bins[:, i, j, :] = ar1_bins(rng, K.K_delta @ Amat[i][j], n_bins, 2e-3 * (1.0 + 0.3 * (i + 2 * j)))
            mean[i, j], cov[i, j], lam = mean_and_cov(bins[:, i, j, :])
            print('element %d %d: lambda %.2e .. %.2e' % (i, j, lam.min(), lam.max()))
    # one FRESH reference object per element (normal entropy on the diagonal, plus-minus off it, as ElementwiseMaxEnt's
    # workers): a reused worker would move the data by the hop from the previous element's rotation (tau_maxent.py:253-288)
    shape = (2, 2, n_alpha, n_w)
    res_A, res_H, Ht = (np.empty(shape) for _ in range(3))
    res_chi2 = np.empty(shape[:3])
    A_out = np.empty((2, 2, n_w))
    alpha = None
    for i in range(2):
        for j in range(2):
            ent = 'normal' if i == j else 'plusminus'
            tm = TauMaxEnt(cov_threshold=COV_THRESHOLD) if i == j else \
                TauMaxEnt(cov_threshold=COV_THRESHOLD, cost_function='plusminus')
            tm.set_verbosity(VerbosityFlags.Quiet)
            tm.omega = omega
            tm.set_G_tau_data(tau, mean[i, j])
            tm.set_cov(cov[i, j])
            tm.alpha_mesh = LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=n_alpha)
            vs, its, conv = mg.record_v(tm)
            res = tm.run()
            p = R.Problem(np.array(tm.K.K), tm.K.U, tm.K.S, tm.K.V, np.array(tm.G), np.array(tm.err), np.array(tm.D.D),
                          entropy=ent)
            Ht[i, j] = mg.truth_rows(p, np.array(res.alpha), vs, ent, list(range(n_alpha)))
            res_A[i, j], res_H[i, j], res_chi2[i, j] = np.array(res.A), np.array(res.H), np.array(res.chi2)
            A_out[i, j] = np.array(res.analyzer_results['LineFitAnalyzer']['A_out'])
            alpha = np.array(res.alpha)
            e = np.linalg.norm(res_H[i, j] - Ht[i, j], axis=-1) / np.linalg.norm(Ht[i, j], axis=-1)
            print('element %d %d: reference vs truth max %.2e' % (i, j, e.max()))
    out.update(e_tau=tau, e_bins=bins, e_mean=mean, e_cov=cov, e_omega=np.array(omega),
               e_A_true=np.array([[A0, Aoff], [Aoff, A1]]), e_beta=beta, e_alpha=alpha,
               e_A=res_A, e_H=res_H, e_chi2=res_chi2, e_A_out=A_out, e_H_truth=Ht)


def main():
    out = dict(cov_threshold=np.array(COV_THRESHOLD))
    single_case(out)
    elementwise_case(out)
    path = os.path.join(HERE, 'bins.npz')
    np.savez_compressed(path, **out)
    print('bins.npz: %d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
