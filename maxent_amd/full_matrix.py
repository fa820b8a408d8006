"""Whole-matrix continuation: ``FullMatrixMaxEnt`` (no counterpart in the reference).

``ElementwiseMaxEnt`` and ``PoormanMaxEnt`` continue a matrix-valued G one element at a time; the matrix A(omega) they give
is Hermitian but, as a rule, not positive semi-definite (``positivity()`` measures by how much).  The reference's guide names
the way out -- "treating the spectral function matrix as a whole", a ``FullMatrixMaxEnt`` it announces and never shipped.
This is it: the unknown is the matrix H_i = D_i exp(Gamma_i) at every frequency, the entropy is the matrix entropy
S = sum_i Tr[H_i - D_i - H_i log(H_i / D_i)] (Kraberger et al., PRB 96, 155128), chi2 is the Frobenius misfit over all
matrix elements, and the solution is Hermitian and positive semi-definite at every omega and alpha because it is a matrix
exponential.  DESIGN 4z has the equations; ``mxe_fullmatrix_solve`` (maxent_amd/csrc/mxe_fullmatrix.hip.h) solves them,
one workgroup per problem; there is no CPU path (``tests/fullmatrix_ref.py`` is a numpy truth for the tests).

What it takes, everything else is refused with NotImplementedError or ValueError: G(tau) or Legendre data (a real kernel
acting on a Hermitian A); one error -- a scalar or one value per tau -- shared by all matrix elements (``set_error``,
``err=``), or one error bar per matrix element, sigma_ab or sigma_ab(tau) with sigma_ab = sigma_ba (``set_element_errors``,
``element_err=``; ``mxe_fullmatrix_solve_metric``: a dense n_s x n_s metric per Hermitian component in the place of the
diagonal S / sigma); the default model D(omega) times the unit matrix; M <= 4 and n_s <= 64.  Not supported: Matsubara and
bosonic data, ``set_cov``, bins, preblur, a matrix-valued default model, the probability-based analyzers (Bryan, Classic)
and ``probability=``.

Error bars: ``FullMatrixMaxEnt.posterior_errors`` / :func:`full_matrix_posterior_errors` (``mxe_fullmatrix_posterior_var``,
DESIGN 4za), the Gaussian posterior around the minimiser for spectral weights in windows, linear functionals and every
A_ab(omega_i); for a job with one error for all matrix elements.  The probability of alpha: ``FullMatrixMaxEnt.evidence`` /
:func:`full_matrix_log_probability` (``mxe_fullmatrix_logdet``), after ``run()``: the classic and Bryan choices
of alpha, the number of good data and the evidence, for the same jobs.  The other result-taking methods of the scalar worker
(samples, diagnostics, response, resampling, bootstrap, model scans, bin checks) are refused, not forwarded.

alpha is scaled by n_tau, the number of data of ONE matrix element (``scale_alpha='Ndata'``): block-diagonal data then
decouple into exactly the ``DiagonalMaxEnt`` problems at the same mesh alpha.
"""

from datetime import datetime

import numpy as np

from . import device as _dev
from . import kernels
from .analyzers import BryanAnalyzer, ClassicAnalyzer
from .maxent_result import MaxEntResult
from .tau_maxent import TauMaxEnt

MAX_M = _dev.FULLMATRIX_MAX_M
MAX_NS = _dev.FULLMATRIX_MAX_NS
RESULT_KEYS = ('u', 'H', 'chi2', 'S', 'Q', 'n_iter', 'converged', 'alpha', 'ms')


def hermitian_basis(M, use_complex):
    """the orthonormal basis E_p (P, M, M) of the Hermitian M x M matrices in the order of the device: the diagonal units,
    (e_ab + e_ba) / sqrt 2 for a < b in row order, then (``use_complex``) i (e_ab - e_ba) / sqrt 2; Tr E_p E_q = delta_pq"""
    E = np.zeros((_dev.fullmatrix_P(M, use_complex), M, M), dtype=complex)
    r = 1.0 / np.sqrt(2.0)
    pairs = [(a, b) for a in range(M) for b in range(a + 1, M)]
    for a in range(M):
        E[a, a, a] = 1.0
    for k, (a, b) in enumerate(pairs):
        E[M + k, a, b] = E[M + k, b, a] = r
        if use_complex:
            E[M + len(pairs) + k, a, b] = 1.0j * r
            E[M + len(pairs) + k, b, a] = -1.0j * r
    return E


def _check_G(G, use_complex, what):
    G = np.asarray(G)
    if G.ndim != 3 or G.shape[0] != G.shape[1] or G.dtype.kind not in 'biufc':
        raise ValueError('%s: G must be numeric of shape (M, M, n); got %s' % (what, G.shape,))
    if G.shape[0] > MAX_M:
        raise ValueError('%s: a %d x %d matrix; at most %d x %d is supported' % (what, G.shape[0], G.shape[0], MAX_M, MAX_M))
    if not np.all(np.isfinite(G)):
        raise ValueError('%s: G is not finite' % what)
    if np.iscomplexobj(G) and not use_complex:
        if np.any(G.imag != 0.0):
            raise ValueError('%s: G is complex; construct FullMatrixMaxEnt(use_complex=True)' % what)
        G = G.real
    return np.array(G, dtype=complex if use_complex else float)


def _check_hermitian(G, err, what):
    """G_ij = conj(G_ji) within the error: |G_ij - conj(G_ji)| <= 4 sqrt(2) err at every point; ``err``: a scalar, one
    value per point, or (M, M, n), one per element and point"""
    asym = np.abs(G - np.conj(np.swapaxes(G, 0, 1)))
    bound = np.broadcast_to(4.0 * np.sqrt(2.0) * np.asarray(err, dtype=float) * np.ones(G.shape[-1]), asym.shape)
    if np.any(asym > bound):
        i, j, k = (int(x) for x in np.argwhere(asym > bound)[0])
        raise ValueError('%s: G is not Hermitian within its error: |G[%d, %d] - conj(G[%d, %d])| = %.3g at point %d (error %.3g)'
                         % (what, i, j, j, i, asym[i, j, k], k, bound[i, j, k] / (4.0 * np.sqrt(2.0))))


def whiten(U, S, V, err):
    """(U^, c, V', Q) of the whitened problem diag(1 / err) U S = U^ diag(c) Q^T, V' = V Q; for one error for all
    points nothing is rotated: U^ = U, c = S / err, Q = None"""
    err = np.asarray(err, dtype=float)
    if err.ndim == 0 or np.all(err == err.flat[0]):
        return U, S / float(err.flat[0]), V, None
    Uh, c, Qt = np.linalg.svd((U * S) / err[:, None], full_matrices=False)
    return Uh, c, np.dot(V, Qt.T), Qt.T


def component_errors(err, M, use_complex, n=None):
    """The error bars of the Hermitian components from those of the matrix elements.  ``err``: sigma_ab of shape (M, M) or
    sigma_ab(t) of shape (M, M, n), positive, finite and symmetric, err[a, b] == err[b, a]: the standard deviation of the
    real and of the imaginary part of the symmetrised G_ab(t).  Returns (P, n) in the order of :func:`hermitian_basis`
    ((P, 1) for an (M, M) input when ``n`` is not given): sigma_aa for the diagonal units, sigma_ab for BOTH the symmetric
    and the antisymmetric component of a pair a < b (the sqrt 2 of the basis cancels), so that the Frobenius misfit
    sum_ab sum_t |G_ab - (K H)_ab|^2 / sigma_ab^2 is sum_p sum_t (g_p - K h_p)_t^2 / sigma_p(t)^2."""
    e = np.asarray(err)
    M = int(M)
    if e.dtype.kind not in 'biuf' or e.ndim not in (2, 3) or e.shape[:2] != (M, M) or (e.ndim == 3 and e.shape[2] < 1):
        raise ValueError('component_errors: the element errors must be real of shape (%d, %d) or (%d, %d, n); got %s %s'
                         % (M, M, M, M, e.dtype, e.shape))
    e = np.array(e, dtype=float)
    if e.ndim == 2:
        e = e[:, :, None]
    if n is not None:
        if e.shape[2] not in (1, int(n)):
            raise ValueError('component_errors: %d data points, but the element errors have shape %s' % (n, np.shape(err)))
        e = np.broadcast_to(e, (M, M, int(n)))
    if not (np.all(np.isfinite(e)) and np.all(e > 0)):
        raise ValueError('component_errors: the element errors must be positive and finite')
    if not np.array_equal(e, np.swapaxes(e, 0, 1)):
        raise ValueError('component_errors: the element errors must be symmetric, err[a, b] == err[b, a]')
    pairs = [(a, b) for a in range(M) for b in range(a + 1, M)]
    rows = [e[a, a] for a in range(M)] + [e[a, b] for a, b in pairs] * (2 if use_complex else 1)
    return np.array(rows, dtype=float)


def whiten_components(U, S, errp):
    """The whitened problem of every component: diag(1 / sigma_p) U S = Q^_p R_p (thin QR), A_p = R_p^T R_p.  ``errp``:
    (P, n) or (P, 1) from :func:`component_errors`.  Returns ``R`` (P, n_s, n_s), ``A`` (P, n_s, n_s), ``Qh`` (P, n, n_s).
    V is not rotated: rho_p = R_p V^T H_p - Qh_p^T (G_p / sigma_p).  Components with the same errors share one
    factorisation (the same bits)."""
    U, S = np.asarray(U, dtype=float), np.asarray(S, dtype=float)
    n, n_s = U.shape
    if n < n_s:
        raise ValueError('whiten_components: U must be (n_data, n_s) with n_data >= n_s; got %s' % (U.shape,))
    errp = np.asarray(errp, dtype=float)
    if errp.ndim != 2 or errp.shape[1] not in (1, n):
        raise ValueError('whiten_components: the component errors must be (P, %d) or (P, 1); got %s' % (n, errp.shape))
    P = errp.shape[0]
    R, Qh = np.empty((P, n_s, n_s)), np.empty((P, n, n_s))
    done = {}
    for p in range(P):
        key = errp[p].tobytes()
        if key not in done:
            done[key] = np.linalg.qr((U * S) / (errp[p] * np.ones(n))[:, None])
        Qh[p], R[p] = done[key]
    return R, np.einsum('pks,pkt->pst', R, R), Qh


def full_matrix_continue(G_batch, U, S, V, D, alpha, err=None, use_complex=False, maxiter=1000, tol_h=1e-9, u0=None, device=0,
                         element_err=None):
    """The batch behind :class:`FullMatrixMaxEnt`: every G of ``G_batch`` (n_prob, M, M, n_data) -- k-points, mock data sets,
    iterations of a self-consistency loop -- is continued as a whole matrix, one workgroup per problem in one launch of
    ``mxe_fullmatrix_solve``.  They share the truncated SVD ``U`` (n_data, n_s), ``S``, ``V`` (n_omega, n_s) of the kernel
    that maps H = A delta_omega to the data, the default model ``D`` (n_omega,; times delta omega), the mesh ``alpha``
    (already scaled by the number of data of one element) and ``err`` (a scalar or one value per data point).  ``u0``: the
    start of the first alpha, (n_prob, P, n_s) in the basis of ``V``.  A problem's bits do not depend on the batch.

    ``element_err`` in the place of ``err`` (giving both is an error): one error bar per matrix element, (M, M) or
    (M, M, n_data), symmetric (:func:`component_errors`).  The job then always runs on ``mxe_fullmatrix_solve_metric``, also
    when all errors are equal; ``V`` is never rotated, so ``u`` and ``u0`` are in the basis of ``V`` as given; everything
    below holds unchanged.

    Returns a dict: ``u`` (n_prob, n_alpha, P, n_s), the coordinates of Gamma = log(H / D) in the basis of ``V`` and of
    :func:`hermitian_basis`; ``H`` (n_prob, M, M, n_alpha, n_omega), complex with ``use_complex``, exactly Hermitian and
    positive semi-definite; ``chi2``, ``S``, ``Q`` (n_prob, n_alpha), one cost per matrix; ``n_iter``, ``converged``;
    ``alpha``; ``ms``, the device time of the kernel.

    ``maxiter`` bounds the trial points of one alpha -- full steps and halved steps alike; ``n_iter`` counts them -- and an
    alpha that uses them up returns the last accepted point with ``converged`` False.  With a start ``u0`` this shows single
    steps of the iteration (tested contract, tests/test_gpu_fullmatrix_steps.py), delta being the solution of J delta = F
    at u0 with the undamped J of the first alpha:

    * ``maxiter=1``, the full step does not raise Q: ``u`` = u0 - delta, ``n_iter`` 1;
    * ``maxiter=1``, the full step raises Q: there is no trial point left for a halved step, ``u`` is u0 bit for bit,
      ``n_iter`` 1, ``converged`` False, and ``H``, ``chi2``, ``S``, ``Q`` are those of u0;
    * ``maxiter=2``, the full step raises Q and half of it does not: ``u`` = u0 - delta / 2, ``n_iter`` 2, ``converged``
      False (a halved step never ends an alpha)."""
    G = np.asarray(G_batch)
    if G.ndim != 4:
        raise ValueError('full_matrix_continue: G_batch must be (n_prob, M, M, n_data); got %s' % (G.shape,))
    G = np.stack([_check_G(g, use_complex, 'full_matrix_continue') for g in G])
    U, S, V, D = (np.asarray(x, dtype=float) for x in (U, S, V, D))
    M, n = G.shape[1], G.shape[-1]
    if U.ndim != 2 or U.shape[0] != n or S.shape != (U.shape[1],) or V.ndim != 2 or V.shape[1] != U.shape[1]:
        raise ValueError('full_matrix_continue: U must be (n_data, n_s), S (n_s,), V (n_omega, n_s); got %s, %s, %s for %d data'
                         % (U.shape, S.shape, V.shape, n))
    if len(S) > MAX_NS:
        raise ValueError('full_matrix_continue: %d singular values; at most %d are supported (the Newton matrix has order '
                         'n_s x %d): cut the singular space with reduce_singular_space' % (len(S), MAX_NS, _dev.fullmatrix_P(M, use_complex)))
    if D.shape != (V.shape[0],):
        raise NotImplementedError('full_matrix_continue: the default model must be one D(omega) of shape (%d,), shared by the '
                                  'diagonal elements; a matrix-valued model is not supported; got %s' % (V.shape[0], D.shape))
    if element_err is not None:
        if err is not None:
            raise ValueError('full_matrix_continue: give err (one error for all matrix elements) or element_err (one per '
                             'element), not both')
        errp = component_errors(element_err, M, use_complex, n)            # (P, n)
        sigma = np.broadcast_to(np.asarray(element_err, dtype=float).reshape(M, M, -1), (M, M, n))
        for g in G:
            _check_hermitian(g, sigma, 'full_matrix_continue')
        G = 0.5 * (G + np.conj(np.swapaxes(G, 1, 2)))
        Gw = np.einsum('pba,nabt->npt', hermitian_basis(M, use_complex), G).real / errp
        Rm, Am, Qh = whiten_components(U, S, errp)
        ghat = np.einsum('pts,npt->nps', Qh, Gw)                           # (n_prob, P, n_s)
        cperp = np.maximum(np.sum(Gw ** 2, axis=(1, 2)) - np.sum(ghat ** 2, axis=(1, 2)), 0.0)
        t = {}
        out = _dev.fullmatrix_solve_metric(V, Rm, Am, D, alpha, ghat, cperp, M, use_complex, u0=u0, maxiter=maxiter,
                                           tol_h=tol_h, device=device, timing=t)
        out['alpha'] = np.array(alpha, dtype=float)
        out['ms'] = t.get('ms', 0.0)
        return out
    if err is None:
        raise ValueError('full_matrix_continue: no error; give err or element_err')
    err = np.asarray(err, dtype=float)
    if err.ndim > 1 or (err.ndim == 1 and err.shape != (n,)):
        raise ValueError('full_matrix_continue: one error for all data or one per data point, shared by all matrix elements; '
                         'per-element errors are not supported here (use element_err=); got shape %s' % (err.shape,))
    if not (np.all(np.isfinite(err)) and np.all(err > 0)):
        raise ValueError('full_matrix_continue: the error must be positive and finite')
    for g in G:
        _check_hermitian(g, err, 'full_matrix_continue')
    G = 0.5 * (G + np.conj(np.swapaxes(G, 1, 2)))
    E = hermitian_basis(M, use_complex)
    Gp = np.einsum('pba,nabt->npt', E, G).real                  # (n_prob, P, n_data): Tr(E_p G)
    Uh, c, Vw, Q = whiten(U, S, V, err)
    Gw = Gp / err
    ghat = np.dot(Gw, Uh)                                       # (n_prob, P, n_s)
    cperp = np.maximum(np.sum(Gw ** 2, axis=(1, 2)) - np.sum(ghat ** 2, axis=(1, 2)), 0.0)
    if u0 is not None and Q is not None:
        u0 = np.dot(np.asarray(u0, dtype=float), Q)             # u' = Q^T u
    t = {}
    out = _dev.fullmatrix_solve(Vw, c, D, alpha, ghat, cperp, M, use_complex, u0=u0, maxiter=maxiter, tol_h=tol_h,
                                device=device, timing=t)
    if Q is not None:
        out['u'] = np.dot(out['u'], Q.T)
    out['alpha'] = np.array(alpha, dtype=float)
    out['ms'] = t.get('ms', 0.0)
    return out


# ---- posterior error bars ------------------------------------------------------------------------------------

def functional_coordinates(functionals, M, use_complex, n_omega):
    """The coordinates f_p,i = Tr(E_p F_i) (n_f, P, n_omega) of the weights ``functionals``, (n_f, M, M, n_omega) or
    (M, M, n_omega), Hermitian at every omega; x = sum_i Tr(F_i H_i) = sum_p,i f_p,i h_p,i.  ValueError for anything else;
    complex weights need ``use_complex``."""
    F = np.asarray(functionals)
    if F.dtype.kind not in 'biufc':
        raise ValueError('functionals: numbers are needed, got %s' % F.dtype)
    if F.ndim == 3:
        F = F[None]
    if F.ndim != 4 or F.shape[1:] != (M, M, n_omega):
        raise ValueError('functionals: shape (n_f, %d, %d, %d) or (%d, %d, %d) is needed, got %s'
                         % (M, M, n_omega, M, M, n_omega, np.shape(functionals)))
    if not np.all(np.isfinite(F)):
        raise ValueError('functionals hold values that are not finite')
    if np.iscomplexobj(F) and not use_complex and np.any(F.imag != 0.0):
        raise ValueError('functionals are complex; construct FullMatrixMaxEnt(use_complex=True)')
    F = np.array(F, dtype=complex)
    asym = np.abs(F - np.conj(np.swapaxes(F, 1, 2)))
    if np.any(asym > 8.0 * np.finfo(float).eps * max(1.0, float(np.max(np.abs(F))) if F.size else 1.0)):
        n, a, b, i = (int(x) for x in np.argwhere(asym == asym.max())[0])
        raise ValueError('functionals: weight %d is not Hermitian at point %d: |F[%d, %d] - conj(F[%d, %d])| = %.3g'
                         % (n, i, a, b, b, a, asym[n, a, b, i]))
    return np.ascontiguousarray(np.einsum('pba,nabi->npi', hermitian_basis(M, use_complex), F).real)


def window_coordinates(omega, windows, M, use_complex):
    """The functionals of the windows ``[(lo, hi), ...]`` as coordinates (n_win (P + 1), P, n_omega): per window the P
    coordinate functionals sum_{i in window} h_p,i, p in the order of :func:`hermitian_basis`, then the trace
    sum_{i in window} Tr H_i"""
    from .posterior import window_rows
    rows = window_rows(omega, windows)                           # (n_win, n_omega)
    P = _dev.fullmatrix_P(M, use_complex)
    f = np.zeros((len(rows), P + 1, P, rows.shape[1]))
    for p in range(P):
        f[:, p, p, :] = rows
    for a in range(M):
        f[:, P, a, :] = rows
    return f.reshape(len(rows) * (P + 1), P, rows.shape[1])


def elements_of_coordinates(x, M, use_complex):
    """(re, im), each (..., M, M): the matrix sum_p x_p E_p of coordinates ``x`` (..., P): re[a, a] = x_a and, for the pair
    p of a < b, re[a, b] = re[b, a] = x_p / sqrt 2, im[a, b] = -im[b, a] = x_p' / sqrt 2 (p' the antisymmetric partner;
    zero without ``use_complex``)"""
    x = np.asarray(x, dtype=float)
    re, im = np.zeros(x.shape[:-1] + (M, M)), np.zeros(x.shape[:-1] + (M, M))
    pairs = [(a, b) for a in range(M) for b in range(a + 1, M)]
    for a in range(M):
        re[..., a, a] = x[..., a]
    for k, (a, b) in enumerate(pairs):
        re[..., a, b] = re[..., b, a] = x[..., M + k] / np.sqrt(2.0)
        if use_complex:
            im[..., a, b] = x[..., M + len(pairs) + k] / np.sqrt(2.0)
            im[..., b, a] = -im[..., a, b]
    return re, im


def element_errors_of_coordinates(var, M, use_complex):
    """(err_re, err_im), each (..., M, M): the standard deviations of the real and of the imaginary part of the matrix
    elements from the variances ``var`` (..., P) of its coordinates: sqrt(var_a) on the diagonal, sqrt(var_p / 2) for both
    elements of a pair; err_im is symmetric, zero on the diagonal and zero without ``use_complex``"""
    re, im = elements_of_coordinates(np.sqrt(np.asarray(var, dtype=float)), M, use_complex)
    return re, np.abs(im)


def _check_minimisers(what, u, U, S, V, D, alpha, err, use_complex):
    """the shape checks of what works on the minimisers u (n_prob, n_alpha, P, n_s) of :func:`full_matrix_continue`;
    returns the arrays as float, alpha one-dimensional, and M"""
    u = np.asarray(u, dtype=float)
    U, S, V, D = (np.asarray(x, dtype=float) for x in (U, S, V, D))
    alpha = np.atleast_1d(np.asarray(alpha, dtype=float))
    if u.ndim != 4 or alpha.ndim != 1 or u.shape[1] != len(alpha):
        raise ValueError('%s: u must be (n_prob, n_alpha, P, n_s) with one alpha per row; got %s and '
                         '%d alphas' % (what, u.shape, alpha.size))
    n_prob, n_alpha, P, n_s = u.shape
    Ms = [m for m in range(1, MAX_M + 1) if _dev.fullmatrix_P(m, use_complex) == P]
    if not Ms:
        raise ValueError('%s: %d components are no %s matrix of at most %d x %d'
                         % (what, P, 'complex Hermitian' if use_complex else 'real symmetric', MAX_M, MAX_M))
    if U.ndim != 2 or S.shape != (U.shape[1],) or V.ndim != 2 or V.shape[1] != U.shape[1] or n_s != U.shape[1]:
        raise ValueError('%s: U must be (n_data, n_s), S (n_s,), V (n_omega, n_s), u (..., n_s); got '
                         '%s, %s, %s, %s' % (what, U.shape, S.shape, V.shape, u.shape))
    if n_s > MAX_NS:
        raise ValueError('%s: %d singular values; at most %d are supported: cut the singular space '
                         'with reduce_singular_space' % (what, n_s, MAX_NS))
    n_omega = V.shape[0]
    if D.shape != (n_omega,):
        raise NotImplementedError('%s: the default model must be one D(omega) of shape (%d,); a '
                                  'matrix-valued model is not supported; got %s' % (what, n_omega, D.shape))
    err = np.asarray(err, dtype=float)
    if err.ndim > 1 or (err.ndim == 1 and err.shape != (U.shape[0],)):
        raise ValueError('%s: one error for all data or one per data point, shared by all matrix '
                         'elements; got shape %s' % (what, err.shape,))
    if not (np.all(np.isfinite(err)) and np.all(err > 0)):
        raise ValueError('%s: the error must be positive and finite' % what)
    return u, U, S, V, D, alpha, err, Ms[0]


def full_matrix_posterior_errors(u, U, S, V, D, alpha, err, use_complex=False, functionals=None, windows=None, omega=None,
                                 pointwise=False, device=0):
    """Posterior error bars of whole-matrix continuations with one error for all matrix elements, in the Gaussian
    approximation around the minimisers ``u`` (n_prob, n_alpha', P, n_s) of :func:`full_matrix_continue` at the scaled
    ``alpha`` (n_alpha',), on the device (``mxe_fullmatrix_posterior_var``, one workgroup per (problem, alpha)).
    ``U, S, V, D, err`` as there (with one error per data point u is rotated into the whitened basis exactly as there).

    ``functionals``: (n_f, M, M, n_omega) or (M, M, n_omega), Hermitian weights F on A delta_omega, x = sum_i Tr(F_i H_i);
    ``windows=[(lo, hi), ...]`` on the mesh ``omega``: the spectral weight of every matrix element and of the trace inside;
    ``pointwise``: the error of every A_ab(omega_i) (``omega``: a mesh with ``delta``, or the points) -- large and strongly
    correlated between neighbours: only integrated quantities have meaningful errors.

    Returns a dict, every array with (n_prob, n_alpha') in front: ``functional_value``, ``functional_err``,
    ``functional_prior_err`` (n_f); ``window_weight``, ``window_err``, ``window_prior_err`` (n_win, M, M), the integral of
    Re A_ab and its standard deviation, with ``use_complex`` also ``window_weight_imag``, ``window_err_imag``;
    ``window_trace``, ``window_trace_err``, ``window_trace_prior_err`` (n_win); ``A``, ``A_err``, ``A_prior_err`` (M, M,
    n_omega), ``A_err`` the standard deviation of Re A_ab(omega_i), with ``use_complex`` also ``A_err_imag`` (zero on the
    diagonal); ``alpha``; ``info`` (``kernel_ms``; ``nan_jobs``: the (problem, alpha) pairs whose u or H is not finite or
    whose curvature is not positive definite: they are NaN).  The prior errors are what the entropy alone would leave."""
    u, U, S, V, D, alpha, err, M = _check_minimisers('full_matrix_posterior_errors', u, U, S, V, D, alpha, err, use_complex)
    n_prob, n_alpha, P, n_s = u.shape
    n_omega = V.shape[0]
    n_win = 0 if windows is None else len(windows)
    if (n_win or pointwise) and omega is None:
        raise ValueError('full_matrix_posterior_errors: windows and pointwise need the mesh omega')
    rows = []
    if n_win:
        if len(np.asarray(omega, dtype=float)) != n_omega:
            raise ValueError('full_matrix_posterior_errors: omega has %d points, V %d' % (len(np.asarray(omega)), n_omega))
        rows.append(window_coordinates(omega, windows, M, use_complex))
    n_fun = 0
    if functionals is not None:
        rows.append(functional_coordinates(functionals, M, use_complex, n_omega))
        n_fun = len(rows[-1])
    if not rows and not pointwise:
        raise ValueError('nothing to compute: give windows=, functionals= or pointwise=True')
    F = np.concatenate(rows) if rows else None
    _, c, Vw, Q = whiten(U, S, V, err)
    uw = u if Q is None else np.dot(u, Q)                       # u' = Q^T u
    t = {}
    out = _dev.fullmatrix_posterior_var(Vw, c, D, np.tile(alpha, n_prob), uw.reshape(n_prob * n_alpha, P, n_s), M, use_complex,
                                        F=F, want_diag=pointwise, device=device, timing=t)
    lead = (n_prob, n_alpha)
    res = dict(alpha=np.array(alpha))
    nan = np.zeros(lead, dtype=bool)
    if F is not None:
        val, var, pri = (out[k].reshape(lead + (-1,)) for k in ('value', 'var', 'prior'))
        nan |= np.any(np.isnan(var), axis=-1)
        if n_win:
            nw1 = P + 1
            wv, wvar, wpri = (x[..., :n_win * nw1].reshape(lead + (n_win, nw1)) for x in (val, var, pri))
            res['window_weight'], wim = elements_of_coordinates(wv[..., :P], M, use_complex)
            res['window_err'], eim = element_errors_of_coordinates(wvar[..., :P], M, use_complex)
            res['window_prior_err'] = element_errors_of_coordinates(wpri[..., :P], M, use_complex)[0]
            if use_complex:
                res['window_weight_imag'], res['window_err_imag'] = wim, eim
            res['window_trace'] = wv[..., P]
            res['window_trace_err'], res['window_trace_prior_err'] = np.sqrt(wvar[..., P]), np.sqrt(wpri[..., P])
        if n_fun:
            o = n_win * (P + 1)
            res['functional_value'] = val[..., o:]
            res['functional_err'], res['functional_prior_err'] = np.sqrt(var[..., o:]), np.sqrt(pri[..., o:])
    if pointwise:
        delta = np.asarray(omega.delta, dtype=float) if hasattr(omega, 'delta') else None
        if delta is None:
            from .analyzers import get_delta
            delta = get_delta(np.asarray(omega, dtype=float))
        if delta.shape != (n_omega,):
            raise ValueError('full_matrix_posterior_errors: omega has %d points, V %d' % (len(delta), n_omega))
        h, dv, dp = (np.moveaxis(out[k].reshape(lead + (P, n_omega)), -2, -1) for k in ('h', 'diag_var', 'diag_prior'))
        nan |= np.any(np.isnan(dv), axis=(-2, -1))
        to_A = lambda x: np.moveaxis(x, -3, -1) / delta                       # (..., n_omega, M, M) -> (..., M, M, n_omega)
        re, im = elements_of_coordinates(h, M, use_complex)
        res['A'] = to_A(re + 1.0j * im) if use_complex else to_A(re)
        ere, eim = element_errors_of_coordinates(dv, M, use_complex)
        res['A_err'] = to_A(ere)
        res['A_prior_err'] = to_A(element_errors_of_coordinates(dp, M, use_complex)[0])
        if use_complex:
            res['A_err_imag'] = to_A(eim)
    res['info'] = dict(kernel_ms=t.get('ms', 0.0), kernel='mxe_fullmatrix_posterior_var',
                       nan_jobs=[(int(a), int(b)) for a, b in np.argwhere(nan)])
    return res


# ---- the evidence of alpha -----------------------------------------------------------------------------------

def full_matrix_log_probability(u, U, S, V, D, alpha, err, Q, use_complex=False, probability=None, device=0, S_entropy=None):
    """log p(alpha | G) of whole-matrix continuations with one error for all matrix elements, in the Gaussian approximation
    around the minimisers ``u`` (n_prob, n_alpha, P, n_s) of :func:`full_matrix_continue` at the scaled ``alpha`` (n_alpha,),
    on the device (``mxe_fullmatrix_logdet``, one workgroup per (problem, alpha)).  ``U, S, V, D, err`` as there
    (with one error per data point u is rotated into the whitened basis exactly as there); ``Q`` (n_prob, n_alpha), the cost
    at the minimisers as :func:`full_matrix_continue` returns it.  ``probability``: a :class:`NormalLogProbability` (its
    ``log_norm_S`` and ``log_prior_alpha`` are honoured, ``log_norm_S`` with P n_omega unknowns); ``S_entropy``
    (n_prob, n_alpha), optional: the entropy at the minimisers, for ``classic_ratio``.

    Returns a dict: ``logdet`` (n_prob, n_alpha), log det(I + c W c / alpha) of order P n_s; ``n_good``, the number of good
    data tr(c W c (alpha I + c W c)^-1); ``log_probability`` = -logdet / 2 - Q - log alpha; ``alpha_index_classic``
    (n_prob,), its maximum (-1 where no alpha is finite); ``weights`` (n_prob, n_alpha), exp(log p - max) normalised to sum
    one over the finite entries (0 for the others): the default rule of ``BryanAnalyzer``; ``classic_ratio`` =
    -2 alpha S / N_g, one at the classic alpha (with ``S_entropy``); ``log_evidence`` (n_prob,) = log sum_k p_k |delta alpha_k|
    over the finite entries with the measure of ``model_scan.log_measure``; ``alpha_at_edge`` (n_prob,): the maximum sits on
    the first or the last alpha, so the mesh may not hold it; ``alpha``; ``info``: ``kernel``, ``kernel_ms``, ``nan_jobs``, the
    (problem, alpha) pairs whose u or H is not finite or whose curvature is not positive definite (they are NaN).

    ``log_probability`` lacks the constants that do not depend on alpha, and the evidence those that depend on the data, the
    error and the meshes: two values of ``log_evidence`` are comparable only between calls on the same data, error, omega
    mesh and alpha mesh -- between default models, say."""
    from .model_scan import log_measure
    from .probabilities import NormalLogProbability
    what = 'full_matrix_log_probability'
    u, U, S, V, D, alpha, err, M = _check_minimisers(what, u, U, S, V, D, alpha, err, use_complex)
    n_prob, n_alpha, P, n_s = u.shape
    Q = np.asarray(Q, dtype=float)
    if Q.shape != (n_prob, n_alpha):
        raise ValueError('%s: Q must be (n_prob, n_alpha) = (%d, %d); got %s' % (what, n_prob, n_alpha, Q.shape))
    if S_entropy is not None:
        S_entropy = np.asarray(S_entropy, dtype=float)
        if S_entropy.shape != (n_prob, n_alpha):
            raise ValueError('%s: S_entropy must be (n_prob, n_alpha) = (%d, %d); got %s' % (what, n_prob, n_alpha, S_entropy.shape))
    if not (np.all(np.isfinite(alpha)) and np.all(alpha > 0)):
        raise ValueError('%s: alpha must be positive and finite' % what)
    measure = log_measure(alpha)
    _, c, Vw, Qr = whiten(U, S, V, err)
    uw = u if Qr is None else np.dot(u, Qr)                     # u' = Q^T u
    t = {}
    out = _dev.fullmatrix_logdet(Vw, c, D, np.tile(alpha, n_prob), uw.reshape(n_prob * n_alpha, P, n_s), M, use_complex,
                                 want_ngood=True, device=device, timing=t)
    logdet, n_good = out['logdet'].reshape(n_prob, n_alpha), out['n_good'].reshape(n_prob, n_alpha)
    prob = NormalLogProbability() if probability is None else probability
    logp = np.stack([np.asarray(prob.from_logdet(logdet[n], alpha, Q[n], P * V.shape[0]), dtype=float) for n in range(n_prob)])
    good = np.isfinite(logp)
    some = np.any(good, axis=1)
    masked = np.where(good, logp, -np.inf)
    top = np.where(some, np.max(masked, axis=1), 0.0)
    idx = np.where(some, np.argmax(masked, axis=1), -1)
    w = np.where(good, np.exp(masked - top[:, None]), 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        weights = np.where(some[:, None], w / np.sum(w, axis=1, keepdims=True), np.nan)
        log_ev = np.where(some, top + np.log(np.sum(np.where(good, np.exp(masked - top[:, None] + measure), 0.0), axis=1)), np.nan)
    res = dict(alpha=np.array(alpha), logdet=logdet, n_good=n_good, log_probability=logp, alpha_index_classic=idx,
               weights=weights, log_evidence=log_ev, alpha_at_edge=some & ((idx == 0) | (idx == n_alpha - 1)))
    if S_entropy is not None:
        with np.errstate(invalid='ignore', divide='ignore'):
            res['classic_ratio'] = -2.0 * alpha * S_entropy / n_good
    res['info'] = dict(kernel_ms=t.get('ms', 0.0), kernel='mxe_fullmatrix_logdet',
                       nan_jobs=[(int(a), int(b)) for a, b in np.argwhere(np.isnan(logdet))])
    return res


class FullMatrixResult(MaxEntResult):
    """the :class:`MaxEntResult` of a whole-matrix job: ``A`` and ``H`` are (M, M, n_alpha, n_omega), ``chi2``, ``S``, ``Q``
    (n_alpha,) belong to the matrix, ``v`` holds u (n_alpha, P, n_s); an analyzer picks one alpha for the whole matrix and
    its ``A_out`` is (M, M, n_omega)"""

    def element_row(self, name, matrix_element, idx):
        arr = np.asarray(self.element_array(name, matrix_element))
        if name in ('A', 'H'):
            return arr[:, :, int(idx)]
        return arr[idx]

    def attach_probability(self, log_probability, analyzer_results):
        """write ``log_probability`` (n_alpha,) into ``probability`` and add ``analyzer_results`` (:class:`AnalyzerResult`
        objects with a ``name``) beside those of ``run()``; the default analyzer stays what it was"""
        self._records[None]['probability'] = np.array(log_probability, dtype=float)
        for ar in analyzer_results:
            ar.maxent_result = self
            self._analysis.setdefault(None, {})[ar['name']] = ar
        self._cache = dict()


_REFUSED = dict(set_G_iw_data='Matsubara data', set_G_iw='Matsubara data', set_chi_tau_data='bosonic data',
                set_chi_iw_data='bosonic data', set_cov='a covariance matrix', set_cov_file='a covariance matrix',
                set_G_tau_bins='Monte Carlo bins', set_G_iw_bins='Monte Carlo bins', set_G_l_bins='Monte Carlo bins',
                set_G_tau='TRIQS Green functions (use set_G_tau_data)', set_G_tau_file='a file of one element (use set_G_tau_data)',
                # what the scalar worker computes from a result has no whole-matrix meaning yet (posterior_errors has)
                posterior_samples='posterior sampling of the whole matrix', fit_diagnostics='the hat matrix of the whole matrix',
                resolution='the linear response of the whole matrix', default_model_response='the linear response of the whole matrix',
                resample_errors='resampling of Monte Carlo bins', parametric_bootstrap='the parametric bootstrap',
                default_model_scan='a default-model scan (it needs the evidence)', check_bins='Monte Carlo bins')


class FullMatrixMaxEnt(object):
    """Continue a matrix-valued G(tau) as ONE unknown, the Hermitian positive semi-definite matrix A(omega).  See the
    module's docstring for what the first version takes.  ``omega``, ``alpha_mesh``, ``D``, ``reduce_singular_space``,
    ``minimizer`` (its ``maxiter`` bounds the trial points per alpha), ``analyzers``, ``scale_alpha`` and the other
    attributes of :class:`TauMaxEnt` are forwarded to ``self.maxent``, as ``ElementwiseMaxEnt`` forwards to its workers.
    ``use_complex``: the matrix is complex Hermitian (P = M^2 unknown functions) instead of real symmetric
    (P = M (M + 1) / 2).  ``tol_h``: the stopping tolerance, the first-order relative change of H of an undamped step."""

    maxent = None

    def __init__(self, use_complex=False, tol_h=1e-9, **kwargs):
        if kwargs.get('probability') is not None:
            raise NotImplementedError('FullMatrixMaxEnt: probability= needs the log-determinant of the whole-matrix problem, '
                                      'which is not implemented')
        if isinstance(kwargs.get('cost_function'), str) and kwargs['cost_function'].lower() != 'normal':
            raise NotImplementedError('FullMatrixMaxEnt: the cost function is the matrix entropy; cost_function=%r is not '
                                      'supported' % (kwargs['cost_function'],))
        object.__setattr__(self, 'maxent', TauMaxEnt(**kwargs))
        object.__setattr__(self, 'use_complex', bool(use_complex))
        object.__setattr__(self, 'tol_h', float(tol_h))
        object.__setattr__(self, 'G_mat', None)
        object.__setattr__(self, 'element_err', None)
        object.__setattr__(self, 'maxent_result', None)
        object.__setattr__(self, 'last_info', None)

    def __getattr__(self, name):
        if name in _REFUSED:
            def refuse(*args, **kwargs):
                raise NotImplementedError('FullMatrixMaxEnt: %s not supported yet (G(tau) and Legendre data with one '
                                          'error for all matrix elements, or one per element, are)' % ('%s: %s is' % (name, _REFUSED[name])))
            return refuse
        return getattr(object.__getattribute__(self, 'maxent'), name)

    def __setattr__(self, name, value):
        if name in self.__dict__ or not hasattr(self.maxent, name):
            object.__setattr__(self, name, value)
        else:
            setattr(self.maxent, name, value)

    # ---- data ---------------------------------------------------------------------------------------------------------
    def _adopt(self, G):
        object.__setattr__(self, 'G_mat', G)
        self.maxent.G = np.array(G[0, 0].real, dtype=float)       # (the worker's own data: what scale_alpha counts)
        self.maxent._adopt_data()

    def set_G_tau_data(self, tau, G):
        """G(tau) of shape (M, M, n_tau), M <= 4, Hermitian at every tau within the error (checked in ``run()``, when the
        error is known); complex data need ``use_complex=True``"""
        G = _check_G(G, self.use_complex, 'set_G_tau_data')
        tau = np.asarray(tau, dtype=float)
        if tau.ndim != 1 or len(tau) != G.shape[-1]:
            raise ValueError("set_G_tau_data: tau and G don't have the same dimension")
        self.maxent._use_kernel(kernels.TauKernel, tau)
        self._adopt(G)

    def set_G_l_data(self, G_l, beta, l=None):
        """Legendre coefficients of shape (M, M, n_l) (:meth:`TauMaxEnt.set_G_l_data` for the normalisation and ``l``)"""
        G = _check_G(G_l, self.use_complex, 'set_G_l_data')
        self.maxent._use_kernel(kernels.LegendreKernel, self.maxent._legendre_orders(l, G.shape[-1]), beta=beta)
        self._adopt(G)

    def set_error(self, error):
        """one standard deviation for all data or one per data point, shared by all matrix elements"""
        if np.ndim(error) > 1:
            raise ValueError('FullMatrixMaxEnt.set_error: one error for all matrix elements (a scalar or one value per data '
                             'point); per-element errors are not supported here (use set_element_errors); got shape %s'
                             % (np.shape(error),))
        if self.G_mat is None:
            raise ValueError('FullMatrixMaxEnt.set_error: set the data first')
        self.maxent.set_error(error)
        object.__setattr__(self, 'element_err', None)

    def set_element_errors(self, error):
        """one standard deviation per matrix element, (M, M) or (M, M, n) with error[a, b] == error[b, a]: that of the real
        and of the imaginary part of the symmetrised G_ab (:func:`component_errors`).  Replaces an earlier ``set_error``, as
        a later ``set_error`` replaces this.  The job runs on ``mxe_fullmatrix_solve_metric``."""
        if self.G_mat is None:
            raise ValueError('FullMatrixMaxEnt.set_element_errors: set the data first')
        M, n = self.G_mat.shape[0], self.G_mat.shape[-1]
        component_errors(error, M, self.use_complex, n)                      # (every refusal)
        e = np.array(np.broadcast_to(np.asarray(error, dtype=float).reshape(M, M, -1), (M, M, n)))
        self.maxent.set_error(np.array(e[0, 0]))      # (the worker's own error: what scale_alpha and _job look at)
        object.__setattr__(self, 'element_err', e)

    # ---- the job --------------------------------------------------------------------------------------------------------
    def _job(self):
        """the arrays of the present job, after every refusal"""
        w = self.maxent
        loop = w.maxent_loop
        if self.G_mat is None:
            raise ValueError('FullMatrixMaxEnt: no data; use set_G_tau_data or set_G_l_data')
        if loop.err is None:
            raise ValueError('FullMatrixMaxEnt: no error; use set_error')
        if loop.probability is not None or any(isinstance(a, (BryanAnalyzer, ClassicAnalyzer)) for a in loop.analyzers):
            raise NotImplementedError('FullMatrixMaxEnt: the probability-based analyzers (BryanAnalyzer, ClassicAnalyzer) and '
                                      'probability= need the log-determinant of the whole-matrix problem, which is not '
                                      'implemented; use LineFitAnalyzer, Chi2CurvatureAnalyzer or EntropyAnalyzer')
        K = w.K
        if hasattr(K, 'kernel') or type(loop.A_of_H).__name__ != 'IdentityA_of_H':
            raise NotImplementedError('FullMatrixMaxEnt: preblur is not supported')
        if getattr(K, 'setter_kind', 'tau') not in ('tau', 'legendre') or getattr(K, 'stacked', False):
            raise NotImplementedError('FullMatrixMaxEnt: only G(tau) and Legendre data are supported')
        if K.rotation is not None:
            raise NotImplementedError('FullMatrixMaxEnt: a covariance matrix (a rotated data space) is not supported')
        D = np.asarray(loop.D.D, dtype=float)
        if D.ndim != 1:
            raise NotImplementedError('FullMatrixMaxEnt: the default model must be one D(omega), shared by the diagonal '
                                      'elements; a matrix-valued model is not supported')
        K.reduce_singular_space(loop.reduce_singular_space)
        if len(K.S) > MAX_NS:
            raise ValueError('FullMatrixMaxEnt: %d singular values pass reduce_singular_space = %g; at most %d are supported '
                             '(the Newton matrix has order n_s x %d): raise reduce_singular_space'
                             % (len(K.S), loop.reduce_singular_space, MAX_NS, _dev.fullmatrix_P(self.G_mat.shape[0], self.use_complex)))
        scale = loop._alpha_scale()
        return dict(U=np.asarray(K.U, dtype=float), S=np.asarray(K.S, dtype=float), V=np.asarray(K.V, dtype=float), D=D,
                    alpha=np.asarray(loop.alpha_mesh, dtype=float) * scale,
                    err=None if self.element_err is not None else np.asarray(loop.err, dtype=float),
                    element_err=self.element_err,
                    maxiter=int(getattr(loop.minimizer, 'maxiter', 1000)))

    def run(self):
        """Continue the matrix; returns a :class:`MaxEntResult` (:class:`FullMatrixResult`): ``A`` and ``H`` (M, M, n_alpha,
        n_omega), complex with ``use_complex``; ``chi2``, ``S``, ``Q``, ``n_iter``, ``converged`` (n_alpha,), one cost for the
        whole matrix; ``v`` = u (n_alpha, P, n_s); the analyzers pick one alpha for the matrix, ``A_out`` is (M, M, n_omega)."""
        job = self._job()
        w = self.maxent
        loop = w.maxent_loop
        t0 = datetime.now()
        sol = full_matrix_continue(self.G_mat[None], job['U'], job['S'], job['V'], job['D'], job['alpha'], job['err'],
                                   use_complex=self.use_complex, maxiter=job['maxiter'], tol_h=self.tol_h,
                                   device=loop.device_id, element_err=job['element_err'])
        t1 = datetime.now()
        H = sol['H'][0]
        delta = np.asarray(w.omega.delta, dtype=float)
        A = H / delta
        X = len(job['alpha'])
        M = H.shape[0]
        G_rec = np.einsum('ti,abxi->abxt', np.asarray(w.K.K_delta, dtype=float), A)
        res = FullMatrixResult(matrix_structure=(M, M), element_wise=False, complex_elements=self.use_complex)
        rec = dict(alpha=job['alpha'], v=sol['u'][0], H=H, A=A, chi2=sol['chi2'][0], S=sol['S'][0], Q=sol['Q'][0],
                   G=np.array(self.G_mat), G_orig=np.array(self.G_mat), G_rec=G_rec,
                   data_variable=np.array(w.K.data_variable, dtype=float), omega=w.omega,
                   probability=np.full(X, np.nan), n_iter=sol['n_iter'][0], converged=sol['converged'][0],
                   run_times=((t1 - t0) / max(1, X),) * X)
        res.start_timing(time=t0)
        res.add_element_results(rec)
        res.end_timing(time=t1)
        if loop.analyzers:
            res._default_analyzer_name = loop.analyzers[0].name
        res.analyze(loop.analyzers)
        object.__setattr__(self, 'maxent_result', res)
        object.__setattr__(self, 'last_info', dict(kernel_ms=sol['ms'], n_iter=sol['n_iter'][0], converged=sol['converged'][0],
                                                      kernel='mxe_fullmatrix_solve' if job['element_err'] is None
                                                      else 'mxe_fullmatrix_solve_metric'))
        return res

    def posterior_errors(self, result=None, alpha=None, windows=None, functionals=None, pointwise=False):
        """Posterior error bars of the whole-matrix result (default: ``run()``) in the Gaussian approximation around the
        minimiser, on the device (:func:`full_matrix_posterior_errors`, which describes the keys).  ``alpha``:
        None -- the alpha of the default analyzer --, an analyzer name, an index into the alpha mesh, a sequence of indices or
        ``'all'`` (the last two keep an alpha axis in front); ``'bryan'`` is a ValueError: the whole-matrix problem has no
        probability.  ``windows=[(lo, hi), ...]``: the spectral weight of every matrix element, and of the trace, inside, with
        its error; ``functionals``: (n_f, M, M, n_omega) or (M, M, n_omega) Hermitian weights on A delta_omega;
        ``pointwise``: the error of every A_ab(omega_i).  The dict also holds ``alpha`` and ``alpha_index``, what was taken, and
        ``info``: ``kernel_ms``, the device time of the kernel, ``kernel``, and ``nan_rows``, the indices into the alpha mesh
        whose u or H is not finite or whose curvature is not positive definite (they are NaN; the name is that of
        ``TauMaxEnt.posterior_errors``, the plain function reports (problem, alpha) pairs as ``nan_jobs``).  A job with ``set_element_errors`` is refused with NotImplementedError."""
        from .posterior import choose_alpha
        if isinstance(alpha, str) and alpha == 'bryan':
            raise ValueError("FullMatrixMaxEnt.posterior_errors: alpha='bryan' needs the probability of alpha, which the "
                             'whole-matrix problem does not have')
        if self.element_err is not None:
            raise NotImplementedError('FullMatrixMaxEnt.posterior_errors: a job with set_element_errors (one error bar per '
                                      'matrix element) is not supported yet; use set_error')
        res = self.run() if result is None else result
        job = self._job()
        al = np.asarray(res.alpha, dtype=float)
        if al.shape != job['alpha'].shape or not np.allclose(al, job['alpha'], rtol=1e-12, atol=0.0):
            raise ValueError('FullMatrixMaxEnt.posterior_errors: the result was not made with the alpha mesh of this object')
        idx, how = choose_alpha(alpha, len(al), res.analyzer_results, res.default_analyzer_name)
        u = np.asarray(res.v, dtype=float)[idx]
        out = full_matrix_posterior_errors(u[None], job['U'], job['S'], job['V'], job['D'], al[idx], job['err'],
                                           use_complex=self.use_complex, functionals=functionals, windows=windows,
                                           omega=self.maxent.omega, pointwise=pointwise,
                                           device=self.maxent.maxent_loop.device_id)
        info = out.pop('info')
        out = dict((k, v[0] if k != 'alpha' else v) for k, v in out.items())
        out['alpha_index'] = np.array(idx)
        if how == 'one':
            out = dict((k, v[0]) for k, v in out.items())
        out['info'] = dict(kernel_ms=info['kernel_ms'], kernel=info['kernel'], nan_rows=[idx[b] for _, b in info['nan_jobs']])
        return out

    def evidence(self, result=None, attach=True):
        """log p(alpha | G) of the whole-matrix result (default: ``run()``) in the Gaussian approximation around the
        minimisers, on the device (:func:`full_matrix_log_probability`, which describes the keys): ``logdet``,
        ``n_good``, ``log_probability``, ``weights``, ``classic_ratio`` (n_alpha,), ``alpha_index_classic``, ``log_evidence``,
        ``alpha_at_edge``, ``alpha``; ``A_classic`` (M, M, n_omega), A at the maximum of the probability, and ``A_bryan`` =
        sum_k weights_k A[:, :, k, :]: a convex mixture of positive semi-definite matrices; ``info``: ``kernel``,
        ``kernel_ms`` and ``nan_rows``, the indices into the alpha mesh that are NaN.  ``run()`` itself still computes no
        probability and still refuses ``BryanAnalyzer``, ``ClassicAnalyzer`` and ``probability=``: this is the way to them.

        ``attach``: write ``log_probability`` into ``result.probability`` and add the entries ``'ClassicAnalyzer'`` (``name``,
        ``alpha_index``, ``A_out``, ``info``) and ``'BryanAnalyzer'`` (``name``, ``A_out``, ``info``) to
        ``result.analyzer_results``, so that ``result.get_A_out('ClassicAnalyzer')``, ``posterior_errors(result,
        alpha='ClassicAnalyzer')`` and ``positivity(result, alpha='BryanAnalyzer')`` work; the default analyzer stays what it
        was.  A job with ``set_element_errors`` is refused with NotImplementedError; a result of another alpha mesh is a
        ValueError, and so is a result whose probability is NaN at every alpha (there is no classic alpha and no weight to
        mix with: nothing is attached)."""
        from .analyzers import AnalyzerResult
        if self.element_err is not None:
            raise NotImplementedError('FullMatrixMaxEnt.evidence: a job with set_element_errors (one error bar per matrix '
                                      'element) is not supported yet; use set_error')
        res = self.run() if result is None else result
        job = self._job()
        al = np.asarray(res.alpha, dtype=float)
        if al.shape != job['alpha'].shape or not np.allclose(al, job['alpha'], rtol=1e-12, atol=0.0):
            raise ValueError('FullMatrixMaxEnt.evidence: the result was not made with the alpha mesh of this object')
        out = full_matrix_log_probability(np.asarray(res.v, dtype=float)[None], job['U'], job['S'], job['V'], job['D'], al,
                                          job['err'], np.asarray(res.Q, dtype=float)[None], use_complex=self.use_complex,
                                          device=self.maxent.maxent_loop.device_id,
                                          S_entropy=np.asarray(res.S, dtype=float)[None])
        info = out.pop('info')
        out = dict((k, v[0] if k != 'alpha' else v) for k, v in out.items())
        A = np.asarray(res.A)
        idx = int(out['alpha_index_classic'])
        if idx < 0:
            raise ValueError('FullMatrixMaxEnt.evidence: the probability is NaN at every alpha (u or H is not finite, or the '
                             'curvature is not positive definite)')
        out['A_classic'] = np.array(A[:, :, idx])
        sel = np.isfinite(out['log_probability'])                  # (a NaN row has the weight 0 and is not read)
        out['A_bryan'] = np.einsum('k,abki->abi', out['weights'][sel], A[:, :, sel])
        out['info'] = dict(kernel_ms=info['kernel_ms'], kernel=info['kernel'], nan_rows=[b for _, b in info['nan_jobs']])
        if attach:
            classic, bryan = AnalyzerResult(), AnalyzerResult()
            classic.update(name='ClassicAnalyzer', alpha_index=idx, A_out=out['A_classic'],
                           info='Ideal alpha (classic): {} (= index {} zero-based)'.format(al[idx], idx))
            bryan.update(name='BryanAnalyzer', A_out=out['A_bryan'],
                         info='Bryan analyzer: average of A weighted by probability calculated.')
            res.attach_probability(out['log_probability'], (classic, bryan))
        return out

    def positivity(self, result=None, alpha=None, floor=0.0, keep_vectors=False):
        """:func:`maxent_amd.positivity.matrix_positivity` of the result (default: ``run()``): ``alpha`` None -- ``A_out`` of
        the default analyzer --, an analyzer name, an index into the alpha mesh, or ``'all'``.  The dict also holds ``alpha``,
        what was taken."""
        from .positivity import matrix_positivity
        res = self.run() if result is None else result
        if isinstance(alpha, str) and alpha == 'all':
            A, which = np.asarray(res.A), 'all'
        elif alpha is None or isinstance(alpha, str):
            A = np.asarray(res.get_A_out(alpha))
            which = res.default_analyzer_name if alpha is None else alpha
        else:
            A, which = np.asarray(res.A)[:, :, int(alpha)], int(alpha)
        out = matrix_positivity(A, delta=np.asarray(self.maxent.omega.delta, dtype=float), floor=floor,
                                keep_vectors=keep_vectors, device=self.maxent.maxent_loop.device_id)
        out['alpha'] = which
        return out
