"""numpy truth of the posterior variances of the whole-matrix continuation, on ``fullmatrix_ref.Problem``
(``state``, ``L``, ``gram``).  Not a test, and not a port of anything: the reference has neither the solver nor error bars.

In the coordinates h_p,i = Tr(E_p H_i) the covariance of h around the minimiser is

    Gamma = (alpha L^-1 + (V c^2 V^T) (x) 1_P)^-1

(a) :func:`variances` -- the form the device uses, of order d = P n_s:
        B = alpha I + c W c = L_B L_B^T,   var(x) = (1 / alpha) [ sum_i f_i^T L_i f_i - |L_B^-1 y|^2 ],
        y_(p,s) = c_s sum_i V_is (L_i f_i)_p
    with B, its Cholesky factor and the forward substitution in ``np.longdouble`` (hand-written: numpy's linalg has no
    extended precision); ``dtype=float`` evaluates the same formula in binary64 with LAPACK, the prototype whose distance
    from the truth sets the gate of the device test.
(b) :func:`dense_covariance` -- of order n_omega P, without inverting L:
        Gamma = L^1/2 (alpha I + L^1/2 K L^1/2)^-1 L^1/2,   L_i^1/2 from ``eigh``,   K = (V c^2 V^T) (x) 1_P
"""

import numpy as np

import fullmatrix_ref as R

LD = np.longdouble


def make_problem(M, use_complex, n_omega, n_s, seed, err=0.05, decay=3.0):
    """A whole-matrix problem for the variance tests: V (n_omega, n_s) with orthonormal columns, singular values falling
    over ``decay`` decades from 1, a smooth positive D.  No data: the variances depend on u alone."""
    rng = np.random.RandomState(seed)
    V = np.linalg.qr(rng.randn(n_omega, n_s))[0]
    S = 10.0 ** (-decay * np.arange(n_s) / max(1, n_s - 1)) if n_s > 1 else np.ones(1)
    w = np.linspace(-3.0, 3.0, n_omega)
    D = (0.2 + np.exp(-0.5 * w ** 2)) * 6.0 / n_omega
    G = np.zeros((M, M, n_s), dtype=complex if use_complex else float)
    return R.Problem(np.eye(n_s), S, V, G, err, D, use_complex)


def random_u(p, seed, scale=0.6):
    return scale * np.random.RandomState(seed).randn(p.P, len(p.S))


def random_functionals(p, n_f, seed):
    """(n_f, P, n_omega) coordinates of random Hermitian weights; the first is the trace of the whole spectrum"""
    F = np.random.RandomState(seed).randn(n_f, p.P, len(p.D))
    F[0] = 0.0
    F[0, :p.M] = 1.0
    return F


def cholesky_ld(B):
    """lower Cholesky factor of the symmetric positive definite B, column by column in B's own precision"""
    d = len(B)
    Lc = np.zeros_like(B)
    for j in range(d):
        col = B[j:, j] - np.dot(Lc[j:, :j], Lc[j, :j])
        if not col[0] > 0:
            raise np.linalg.LinAlgError('not positive definite at column %d' % j)
        Lc[j:, j] = col / np.sqrt(col[0])
    return Lc


def forward_ld(Lc, Y):
    """Z with Lc Z = Y, row by row in Lc's own precision"""
    Z = np.array(Y, dtype=Lc.dtype)
    for r in range(len(Lc)):
        Z[r] = (Z[r] - np.dot(Lc[r, :r], Z[:r])) / Lc[r, r]
    return Z


def variances(p, u, alpha, F=None, diag=False, dtype=LD):
    """(a).  ``F`` (n_f, P, n_omega).  Returns a dict: ``value``, ``var``, ``prior`` (n_f,), ``terms_value``, ``terms_prior``
    (n_f,): the sums of the magnitudes of the terms of x and of f^T L f; with ``diag``: ``diag_var``, ``diag_prior``, ``h``
    (P, n_omega).  ``dtype``: np.longdouble (the truth) or float (the binary64 prototype)."""
    st = p.state(u)
    L = p.L(st)                                                   # (n_omega, P, P)
    P, n_s, n_w = p.P, len(p.S), len(p.D)
    d = P * n_s
    Lx, Vx, cx = L.astype(dtype), p.V.astype(dtype), p.c.astype(dtype)
    a = dtype(alpha)
    W = np.einsum('is,ipq,it->psqt', Vx, Lx, Vx)
    B = (cx[None, :, None, None] * W * cx[None, None, None, :]).reshape(d, d)
    B = 0.5 * (B + B.T) + a * np.eye(d, dtype=dtype)
    cols, out = [], {}
    n_f = 0 if F is None else len(F)
    if n_f:
        Fx = np.asarray(F).astype(dtype)
        g = np.einsum('ipq,nqi->npi', Lx, Fx)                     # L_i f_i
        cols.append(np.einsum('s,is,npi->psn', cx, Vx, g).reshape(d, n_f))
        prior = np.einsum('npi,npi->n', Fx, g)
        out['value'] = np.einsum('npi,pi->n', Fx, st['Hc'].astype(dtype))
        out['terms_value'] = np.einsum('npi,pi->n', np.abs(Fx), np.abs(st['Hc']).astype(dtype)).astype(float)
        out['terms_prior'] = np.einsum('npi,ipq,nqi->n', np.abs(Fx), np.abs(Lx), np.abs(Fx)).astype(float)
    if diag:
        # column (p, i): y_(q,s) = c_s V_is L_i,qp
        cols.append(np.einsum('s,is,iqp->qspi', cx, Vx, Lx).reshape(d, P * n_w))
    Y = np.concatenate(cols, axis=1)
    if dtype is LD:
        Z = forward_ld(cholesky_ld(B), Y)
    else:
        Z = np.linalg.solve(np.linalg.cholesky(B), Y)
    q = np.sum(Z * Z, axis=0)
    if n_f:
        out['var'] = np.maximum(prior - q[:n_f], 0) / a
        out['prior'] = prior / a
    if diag:
        dprior = np.einsum('ipp->pi', Lx)
        out['diag_var'] = np.maximum(dprior - q[n_f:].reshape(P, n_w), 0) / a
        out['diag_prior'] = dprior / a
        out['h'] = st['Hc'].astype(dtype)
    return out


def dense_covariance(p, u, alpha):
    """(b): Gamma (n_omega P, n_omega P) in the order (i, p), and L (n_omega, P, P)"""
    st = p.state(u)
    L = p.L(st)
    n_w, P = len(p.D), p.P
    n = n_w * P
    lam, X = np.linalg.eigh(L)
    Lh_i = np.einsum('ipk,ik,iqk->ipq', X, np.sqrt(np.maximum(lam, 0.0)), X)
    Lh = np.zeros((n, n))
    for i in range(n_w):
        Lh[i * P:(i + 1) * P, i * P:(i + 1) * P] = Lh_i[i]
    K = np.kron(np.dot(p.V * p.c ** 2, p.V.T), np.eye(P))
    inner = alpha * np.eye(n) + np.dot(Lh, np.dot(K, Lh))
    Gam = np.dot(Lh, np.linalg.solve(inner, Lh))
    return 0.5 * (Gam + Gam.T), L, float(np.linalg.cond(inner))


def scalar_variances(H, V, c, alpha, F=None, diag=False):
    """the scalar formula of DESIGN 4m with w = H (n_omega,): var(f^T H) and the diagonal of Gamma, in np.longdouble"""
    Hx, Vx, cx, a = H.astype(LD), V.astype(LD), c.astype(LD), LD(alpha)
    n_s = len(c)
    B = cx[:, None] * np.einsum('is,i,it->st', Vx, Hx, Vx) * cx[None, :]
    Lc = cholesky_ld(0.5 * (B + B.T) + a * np.eye(n_s, dtype=LD))
    out = {}
    if F is not None:
        Fx = np.asarray(F).astype(LD)                                # (n_f, n_omega)
        Z = forward_ld(Lc, cx[:, None] * np.dot(Vx.T, (Hx * Fx).T))
        prior = np.sum(Hx * Fx * Fx, axis=1)
        out['var'], out['prior'] = (prior - np.sum(Z * Z, axis=0)) / a, prior / a
    if diag:
        Z = forward_ld(Lc, cx[:, None] * Vx.T)
        out['diag_var'] = (Hx / a) * (1 - Hx * np.sum(Z * Z, axis=0))
    return out
