"""numpy truth of the whole-matrix continuation: the equations of ``FullMatrixMaxEnt`` in plain numpy, with
``numpy.linalg.eigh`` for the matrix exponential and a damped Newton iteration that runs to a relative residual of 1e-11.

Not a port of anything: the reference has no such solver.  The tests of ``mxe_fullmatrix_solve`` compare with it, and
``tests/test_fullmatrix_host.py`` checks it (finite differences, block-diagonal data against the scalar truth, unitary
covariance).

Notation: H_i = D_i exp(Gamma_i), Gamma_i = sum_p (V u)_ip E_p, E_p an orthonormal basis of the Hermitian M x M matrices;
``u`` is (P, n_s).  ``c`` = S / sigma, ``ghat`` = U^T G_p / sigma (P, n_s), ``cperp`` the part of chi2 outside the singular
space; F = alpha u + c (c V^T H_p - ghat_p).
"""

import numpy as np

SQ2 = np.sqrt(2.0)


def basis(M, use_complex):
    """E_p (P, M, M): the diagonal units, then (e_ab + e_ba) / sqrt 2 for a < b, then (complex) i (e_ab - e_ba) / sqrt 2"""
    E = []
    for a in range(M):
        X = np.zeros((M, M), dtype=complex)
        X[a, a] = 1.0
        E.append(X)
    for a in range(M):
        for b in range(a + 1, M):
            X = np.zeros((M, M), dtype=complex)
            X[a, b] = X[b, a] = 1.0 / SQ2
            E.append(X)
    if use_complex:
        for a in range(M):
            for b in range(a + 1, M):
                X = np.zeros((M, M), dtype=complex)
                X[a, b] = 1.0j / SQ2
                X[b, a] = -1.0j / SQ2
                E.append(X)
    return np.array(E)


def coords(X, E):
    """Tr(E_p X) along the two leading axes of X: (M, M, ...) -> (P, ...), real"""
    return np.einsum('pba,ab...->p...', E, X).real


def from_coords(x, E):
    """sum_p x_p E_p: (P, ...) -> (M, M, ...)"""
    return np.einsum('p...,pab->ab...', x, E)


def phi(a, b):
    """(e^a - e^b) / (a - b) = e^((a + b) / 2) sinh(x) / x, x = (a - b) / 2; a series for small x"""
    x = 0.5 * (a - b)
    x2 = x * x
    series = 1.0 + x2 / 6.0 * (1.0 + x2 / 20.0 * (1.0 + x2 / 42.0 * (1.0 + x2 / 72.0 * (1.0 + x2 / 110.0))))
    with np.errstate(all='ignore'):
        direct = np.sinh(x) / np.where(x == 0.0, 1.0, x)
    return np.exp(0.5 * (a + b)) * np.where(np.abs(x) < 0.1, series, direct)


class Problem(object):
    """One whole-matrix job.  ``K`` (n_tau, n_omega) maps H to G; ``U, S, V`` its truncated SVD; ``G`` (M, M, n_tau)
    Hermitian; ``err`` a scalar; ``D`` (n_omega,) including delta omega."""

    def __init__(self, U, S, V, G, err, D, use_complex):
        self.U, self.S, self.V = (np.asarray(x, dtype=float) for x in (U, S, V))
        self.D = np.asarray(D, dtype=float)
        G = np.asarray(G)
        self.M = G.shape[0]
        self.E = basis(self.M, use_complex)
        self.P = len(self.E)
        self.err = float(err)
        Gp = coords(G, self.E)                                  # (P, n_tau)
        self.c = self.S / self.err
        self.ghat = np.dot(Gp, self.U) / self.err               # (P, n_s)
        self.cperp = float(np.sum((Gp / self.err) ** 2) - np.sum(self.ghat ** 2))
        self.cperp = max(self.cperp, 0.0)
        self.n_tau = G.shape[-1]

    def state(self, u):
        """everything at u: eigenvalues g (n_omega, M), eigenvectors W, H coordinates (P, n_omega), rho, chi2, S"""
        Gam = from_coords(np.dot(u, self.V.T), self.E)          # (M, M, n_omega)
        g, W = np.linalg.eigh(np.moveaxis(Gam, -1, 0))
        B = W * np.exp(0.5 * g)[:, None, :]
        Hm = self.D[:, None, None] * np.einsum('iak,ibk->iab', B, B.conj())
        Hc = coords(np.moveaxis(Hm, 0, -1), self.E)
        rho = self.c * np.dot(Hc, self.V) - self.ghat
        e = np.exp(g)
        S = float(np.sum(self.D[:, None] * (e - 1.0 - g * e)))
        chi2 = float(np.sum(rho ** 2) + self.cperp)
        return dict(g=g, W=W, Hm=Hm, Hc=Hc, rho=rho, chi2=chi2, S=S)

    def Q(self, alpha, u):
        st = self.state(u)
        return 0.5 * st['chi2'] - alpha * st['S']

    def F(self, alpha, u, st=None):
        st = self.state(u) if st is None else st
        return alpha * u + self.c * st['rho']

    def L(self, st):
        """the Frechet derivative of D exp in the coordinates of E: (n_omega, P, P), symmetric"""
        W = st['W']
        Et = np.einsum('iak,pab,ibl->ipkl', W.conj(), self.E, W)
        ph = phi(st['g'][:, :, None], st['g'][:, None, :])
        return self.D[:, None, None] * np.einsum('ipkl,ikl,iqkl->ipq', Et, ph, Et.conj()).real

    def gram(self, st):
        """W_(p,s),(q,t) = sum_i V_is L_i,pq V_it as (P, n_s, P, n_s)"""
        return np.einsum('is,ipq,it->psqt', self.V, self.L(st), self.V)

    def J(self, alpha, u, st=None):
        st = self.state(u) if st is None else st
        d = u.size
        return alpha * np.eye(d) + (self.c[None, :, None, None] ** 2 * self.gram(st)).reshape(d, d)

    def grad_Q(self, alpha, u):
        """dQ/du = W F (the gradient the finite differences of Q see)"""
        st = self.state(u)
        d = u.size
        return np.dot(self.gram(st).reshape(d, d), self.F(alpha, u, st).ravel()).reshape(u.shape)


def newton(p, alpha, u0, tol=1e-11, maxiter=400):
    """damped Newton to || F || <= tol (|| alpha u || + || c ghat ||); returns (u, n_iter, converged)"""
    u = np.array(u0, dtype=float)
    st = p.state(u)
    Q0 = 0.5 * st['chi2'] - alpha * st['S']
    mu = 0.0
    scale = np.linalg.norm(p.c * p.ghat)
    for it in range(maxiter):
        F = p.F(alpha, u, st)
        if np.linalg.norm(F) <= tol * (scale + alpha * np.linalg.norm(u)):
            return u, it, True
        J = p.J(alpha, u, st)
        d = u.size
        while True:
            delta = np.linalg.solve(J + mu * np.eye(d), F.ravel()).reshape(u.shape)
            with np.errstate(all='ignore'):
                st1 = p.state(u - delta)
                Q1 = 0.5 * st1['chi2'] - alpha * st1['S']
            if np.isfinite(Q1) and Q1 <= Q0 + 1e-13 * abs(Q0):
                break
            mu = alpha * 1e-3 if mu == 0.0 else mu * 4.0
            if mu > 1e12 * alpha:
                return u, it, False
        u, st, Q0 = u - delta, st1, Q1
        mu = mu / 4.0 if mu > alpha * 1e-3 else 0.0
    return u, maxiter, False


def alpha_scan(p, alphas, u0=None, tol=1e-11):
    """the alpha mesh in order, warm-started; ``alphas`` already scaled by n_tau.  Returns a dict: u (n_alpha, P, n_s),
    H (M, M, n_alpha, n_omega) complex, chi2, S, Q, n_iter, converged"""
    n_s, n_w = len(p.S), len(p.D)
    u = np.zeros((p.P, n_s)) if u0 is None else np.array(u0, dtype=float)
    X = len(alphas)
    out = dict(u=np.empty((X, p.P, n_s)), H=np.empty((p.M, p.M, X, n_w), dtype=complex), chi2=np.empty(X), S=np.empty(X),
               Q=np.empty(X), n_iter=np.zeros(X, dtype=int), converged=np.zeros(X, dtype=bool))
    for ia, a in enumerate(alphas):
        u, n, ok = newton(p, float(a), u, tol=tol)
        st = p.state(u)
        out['u'][ia] = u
        out['H'][:, :, ia, :] = np.moveaxis(st['Hm'], 0, -1)
        out['chi2'][ia], out['S'][ia] = st['chi2'], st['S']
        out['Q'][ia] = 0.5 * st['chi2'] - a * st['S']
        out['n_iter'][ia], out['converged'][ia] = n, ok
    return out
