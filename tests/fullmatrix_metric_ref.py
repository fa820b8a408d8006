"""numpy truth of the whole-matrix continuation with one error bar per matrix element: ``MetricProblem`` is
``fullmatrix_ref.Problem`` with the diagonal metric c = S / sigma replaced by a dense factor per Hermitian component,

    diag(1 / sigma_p) U S = Q^_p R_p,   g^_p = Q^_p^T (G_p / sigma_p),   A_p = R_p^T R_p,
    rho_p = R_p V^T H_p - g^_p,   chi2 = sum_p |rho_p|^2 + c_perp,   F_p = alpha u_p + R_p^T rho_p,
    J = alpha I + blockdiag_p(A_p) W.

V is not rotated; S, L, W and Q = chi2 / 2 - alpha S are the parent's.  Written from the equations with numpy's QR, not
with the package's ``whiten_components``; ``fullmatrix_cases.newton_step``, ``step_gate`` and ``backward_error`` work on it
unchanged.  ``pattern`` is the seeded error pattern of the tests.  Plain helpers: no pytest hooks.
"""
import functools

import numpy as np

import fullmatrix_ref as R
import fullmatrix_cases as C


def component_sigma(sigma, M, use_complex):
    """sigma_p (P, n) of the components from sigma_ab (M, M, n): sigma_aa, then sigma_ab for the symmetric and again for the
    antisymmetric component of every pair a < b"""
    pairs = [(a, b) for a in range(M) for b in range(a + 1, M)]
    rows = [sigma[a, a] for a in range(M)] + [sigma[a, b] for a, b in pairs]
    if use_complex:
        rows += [sigma[a, b] for a, b in pairs]
    return np.array(rows, dtype=float)


class MetricProblem(R.Problem):
    """One whole-matrix job with ``sigma`` (M, M, n_tau), symmetric in its first two axes"""

    def __init__(self, U, S, V, G, sigma, D, use_complex):
        R.Problem.__init__(self, U, S, V, G, 1.0, D, use_complex)
        self.err = self.c = None                                # (nothing of the one-error metric is left to be used)
        self.sigma = np.array(sigma, dtype=float)
        assert self.sigma.shape == np.shape(G) and np.array_equal(self.sigma, np.swapaxes(self.sigma, 0, 1))
        self.sp = component_sigma(self.sigma, self.M, use_complex)
        Gw = R.coords(np.asarray(G), self.E) / self.sp          # (P, n_tau)
        n_s = len(self.S)
        self.R, self.ghat = np.empty((self.P, n_s, n_s)), np.empty((self.P, n_s))
        for p in range(self.P):
            Q, self.R[p] = np.linalg.qr((self.U * self.S) / self.sp[p][:, None])
            self.ghat[p] = np.dot(Q.T, Gw[p])
        self.A = np.einsum('pks,pkt->pst', self.R, self.R)
        self.cperp = max(float(np.sum(Gw ** 2) - np.sum(self.ghat ** 2)), 0.0)

    def state(self, u):
        """everything at u, as the parent's, with rho = R_p V^T H_p - ghat_p"""
        Gam = R.from_coords(np.dot(u, self.V.T), self.E)
        g, W = np.linalg.eigh(np.moveaxis(Gam, -1, 0))
        B = W * np.exp(0.5 * g)[:, None, :]
        Hm = self.D[:, None, None] * np.einsum('iak,ibk->iab', B, B.conj())
        Hc = R.coords(np.moveaxis(Hm, 0, -1), self.E)
        rho = np.einsum('pks,ps->pk', self.R, np.dot(Hc, self.V)) - self.ghat
        e = np.exp(g)
        S = float(np.sum(self.D[:, None] * (e - 1.0 - g * e)))
        return dict(g=g, W=W, Hm=Hm, Hc=Hc, rho=rho, chi2=float(np.sum(rho ** 2) + self.cperp), S=S)

    def F(self, alpha, u, st=None):
        st = self.state(u) if st is None else st
        return alpha * u + np.einsum('pks,pk->ps', self.R, st['rho'])

    def J(self, alpha, u, st=None):
        st = self.state(u) if st is None else st
        d = u.size
        return alpha * np.eye(d) + np.einsum('pks,psqt->pkqt', self.A, self.gram(st)).reshape(d, d)


def newton(p, alpha, u0, tol=1e-11, maxiter=400):
    """``fullmatrix_ref.newton`` with the scale of the metric problem: || F || <= tol (|| alpha u || + || R^T ghat ||)"""
    u = np.array(u0, dtype=float)
    st = p.state(u)
    Q0 = 0.5 * st['chi2'] - alpha * st['S']
    mu = 0.0
    scale = np.linalg.norm(np.einsum('pks,pk->ps', p.R, p.ghat))
    d = u.size
    for it in range(maxiter):
        F = p.F(alpha, u, st)
        if np.linalg.norm(F) <= tol * (scale + alpha * np.linalg.norm(u)):
            return u, it, True
        J = p.J(alpha, u, st)
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
    """``fullmatrix_ref.alpha_scan`` over :func:`newton`"""
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


# ---- the jobs of the tests: those of fullmatrix_cases under a seeded error pattern ---------------------------------------

def pattern(M, n):
    """sigma_ab(t) = 1e-3 (1 + sin^2(t / 7) / 2) (1 if a = b else 3) (1 + min(a, b) / 4) (1 + 0.2 cos(t (a + b + 1) / 5))"""
    t = np.arange(n, dtype=float)
    s = np.empty((M, M, n))
    for a in range(M):
        for b in range(M):
            s[a, b] = 1e-3 * (1.0 + 0.5 * np.sin(t / 7.0) ** 2) * (1.0 if a == b else 3.0) * (1.0 + 0.25 * min(a, b)) \
                * (1.0 + 0.2 * np.cos(t * (a + b + 1) / 5.0))
    return s


@functools.lru_cache(maxsize=None)
def problem(case):
    """(MetricProblem, args) of a case of ``fullmatrix_cases``: its G, U, S, V, D under ``pattern``; ``args['sigma']``"""
    _, a = C.problem(case)
    sigma = pattern(case[0], case[4])
    sigma.setflags(write=False)
    p = MetricProblem(a['U'], a['S'], a['V'], a['G'], sigma, a['D'], a['use_complex'])
    return p, dict(a, sigma=sigma, err=None)


@functools.lru_cache(maxsize=None)
def reference_scan(case):
    """:func:`alpha_scan` from zero over ``fullmatrix_cases.case_alphas``; computed once per process, read-only"""
    p, _ = problem(case)
    ref = alpha_scan(p, np.array(C.case_alphas(case)))
    assert ref['converged'].all(), case
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def accepted_step(case):
    """``fullmatrix_cases.accepted_step`` of the metric problem: u0 = the truth's u(a0), one step at a1"""
    p, _ = problem(case)
    a1 = C.case_alphas(case)[1]
    u0 = reference_scan(case)['u'][0]
    step = C.newton_step(p, a1, u0)
    eta_ref, eta_pert, gate = C.step_gate(p, a1, u0, step)
    step.update(u0=u0, alpha=a1, eta_ref=eta_ref, eta_pert=eta_pert, gate=gate)
    return step


@functools.lru_cache(maxsize=None)
def rejected_step(index):
    """``fullmatrix_cases.rejected_step`` of the metric problem"""
    case, seed = C.REJECT_CASES[index]
    p, _ = problem(case)
    u0, alpha = C.bad_start(case, seed)
    step = C.newton_step(p, alpha, u0)
    eta_ref, eta_pert, gate = C.step_gate(p, alpha, u0, step)
    step.update(u0=u0, alpha=alpha, eta_ref=eta_ref, eta_pert=eta_pert, gate=gate, case=case)
    return step
