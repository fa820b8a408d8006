"""Jobs of chosen size for the whole-matrix solver, and the numpy truth of ONE Newton step.

``full_matrix_continue(..., u0=, maxiter=)`` shows single steps of the device's Newton iteration: with ``maxiter=1`` an
accepted full step returns u0 - delta, (J + 0 I) delta = F; a rejected one returns u0; with ``maxiter=2`` a rejected full
step followed by an accepted half step returns u0 - delta / 2.  This module builds problems whose n_s is chosen, not
discovered (``synthetic_problem``), the truth of a step (``newton_step``) and the measure it is judged by
(``backward_error``).  Plain helpers: no pytest hooks.  Used by tests/test_fullmatrix_steps_host.py (the conditions, with
numpy alone) and tests/test_gpu_fullmatrix_steps.py (the device).
"""
import functools

import numpy as np

import fullmatrix_ref as R

EPS = np.finfo(float).eps
GATE_FACTOR = 100.0          # the gate on eta is GATE_FACTOR * max(eta_ref, eta_pert): see step_gate

# (M, use_complex, n_s, n_omega, n_data, near_degenerate): the accepted-step cases and what each one reaches
ACCEPT_CASES = [
    (4, True, 64, 70, 80, False),      # d = 1024, the LDS maximum, n_omega no multiple of 4
    (4, False, 64, 70, 80, False),     # d = 640, M = 4 real
    (3, True, 33, 40, 48, False),      # d = 297 >= 272: a whole pass of 256 columns in the trailing update; d % 16 = 9
    (3, True, 17, 21, 24, False),      # pivoting moves rows, d = 153, n_omega % 4 = 1
    (2, True, 17, 21, 24, False),      # d = 68
    (2, False, 16, 20, 24, False),     # one full tile, d = 48
    (3, False, 1, 5, 6, False),        # d = 6 < 16, n_s = 1
    (1, True, 15, 300, 20, False),     # M = 1 complex, d = 15, n_omega > 256
    (1, False, 17, 300, 24, False),    # d = 17: a last panel of one column
    (2, True, 12, 40, 20, True),       # every omega with eigenvalue gaps of about 1e-9
]
LIMIT_CASES = ACCEPT_CASES[:2]         # end to end at the limit
# the starts whose full Newton step makes Q rise and whose half step lowers it: the case and the seed of u0
REJECT_CASES = [((2, True, 17, 21, 24, False), 5), ((3, False, 33, 40, 48, False), 5)]
SEED = 3


def case_id(case):
    M, cx, n_s, n_w, _, deg = case
    return 'M%d%s-ns%d-nw%d%s' % (M, 'c' if cx else 'r', n_s, n_w, '-deg' if deg else '')


def synthetic_problem(M, use_complex, n_s, n_omega, n_data, seed, sigma=1e-3, near_degenerate=False):
    """A job from its factors: U (n_data, n_s) and V (n_omega, n_s) are the Q factors of seeded Gaussian matrices,
    S = logspace(0, -4, n_s), D = 1 / n_omega, the true H_i = D_i exp(Gamma_i) with Gamma a smooth seeded Hermitian function
    of omega, G = (U S V^T) H + Hermitian noise of size ``sigma``.  ``near_degenerate``: Gamma = gamma(omega) 1 + 1e-9
    X(omega) and the noise likewise a multiple of the unit matrix plus 1e-9 of a Hermitian one, so that Gamma(u) of the
    continued solution has eigenvalue gaps of about 1e-9 at every omega: its eigenvectors are ill-defined, L is not.
    Returns (p, args): the ``fullmatrix_ref.Problem`` and a dict with ``G, U, S, V, D, err, use_complex, n_data``;
    ``full_matrix_continue(G[None], U, S, V, D, alpha, err, use_complex=use_complex)`` is the same job."""
    rng = np.random.RandomState(seed)
    V, _ = np.linalg.qr(rng.randn(n_omega, n_s))
    U, _ = np.linalg.qr(rng.randn(n_data, n_s))
    S = np.logspace(0, -4, n_s)
    w = np.linspace(-4.0, 4.0, n_omega)
    D = np.full(n_omega, 1.0 / n_omega)

    def hermitian(n):
        X = rng.randn(M, M, n) + (1j * rng.randn(M, M, n) if use_complex else 0.0)
        return 0.5 * (X + np.conj(np.swapaxes(X, 0, 1)))
    A = hermitian(3)
    shape = np.array([np.cos(w), np.sin(0.7 * w), 0.3 * w])               # (3, n_omega)
    Gam = np.einsum('abk,kw->abw', A, shape)
    noise = sigma * hermitian(n_data)
    if near_degenerate:
        one = np.eye(M)[:, :, None]
        Gam = one * np.dot(rng.randn(3), shape) + 1e-9 * Gam
        noise = one * (sigma * rng.randn(n_data)) + 1e-9 * noise
    g, W = np.linalg.eigh(np.moveaxis(Gam, -1, 0))
    H = np.moveaxis(D[:, None, None] * np.einsum('iak,ik,ibk->iab', W, np.exp(g), W.conj()), 0, -1)
    G = np.einsum('tw,abw->abt', np.dot(U * S, V.T), H) + noise
    G = 0.5 * (G + np.conj(np.swapaxes(G, 0, 1)))
    if not use_complex:
        G = np.ascontiguousarray(G.real)
    p = R.Problem(U, S, V, G, sigma, D, use_complex)
    return p, dict(G=G, U=U, S=S, V=V, D=D, err=sigma, use_complex=use_complex, n_data=n_data)


@functools.lru_cache(maxsize=None)
def problem(case):
    M, cx, n_s, n_w, n_t, deg = case
    return synthetic_problem(M, cx, n_s, n_w, n_t, SEED, near_degenerate=deg)


# a1 / n_data where it is not 20.  With its one singular value, c = 1e3, the n_s = 1 job is decided by the data at
# alpha = 20 n_data: halving alpha moves the minimum so little that the step lowers Q by 9e-5 of |Q| (every seed from 1 to 12
# gave 6e-5 to 1e-3), too little to call the step clearly accepted; at 5000 n_data, where alpha is within a factor of a
# hundred of c^2 L, it is 2e-2.
A1_FACTOR = {(3, False, 1, 5, 6, False): 5000.0}


def case_alphas(case):
    """(a0, a1) = (40, 20) n_data (A1_FACTOR: 2 f, f): the reference converges from zero at a0; the warm full step at
    a1 = a0 / 2 lowers Q"""
    f = A1_FACTOR.get(case, 20.0)
    return 2.0 * f * case[4], f * case[4]


@functools.lru_cache(maxsize=None)
def reference_scan(case):
    """``fullmatrix_ref.alpha_scan`` from zero over (a0, a1): u[0] is the start of the accepted step at a1, and the whole
    of it the truth of the end-to-end runs.  Computed once per process; nobody writes to it."""
    p, _ = problem(case)
    ref = R.alpha_scan(p, np.array(case_alphas(case)))
    assert ref['converged'].all(), case
    for v in ref.values():
        v.setflags(write=False)
    return ref


def backward_error(J, F, delta):
    """eta = || J delta - F ||_inf / (|| J ||_inf || delta ||_inf + || F ||_inf): the size, relative to J and F, of the
    smallest change of them that makes delta exact (Rigal & Gaches).  It does not grow with cond(J); rounding shows as a
    small multiple of eps, a structural error of J or of the solve at 1 / (n_omega d) or more."""
    J, F, delta = np.asarray(J), np.ravel(F), np.ravel(delta)
    r = np.dot(J, delta) - F
    return float(np.max(np.abs(r)) / (np.linalg.norm(J, np.inf) * np.max(np.abs(delta)) + np.max(np.abs(F))))


def newton_step(p, alpha, u0):
    """the truth of one undamped Newton step at u0: ``J`` (d, d), ``F`` (d,), ``delta`` = solve(J, F) (d,), ``Q0``, and
    ``dQ``, the change of Q relative to |Q0| at u0 - delta, u0 - delta / 2 and u0 - delta / 4"""
    u0 = np.asarray(u0, dtype=float)
    st = p.state(u0)
    J, F = p.J(alpha, u0, st), p.F(alpha, u0, st).ravel()
    delta = np.linalg.solve(J, F)
    Q0 = 0.5 * st['chi2'] - alpha * st['S']
    with np.errstate(all='ignore'):
        dQ = [(p.Q(alpha, u0 - f * delta.reshape(u0.shape)) - Q0) / abs(Q0) for f in (1.0, 0.5, 0.25)]
    return dict(J=J, F=F, delta=delta, Q0=Q0, dQ=dQ, st=st)


def perturbed_delta(p, alpha, u0, seed=1):
    """the step solved at u0 (1 +- eps) with seeded signs: what a last-bit change of every input of the assembly does"""
    u0 = np.asarray(u0, dtype=float)
    up = u0 * (1.0 + EPS * np.sign(np.random.RandomState(seed).randn(*u0.shape)))
    st = p.state(up)
    return np.linalg.solve(p.J(alpha, up, st), p.F(alpha, up, st).ravel())


def step_gate(p, alpha, u0, step=None):
    """(eta_ref, eta_pert, gate) of the step at u0, from the reference alone: eta_ref is LAPACK's own backward error on the
    system, eta_pert that of the step solved at u0 (1 +- eps) against the unperturbed J and F, the gate
    GATE_FACTOR = 100 times the larger.  The factor covers what differs legitimately on the device: Jacobi instead of
    LAPACK eigenvectors, FMA chains of length n_omega in another order, the elimination order of a blocked LU."""
    step = newton_step(p, alpha, u0) if step is None else step
    eta_ref = backward_error(step['J'], step['F'], step['delta'])
    eta_pert = backward_error(step['J'], step['F'], perturbed_delta(p, alpha, u0))
    return eta_ref, eta_pert, GATE_FACTOR * max(eta_ref, eta_pert)


@functools.lru_cache(maxsize=None)
def accepted_step(case):
    """the accepted-step job of a case: start u0 = the reference's converged u at a0, one step at a1 = a0 / 2.  A dict with
    ``u0``, ``alpha``, the entries of ``newton_step`` and ``eta_ref``, ``eta_pert``, ``gate``.  Computed once per process."""
    p, _ = problem(case)
    a1 = case_alphas(case)[1]
    u0 = reference_scan(case)['u'][0]
    step = newton_step(p, a1, u0)
    eta_ref, eta_pert, gate = step_gate(p, a1, u0, step)
    step.update(u0=u0, alpha=a1, eta_ref=eta_ref, eta_pert=eta_pert, gate=gate)
    return step


def bad_start(case, seed):
    """u0 = randn(P, n_s) logspace(0, -2, n_s) and alpha = n_data: a start far from the minimum"""
    p, _ = problem(case)
    n_s = case[2]
    return np.random.RandomState(seed).randn(p.P, n_s) * np.logspace(0, -2, n_s), 1.0 * case[4]


@functools.lru_cache(maxsize=None)
def rejected_step(index):
    """the job of REJECT_CASES[index]: ``u0``, ``alpha``, the entries of ``newton_step`` and the gate of the step"""
    case, seed = REJECT_CASES[index]
    p, _ = problem(case)
    u0, alpha = bad_start(case, seed)
    step = newton_step(p, alpha, u0)
    eta_ref, eta_pert, gate = step_gate(p, alpha, u0, step)
    step.update(u0=u0, alpha=alpha, eta_ref=eta_ref, eta_pert=eta_pert, gate=gate, case=case)
    return step


def gate_row(name, step, eta_dev=None, fwd=None):
    """one line of the table the tests print"""
    row = '%-22s d %4d  eta_ref %.1e  eta_pert %.1e  gate %.1e' % (name, step['F'].size, step['eta_ref'], step['eta_pert'],
                                                                 step['gate'])
    if eta_dev is not None:
        row += '  device eta %.1e  |delta - delta_ref| / |delta_ref| %.1e' % (eta_dev, fwd)
    return row
