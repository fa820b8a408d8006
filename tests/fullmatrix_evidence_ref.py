"""numpy truth of the evidence of alpha of the whole-matrix continuation, on ``fullmatrix_ref.Problem``.  Not a
test, and not a port of anything: the reference has neither the solver nor a probability of alpha for it.

With A = c W c (order d = P n_s, W the solver's Gram matrix) and B = alpha I + A = L_B L_B^T:

    logdet = log det(I + A / alpha) = sum_j log(l_jj^2 / alpha)          N_g = tr(A B^-1)

(a) :func:`truth` -- ``np.longdouble``: B and its Cholesky factor by hand (:func:`fullmatrix_postvar_ref.cholesky_ld`), the
    sum of the logarithms as written, and N_g = tr(L_B^-1 A L_B^-T), the trace of a positive semi-definite matrix: nothing
    cancels.
(b) :func:`prototype` -- binary64 with LAPACK, the device's own formulas: the same sum, and N_g = d - alpha |L_B^-1|_F^2.  Its
    distance from (a) sets the gate of the device test.
(c) :func:`dense_logdet` -- of order n_omega P, from the other side of Sylvester's identity:
    slogdet(I + L^1/2 K L^1/2 / alpha), K = (V c^2 V^T) (x) 1_P, L_i^1/2 from ``eigh``; (a) is pinned to it.
:func:`wrong_logdets` holds three plausible mistakes, for the test that the gate would see them.
"""

import numpy as np

import fullmatrix_ref as R                                        # noqa: F401  (Problem: what the functions here work on)
from fullmatrix_postvar_ref import make_problem, random_u, cholesky_ld, forward_ld    # noqa: F401

LD = np.longdouble


def curvature(p, u, dtype=float):
    """A = c W c (d, d) at u, symmetrised, in ``dtype``"""
    st = p.state(u)
    L = p.L(st)
    d = p.P * len(p.S)
    Lx, Vx, cx = L.astype(dtype), p.V.astype(dtype), p.c.astype(dtype)
    W = np.einsum('is,ipq,it->psqt', Vx, Lx, Vx)
    A = (cx[None, :, None, None] * W * cx[None, None, None, :]).reshape(d, d)
    return 0.5 * (A + A.T)


def truth(p, u, alpha, want_ngood=True):
    """(a): dict of ``logdet``, ``n_good`` (np.longdouble; with ``want_ngood``), ``d`` and ``lam_max``, the largest eigenvalue
    of c W c"""
    A = curvature(p, u, LD)
    d = len(A)
    a = LD(alpha)
    Lc = cholesky_ld(A + a * np.eye(d, dtype=LD))
    diag = np.diagonal(Lc)
    out = dict(logdet=np.sum(np.log(diag * diag / a)), d=d, lam_max=float(np.linalg.eigvalsh(A.astype(float))[-1]))
    if want_ngood:
        out['n_good'] = n_good_of_factor(Lc, A)
    return out


def n_good_of_factor(Lc, A):
    """tr(L_B^-1 A L_B^-T) in the precision of Lc: two forward substitutions, the second on (L_B^-1 A)^T"""
    return np.trace(forward_ld(Lc, forward_ld(Lc, A).T))


def prototype(p, u, alpha):
    """(b): the device's formulas in binary64"""
    A = curvature(p, u, float)
    d = len(A)
    Lc = np.linalg.cholesky(A + alpha * np.eye(d))
    diag = np.diagonal(Lc)
    Z = np.linalg.solve(Lc, np.eye(d))
    return dict(logdet=float(np.sum(np.log(diag * diag / alpha))), n_good=float(d - alpha * np.sum(Z * Z)), d=d)


def dense_logdet(p, u, alpha):
    """(c): log det(I + L^1/2 K L^1/2 / alpha) of order n_omega P, and N_g as the trace of M (alpha I + M)^-1 there"""
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
    Mm = np.dot(Lh, np.dot(K, Lh))
    Mm = 0.5 * (Mm + Mm.T)
    sign, ld = np.linalg.slogdet(np.eye(n) + Mm / alpha)
    assert sign > 0
    return float(ld), float(np.trace(np.linalg.solve(alpha * np.eye(n) + Mm, Mm)))


# ---- the cases and the gate of the device test (shared with the host test of the gate's sensitivity) ---------------------------

EPS = np.finfo(float).eps
MARGIN, LOGDET_CAP, NGOOD_CAP, KAPPA_MAX = 8.0, 1e-6, 1e-6, 1e8
# (M, complex, n_omega, n_s): d = P n_s = 1; 16 (one panel exactly, n_omega no multiple of 4); 17 (a last panel of one column);
# 45; 153 (d % 16 = 9); n_omega > 256; 640; 1024 (the limit)
SHAPES = [(1, False, 24, 1), (2, True, 37, 4), (1, False, 40, 17), (3, True, 40, 5), (3, True, 21, 17), (1, True, 300, 15),
          (4, False, 70, 64), (4, True, 70, 64)]
ALPHAS = np.array([0.5, 2.0, 0.1, 5.0, 3.0])
_cases = {}


def case(shape, want_ngood=False):
    """the problem of a shape, five jobs (u, alpha), and for job 0 the truth and the binary64 prototype (computed once; the
    truth of N_g, the slow part at d = 1024, only when it is asked for)"""
    if shape not in _cases:
        M, cx, n_w, n_s = shape
        p = make_problem(M, cx, n_w, n_s, seed=100 + n_w, err=0.01)
        u = np.stack([random_u(p, 7 * n_w + k) for k in range(len(ALPHAS))])
        u.setflags(write=False)
        _cases[shape] = dict(p=p, u=u, truth=truth(p, u[0], ALPHAS[0], want_ngood=False), proto=prototype(p, u[0], ALPHAS[0]))
    c = _cases[shape]
    if want_ngood and 'n_good' not in c['truth']:
        t = truth(c['p'], c['u'][0], ALPHAS[0])
        assert t['logdet'] == c['truth']['logdet']
        c['truth'] = t
    return c


def logdet_scale(t):
    """eps (d + logdet): d pivots, each with a relative rounding error of a few eps, that is an absolute one in its logarithm,
    and the rounding of a sum of that size"""
    return EPS * (t['d'] + float(t['logdet']))


def ngood_scale(t):
    """eps d.  The worst case of d - alpha |L_B^-1|_F^2 is eps d (1 + lam_max / alpha): alpha |L_B^-1|_F^2 <= d, through a
    factor whose condition enters.  The binary64 prototype shows another scale: against eps d (1 + lam_max / alpha) its k falls
    from 2e-3 to 2e-5 as lam_max / alpha rises from 2e2 to 9e3, against eps d it is 0.1 ... 0.7 for d = 1 ... 1024 -- the terms
    alpha / (lam + alpha) near 1, which make up the sum, belong to the well-conditioned directions.  So eps d it is."""
    return EPS * t['d']


def k_proto_logdet(verbose=True):
    """max over the cases of |prototype - truth| / (eps (d + logdet))"""
    ks = []
    for shape in SHAPES:
        t, b = case(shape)['truth'], case(shape)['proto']
        ks.append(abs(b['logdet'] - float(t['logdet'])) / logdet_scale(t))
        if verbose:
            print('%s: d %d, logdet %.6g, lam_max / alpha %.3g; binary64 prototype k_logdet %.3f'
                  % (shape, t['d'], float(t['logdet']), t['lam_max'] / ALPHAS[0], ks[-1]))
    if verbose:
        print('k_proto of logdet: %.3f' % max(ks))
    return max(ks)


def k_proto_ngood(verbose=True):
    """max over the cases of |prototype - truth| / (eps d)"""
    ks = []
    for shape in SHAPES:
        c = case(shape, want_ngood=True)
        t, b = c['truth'], c['proto']
        ks.append(abs(float(b['n_good'] - t['n_good'])) / ngood_scale(t))
        if verbose:
            print('%s: d %d, N_g %.6g, lam_max / alpha %.3g; binary64 prototype k_ngood %.3f (against eps d (1 + lam_max / alpha): '
                  '%.3g)' % (shape, t['d'], float(t['n_good']), t['lam_max'] / ALPHAS[0], ks[-1],
                            ks[-1] / (1.0 + t['lam_max'] / ALPHAS[0])))
    if verbose:
        print('k_proto of N_g: %.3f' % max(ks))
    return max(ks)


def logdet_allowed(k, t):
    return min(MARGIN * k * logdet_scale(t), LOGDET_CAP * max(1.0, float(t['logdet'])))


def ngood_allowed(k, t):
    return min(MARGIN * k * ngood_scale(t), NGOOD_CAP * t['d'])


def wrong_logdets(p, u, alpha):
    """three mistakes a kernel could make, in binary64: ``no_alpha`` -- log det B without - d log alpha; ``c_once`` --
    log det(I + c W / alpha), c applied to the rows alone; ``blocks`` -- the blocks W_pq, p != q, dropped (None for P = 1,
    where there are none)"""
    A = curvature(p, u, float)
    d, n_s, P = len(A), len(p.S), p.P
    out = dict(no_alpha=float(np.linalg.slogdet(A + alpha * np.eye(d))[1]))
    c_full = np.tile(p.c, P)
    out['c_once'] = float(np.linalg.slogdet(np.eye(d) + (A / c_full[None, :]) / alpha)[1])
    out['blocks'] = None
    if P > 1:
        Ab = np.zeros_like(A)
        for q in range(P):
            Ab[q * n_s:(q + 1) * n_s, q * n_s:(q + 1) * n_s] = A[q * n_s:(q + 1) * n_s, q * n_s:(q + 1) * n_s]
        out['blocks'] = float(np.linalg.slogdet(np.eye(d) + Ab / alpha)[1])
    return out
