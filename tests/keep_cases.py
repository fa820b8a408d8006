"""Small problems with DESIGNED singular spectra for ``batch_solver.directions_to_keep``: the directions the device would drop
sit at a chosen distance from the edge of its decision, which no kernel of a physical grid offers (1 000 imaginary times put
them some 1e5 below it).  TEST INFRASTRUCTURE: imports oracle/.  Nothing is read from disk and nothing is tuned on a GPU:
every number below is fixed here, and ``tests/test_keep_bound_host.py`` checks on the CPU where each case lands.

A problem:  K = U diag(S) V^T  with orthonormal U (n_data x n_data) and V (n_omega x n_data) from seeded QRs,

    S_k = 10^(-10 k / 63)   for k < 64            (steep: 1 ... 1e-10),
    S_k = 1e-9              for 64 <= k < keep     (the 160 x 180 shape only: 64 directions are too few there),
    S_k = plateau           for k >= keep          (flat: what the device may or may not drop),

G = K H_true + sigma * noise, ONE error bar sigma = 1e-3, a flat default model.  The fixed point of the device depends on
alpha and eta = chi2_factor through alpha / eta alone, and the bound of ``directions_to_keep`` is, for data dominated by the
noise in the dropped directions, proportional to  plateau * eta / alpha  -- the invariant along which a case may be moved.

Positions (the function's own bound, with eta, against ``KEEP_BOUND`` = 1e-7):
    'below'  within a factor 2 below the edge: the function returns ``keep`` and its claims are measured against the truth;
    'above'  within a factor 2 above: ``None``;
    'far'    a hundred times the 'below' plateau: ``None``.  At eta = 100 and eta = 1e4 this is the plateau of eta = 1's 'below'
             case: the problem that a bound formed with alpha instead of alpha / eta let through (measured before the fix,
             96 x 120, normal entropy: max |delta u| 3.3e-6 and 7.2e-4 where 1e-7 was claimed).
eta = 1e4 at alpha = 1 would need a 'below' plateau of 1.5e-15, under the 1e-14 at which the singular space is cut; its
'below' and 'above' cases are therefore moved along the invariant to alpha = 100 (alpha / eta = 1e-2, the plateaus of
eta = 100), and alpha = 1 is kept for its 'far' case.
"""
import collections
import functools

import numpy as np

import maxent_amd as mx
from maxent_amd import batch_solver
from oracle import hp_truth

SIGMA = 1e-3
N_LADDER = 8                    # alphas of a scan: descending, three decades, the last one the case's
ETAS = (1.0, 100.0, 1e4)
ENTROPIES = ('normal', 'plusminus')
SHAPES = {64: (96, 120), 128: (160, 180)}          # keep -> (n_data, n_omega)
BELOW, ABOVE = 1.5e-11, 2.4e-11                    # plateaus at alpha / eta = 1; 'far' is 100 * BELOW

Case = collections.namedtuple('Case', 'keep entropy eta alpha plateau position')


def _decimal(x):
    """x as the binary64 number of its three-digit decimal: 100 * 1.5e-11 * 0.01 IS the plateau 1.5e-11"""
    return float('%.2e' % x)


def _cases():
    out = []
    for keep in SHAPES:
        for entropy in ENTROPIES:
            for eta in ETAS:
                alpha = 100.0 if eta == 1e4 else 1.0            # (moved along the invariant: the module's docstring)
                x = alpha / eta
                out.append(Case(keep, entropy, eta, alpha, _decimal(BELOW * x), 'below'))
                out.append(Case(keep, entropy, eta, alpha, _decimal(ABOVE * x), 'above'))
                out.append(Case(keep, entropy, eta, alpha, _decimal(100 * BELOW * x), 'far'))
                if alpha != 1.0:
                    out.append(Case(keep, entropy, eta, 1.0, BELOW, 'far'))
    return out


CASES = _cases()


def case_id(c):
    return 'keep%d-%s-eta%g-alpha%g-%s' % (c.keep, c.entropy, c.eta, c.alpha, c.position)


def find(keep, entropy, eta, position, alpha=None):
    got = [c for c in CASES if (c.keep, c.entropy, c.eta, c.position) == (keep, entropy, eta, position) and
           (alpha is None or c.alpha == alpha)]
    assert got, (keep, entropy, eta, position, alpha)
    return got[0]


def expected_decision(c):
    return c.keep if c.position == 'below' else None


def ladder(c):
    """the scaled alphas of the case's scan, in visiting order"""
    return c.alpha * np.geomspace(1e3, 1.0, N_LADDER)


def spectrum(keep, n_data, plateau):
    S = np.full(n_data, float(plateau))
    S[:64] = 10.0 ** (-10.0 * np.arange(64) / 63.0)
    S[64:keep] = 1e-9
    return S


@functools.lru_cache(maxsize=None)
def _basis(keep):
    n_data, n_omega = SHAPES[keep]
    rng = np.random.RandomState(7 + keep)
    U, _ = np.linalg.qr(rng.randn(n_data, n_data))
    V, _ = np.linalg.qr(rng.randn(n_omega, n_data))
    noise = rng.randn(n_data)
    return U, V, noise


@functools.lru_cache(maxsize=None)
def _problem(keep, plateau, entropy):
    n_data, n_omega = SHAPES[keep]
    U, V, noise = _basis(keep)
    Kmat = (U * spectrum(keep, n_data, plateau)[None, :]) @ V.T
    w = np.linspace(-5.0, 5.0, n_omega)
    omega = mx.DataOmegaMesh(w)
    delta = np.asarray(omega.delta, dtype=float)
    a = np.exp(-(w - 1.0) ** 2 / (2 * 0.5 ** 2)) / np.sqrt(2 * np.pi * 0.5 ** 2)
    b = np.exp(-(w + 1.5) ** 2 / (2 * 0.8 ** 2)) / np.sqrt(2 * np.pi * 0.8 ** 2)
    A = 0.6 * a + 0.4 * b if entropy == 'normal' else 0.5 * (a - b)
    H_true = A * delta
    G = Kmat @ H_true + SIGMA * noise
    K = mx.DataKernel(np.arange(float(n_data)), omega, Kmat)
    K.reduce_singular_space(1e-14)
    assert len(K.S) == n_data, 'the designed plateau lies above the cut of the singular space'
    D = np.asarray(mx.FlatDefaultModel(omega).D, dtype=float)
    for x in (Kmat, G, D, H_true):
        x.setflags(write=False)
    return dict(K=K, Kmat=Kmat, omega=omega, delta=delta, G=G, err=SIGMA * np.ones(n_data), D=D, H_true=H_true)


def problem(c):
    """dict(K: DataKernel with all its directions, Kmat, omega, delta, G, err, D, H_true) -- shared, read-only"""
    return _problem(c.keep, c.plateau, c.entropy)


def spec(c, alpha=None):
    """the job of the case as one spec of ``directions_to_keep``"""
    p = problem(c)
    return dict(G=p['G'], err=p['err'], alpha=ladder(c) if alpha is None else np.asarray(alpha, dtype=float), U_rot=None, D=p['D'])


def arrays(c, alpha=None, n=2):
    """the same job as the arrays of ``directions_to_keep``: ``n`` elements with the same data"""
    p = problem(c)
    al = ladder(c) if alpha is None else np.asarray(alpha, dtype=float)
    return dict(n=n, G=np.tile(p['G'], (n, 1)), err=p['err'][None, :], alpha=al[None, :], sel=np.zeros(n, dtype=int), D=p['D'][None, :])


def own_bound(c, keep=None):
    """the bound of ``directions_to_keep`` on max |delta u| for this case, with eta, written out once more:
    |c_k (|ghat_k| + c_k h1)|_2 / (alpha / eta) over the directions behind ``keep``"""
    p = problem(c)
    keep = c.keep if keep is None else keep
    K = p['K']
    ck = np.asarray(K.S)[keep:] / SIGMA
    ghat = np.abs(np.asarray(K.U)[:, keep:].T @ (p['G'] / SIGMA))
    h1 = 1e3 * max(1.0, float(np.sum(np.abs(p['D']))))
    return float(np.linalg.norm(ck * (ghat + ck * h1)) / (c.alpha / c.eta))


def _walk(p, U, S, V, entropy, alphas):
    """binary64 Newton iterates of the gradient  S U^T (K H - G) / sigma^2 + a v  down ``alphas`` (= alpha / eta), each from the
    one before: steps capped at a rise of u by 2 and halved until the gradient shrinks.  Only the START of the polish: the fixed
    point is unique, and whether the polish reached it is asserted there."""
    D, G, Kmat = p['D'], p['G'], p['Kmat']
    m = (S / SIGMA) ** 2
    v = np.zeros(len(S))

    def at(v):
        e = np.exp(V @ v)
        H, w = (D * e, D * e) if entropy == 'normal' else (D * (e - 1 / e), D * (e + 1 / e))
        return H, w, S * (U.T @ (Kmat @ H - G)) / SIGMA ** 2
    out = []
    for a in alphas:
        H, w, gd = at(v)
        g = gd + a * v
        for _ in range(300):
            dv = np.linalg.solve(m[:, None] * ((V.T * w) @ V) + a * np.eye(len(S)), g)
            du = V @ dv
            rise = float(np.max(-du if entropy == 'normal' else np.abs(du)))
            t = 1.0 if rise <= 2.0 else 2.0 / rise
            small = t == 1.0 and np.linalg.norm(w * du) <= 1e-10 * np.linalg.norm(H)
            while True:
                vt = v - t * dv
                Ht, wt, gd = at(vt)
                gt = gd + a * vt
                if np.linalg.norm(gt) < np.linalg.norm(g) or t < 1.0 / 64 or small:
                    break
                t /= 2
            v, H, w, g = vt, Ht, wt, gt
            if small:
                break
        out.append(v.copy())
    return out


@functools.lru_cache(maxsize=None)
def _fixed_points(keep, plateau, entropy, eta, alpha, n_dir):
    """(v, H) of the extended-precision fixed point at the first and the last alpha of the ladder, on the first ``n_dir``
    directions (None: all): binary64 Newton iterates walk the ladder at alpha / eta (:func:`_walk`) and are polished in extended
    precision there (oracle/hp_truth.py).  The polish must have converged (as tests/anchor.py asserts it)."""
    c = Case(keep, entropy, eta, alpha, plateau, None)
    p = problem(c)
    K = p['K']
    n = len(K.S) if n_dir is None else n_dir
    U, S, V = np.asarray(K.U)[:, :n], np.asarray(K.S)[:n], np.asarray(K.V)[:, :n]
    al = ladder(c)
    start = _walk(p, U, S, V, entropy, al / eta)
    out = {}
    for ia in (0, len(al) - 1):
        info = {}
        v, H = hp_truth.polish(p['Kmat'], p['G'], p['err'], p['D'], V, S, al[ia] / eta, start[ia], entropy, iters=6, info=info)
        assert info['converged'], ('the extended-precision polish did not converge', case_id(c), ia, info)
        assert np.all(np.isfinite(H)) and np.all(np.isfinite(v)), 'the fixed point is not finite'
        v.setflags(write=False)
        H.setflags(write=False)
        out[ia] = (v, H)
    return out


def truth(c, ia=-1):
    """(v, H, u = V v) of the ALL-direction fixed point at alpha index ``ia`` (0 or -1) of the case's ladder"""
    return _with_u(c, None, ia)


def truncated(c, ia=-1, keep=None):
    """the same on the first ``keep`` directions (the case's, by default): what the device is asked to find"""
    return _with_u(c, c.keep if keep is None else keep, ia)


def _with_u(c, n_dir, ia):
    v, H = _fixed_points(c.keep, c.plateau, c.entropy, c.eta, c.alpha, n_dir)[ia % N_LADDER]
    return v, H, np.asarray(problem(c)['K'].V)[:, :len(v)] @ v


def dropped_residual(c, H, keep=None, ia=-1):
    """first-order size of what the dropped directions would carry at the image ``H``:
    |c_k (c_k h_k - ghat_k)|_2 / (alpha / eta) over k >= keep, with c_k = S_k / sigma, h_k = V_k^T H, ghat_k = U_k^T G / sigma"""
    p = problem(c)
    keep = c.keep if keep is None else keep
    K = p['K']
    ck = np.asarray(K.S)[keep:] / SIGMA
    hk = np.asarray(K.V)[:, keep:].T @ np.asarray(H, dtype=float)
    ghat = np.asarray(K.U)[:, keep:].T @ (p['G'] / SIGMA)
    return float(np.linalg.norm(ck * (ck * hk - ghat)) / (ladder(c)[ia] / c.eta))


def h1_guess(c):
    """what ``directions_to_keep`` takes for the largest |V_k^T H|"""
    return 1e3 * max(1.0, float(np.sum(np.abs(problem(c)['D']))))


KEEP_BOUND = batch_solver.KEEP_BOUND
