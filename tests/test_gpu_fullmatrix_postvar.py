"""Posterior variances of the whole-matrix continuation on the device (mxe_fullmatrix_posterior_var) against
the extended-precision truth (a) of tests/fullmatrix_postvar_ref.py.  Every test hands a seeded random u to the C interface
or to ``full_matrix_posterior_errors``: no solve, so a fault of the kernel cannot hide behind convergence.

The gate.  A variance is a difference, prior - |L_B^-1 y|^2, and the relative error of what binary64 evaluates grows as 1 / r,
r = var / prior.  ``k_proto`` is measured here, on the CPU: the same formula in binary64 numpy (LAPACK) on these
very cases against the truth, k_proto = max |dvar| / var * r / eps.  The device may be off by 8 k_proto eps / r -- 8 is the
project's margin for another summation order, as in the shrinkage tests -- and never by more than the project's 1e-6.  alpha
and the error are chosen so that r >= 1e-8 for every pair, which is asserted; no pair is left out.  The values x and the
priors, plain sums, must agree to 64 eps sum |terms|."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, synthetic
from maxent_amd.full_matrix import FullMatrixMaxEnt, full_matrix_posterior_errors
from maxent_amd.kernels import TauKernel
import fullmatrix_postvar_ref as PR

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = np.finfo(float).eps
GATE, R_MIN, MARGIN, SUM_GATE = 1e-6, 1e-8, 8.0, 64.0

# (M, complex, n_omega, n_s): d = P n_s = 1; 16 (one panel exactly, n_omega no multiple of 4); 17 (the first row of a second
# panel); 21; 45; 640; 1024 (the limit)
SHAPES = [(1, False, 24, 1), (2, True, 37, 4), (1, False, 40, 17), (2, False, 33, 7), (3, True, 40, 5), (4, False, 70, 64),
          (4, True, 72, 64)]
ALPHAS = np.array([0.5, 2.0, 0.1, 5.0, 1.0])
N_F = 17


@functools.lru_cache(maxsize=None)
def case(shape):
    """the problem of a shape, five jobs (u, alpha), 17 functionals, and for job 0 the truth and the binary64 prototype"""
    M, cx, n_w, n_s = shape
    p = PR.make_problem(M, cx, n_w, n_s, seed=100 + n_w, err=0.01)
    u = np.stack([PR.random_u(p, 7 * n_w + k) for k in range(len(ALPHAS))])
    F = PR.random_functionals(p, N_F, 3 * n_w)
    truth = PR.variances(p, u[0], ALPHAS[0], F, diag=True)
    proto = PR.variances(p, u[0], ALPHAS[0], F, diag=True, dtype=float)
    for x in (u, F):
        x.setflags(write=False)
    return dict(p=p, u=u, F=F, truth=truth, proto=proto)


def figure(var, var_t, prior_t):
    """(max |dvar| / var * r / eps, smallest r) of variances against the truth"""
    var_t, prior_t = np.asarray(var_t, dtype=float), np.asarray(prior_t, dtype=float)
    r = var_t / prior_t
    return float(np.max(np.abs(np.asarray(var, dtype=float) - var_t) / var_t * r / EPS)), float(r.min())


@pytest.fixture(scope='module')
def k_proto():
    ks = []
    for shape in SHAPES:
        c = case(shape)
        for key in ('var', 'diag_var'):
            k, r_min = figure(c['proto'][key], c['truth'][key], c['truth'][key.replace('var', 'prior')])
            print('%s %s: binary64 prototype k = %.2f, smallest r %.3g' % (shape, key, k, r_min))
            ks.append(k)
    k = max(ks)
    print('k_proto = %.2f' % k)
    assert 0.1 < k < 1e3, k                                           # (the prototype itself is sane)
    return k


def gate(label, k, var, var_t, prior_t):
    var, var_t, prior_t = (np.asarray(x, dtype=float) for x in (var, var_t, prior_t))
    r = var_t / prior_t
    assert np.all(r >= R_MIN) and np.all(var_t > 0), (label, float(r.min()))
    assert np.all(np.isfinite(var)) and np.all(var >= 0), label
    rel = np.abs(var - var_t) / var_t
    allowed = np.minimum(MARGIN * k * EPS / r, GATE)
    print('%s: %d variances, r in [%.3g, %.3g], worst |dvar| / var %.3e, worst k = |dvar| / var * r / eps %.2f (k_proto %.2f), '
          'worst error / allowed %.3f' % (label, var.size, r.min(), r.max(), rel.max(), float(np.max(rel * r / EPS)), k,
                                         float(np.max(rel / allowed))))
    assert np.all(rel <= allowed), (label, float(np.max(rel / allowed)))


def sums(label, x, x_t, terms):
    x, x_t, terms = (np.asarray(a, dtype=float) for a in (x, x_t, terms))
    e = np.abs(x - x_t) / (EPS * terms)
    print('%s: worst |dx| / (eps sum |terms|) %.2f' % (label, e.max()))
    assert np.all(e <= SUM_GATE), (label, float(e.max()))


def run(c, shape, jobs=(0,), fsel=slice(None), want_diag=False, alpha=None, u=None):
    p = c['p']
    jobs = list(jobs)
    F = c['F'][fsel]
    return device.fullmatrix_posterior_var(p.V, p.c, p.D, ALPHAS[jobs] if alpha is None else alpha, c['u'][jobs] if u is None else u,
                                           shape[0], shape[1], F=F if len(F) else None, want_diag=want_diag)


@pytest.mark.parametrize('want_diag', [False, True])
@pytest.mark.parametrize('n_f', [1, 16, 17])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d%s_w%d_s%d' % (s[0], 'c' if s[1] else 'r', s[2], s[3]))
def test_against_the_truth(shape, n_f, want_diag, k_proto):
    c = case(shape)
    t = c['truth']
    out = run(c, shape, fsel=slice(0, n_f), want_diag=want_diag)
    label = '%s n_f %d' % (shape, n_f)
    assert out['var'].shape == (1, n_f)
    gate(label + ' functionals', k_proto, out['var'][0], t['var'][:n_f], t['prior'][:n_f])
    sums(label + ' values', out['value'][0], t['value'][:n_f], t['terms_value'][:n_f])
    sums(label + ' priors', out['prior'][0], t['prior'][:n_f], t['terms_prior'][:n_f] / ALPHAS[0])
    assert np.all(out['var'] <= out['prior'])
    if want_diag:
        gate(label + ' diagonal', k_proto, out['diag_var'][0], t['diag_var'], t['diag_prior'])
        # L_pp is a sum of non-negative terms: its own magnitude
        sums(label + ' diagonal priors', out['diag_prior'][0], t['diag_prior'], t['diag_prior'])
        assert np.all(out['diag_var'] <= out['diag_prior'])
        p = c['p']
        st = p.state(c['u'][0])
        # h_p,i = D_i sum_k (W e^gamma W^H) in the coordinates of E_p: the terms are those of |W| e^gamma |W|^T
        Habs = p.D[:, None, None] * np.einsum('iak,ik,ibk->iab', np.abs(st['W']), np.exp(st['g']), np.abs(st['W']))
        terms = np.einsum('pab,iab->pi', np.abs(p.E), Habs)
        sums(label + ' h', out['h'][0], t['h'], terms)
    else:
        assert 'diag_var' not in out


# ---- bits -------------------------------------------------------------------------------------------------------------------

BIT_SHAPES = [(2, True, 37, 4), (1, False, 40, 17), (3, True, 40, 5)]


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and set(a) == set(b)


@pytest.mark.parametrize('shape', BIT_SHAPES)
def test_a_job_alone_is_the_job_in_a_batch(shape):
    c = case(shape)
    batch = run(c, shape, jobs=range(5), want_diag=True)
    again = run(c, shape, jobs=range(5), want_diag=True)
    assert same(batch, again)                                         # a repeat is the first run
    assert np.all(np.isfinite(batch['var'])) and np.all(np.isfinite(batch['diag_var']))
    for j in range(5):
        alone = run(c, shape, jobs=[j], want_diag=True)
        assert all(np.array_equal(alone[k][0], batch[k][j]) for k in batch), j
    assert not np.array_equal(batch['var'][0], batch['var'][1])


@pytest.mark.parametrize('shape', BIT_SHAPES)
def test_a_functional_alone_is_the_functional_at_position_9_of_17(shape):
    c = case(shape)
    full = run(c, shape)
    for pos in (9, 16, 0):
        alone = run(c, shape, fsel=slice(pos, pos + 1))
        assert all(np.array_equal(alone[k][:, 0], full[k][:, pos]) for k in ('value', 'var', 'prior')), pos
    # and the diagonal does not depend on the functionals
    a, b = run(c, shape, want_diag=True), run(c, shape, fsel=slice(0, 0), want_diag=True)
    assert all(np.array_equal(a[k], b[k]) for k in ('diag_var', 'diag_prior', 'h'))


def test_more_jobs_than_scratch_slices():
    """2^20 frequencies make a slice of the scratch 176 MB: six slices fit below the cap of 1 GiB, seven jobs go through
    them in strides, workgroup 0 jobs 0 and 6.  Job 0 has a NaN in its u: it is NaN, and job 6, which the same workgroup
    takes after it, is bit for bit the job alone (one slice), as are the others.  The sums of 2^20 terms run as 16 chains of
    2^16: (2^16 + 16) eps = 7e-12 bounds their rounding."""
    n_w, n_s = 1 << 20, 1
    rng = np.random.RandomState(5)
    V = np.abs(rng.randn(n_w, n_s)) / np.sqrt(n_w)
    c, D = np.array([3e4]), np.full(n_w, 1.0 / n_w)
    alpha = np.linspace(0.5, 2.0, 7)
    u = rng.randn(7, 1, n_s)
    F = np.ones((1, 1, n_w))
    u[0, 0, 0] = np.nan
    batch = device.fullmatrix_posterior_var(V, c, D, alpha, u, 1, False, F=F)
    assert all(np.all(np.isnan(batch[k][0])) and np.all(np.isfinite(batch[k][1:])) for k in batch)
    for j in (1, 5, 6):
        alone = device.fullmatrix_posterior_var(V, c, D, alpha[j:j + 1], u[j:j + 1], 1, False, F=F)
        assert all(np.array_equal(alone[k][0], batch[k][j]) for k in batch), j
    # and the numbers are right: the scalar formula, d = 1
    H = D * np.exp(np.dot(V, u[6, 0]))
    prior = np.sum(H)
    y = c[0] * np.sum(V[:, 0] * H)
    B = alpha[6] + c[0] ** 2 * np.sum(V[:, 0] ** 2 * H)
    assert np.isclose(batch['value'][6, 0], prior, rtol=1e-10) and np.isclose(batch['prior'][6, 0], prior / alpha[6], rtol=1e-10)
    assert 0.05 < 1 - y * y / B / prior < 0.95                        # (r is neither 0 nor 1)
    assert np.isclose(batch['var'][6, 0], (prior - y * y / B) / alpha[6], rtol=1e-9)


def tau_problem(n_prob=1):
    """a whole-matrix job for the plain function: the kernel of 41 tau x 40 omega, M = 2 real"""
    tau, omega = synthetic.grids(41, 40)
    K = TauKernel(tau=tau, omega=omega, beta=synthetic.BETA)
    K.reduce_singular_space(1e-10)
    D = synthetic.flat_D(omega)
    rng = np.random.RandomState(17)
    return K, omega, np.asarray(D, dtype=float), 0.5 * rng.randn(n_prob, 6, 3, len(K.S))


def test_alpha_all_is_the_per_alpha_calls():
    K, omega, D, u = tau_problem(2)
    alpha = np.geomspace(0.3, 300.0, 6)
    kw = dict(use_complex=False, windows=[(-2, 0), (0, 2)], omega=omega, pointwise=True)
    err = 1e-2 * (1.0 + 0.5 * np.linspace(0, 1, 41))                  # one error per tau: u is rotated as in the solve
    for e in (1e-2, err):
        al = full_matrix_posterior_errors(u, K.U, K.S, K.V, D, alpha, e, **kw)
        assert al['window_err'].shape == (2, 6, 2, 2, 2) and al['A_err'].shape == (2, 6, 2, 2, 40) and not al['info']['nan_jobs']
        for n in range(2):
            for a in range(6):
                one = full_matrix_posterior_errors(u[n:n + 1, a:a + 1], K.U, K.S, K.V, D, alpha[a:a + 1], e, **kw)
                for k in one:
                    if k not in ('info', 'alpha'):
                        assert np.array_equal(one[k][0, 0], al[k][n, a]), (k, n, a)


def test_one_error_per_tau_against_the_truth_in_the_whitened_basis(k_proto):
    """err(tau) not constant: diag(1 / err) U S = U^ c Q^T, V' = V Q, and Gamma = V u = V' (Q^T u).  The truth is computed on
    a problem built here from V' and c, at u' = Q^T u formed here: a rotation of u the wrong way round would not pass."""
    import fullmatrix_ref as R
    from maxent_amd import full_matrix
    K, omega, D, u = tau_problem(1)
    U, S, V = (np.asarray(x, dtype=float) for x in (K.U, K.S, K.V))
    n_s, n_w = len(S), len(D)
    err = 1e-2 * (1.0 + 0.5 * np.linspace(0, 1, 41))
    _, c, Qt = np.linalg.svd((U * S) / err[:, None], full_matrices=False)
    Vw = np.dot(V, Qt.T)
    alpha = np.array([0.3, 30.0])
    rng = np.random.RandomState(23)
    X = rng.randn(5, 2, 2, n_w)
    Fm = X + np.swapaxes(X, 1, 2)
    out = full_matrix_posterior_errors(u[:, :2], U, S, V, D, alpha, err, functionals=Fm, omega=omega, pointwise=True)
    p = R.Problem(np.eye(n_s), c, Vw, np.zeros((2, 2, n_s)), 1.0, D, False)
    assert np.allclose(p.c, c)
    f = full_matrix.functional_coordinates(Fm, 2, False, n_w)
    delta = np.asarray(omega.delta, dtype=float)
    for a in range(2):
        uw = np.dot(u[0, a], Qt.T)                                    # rows u_p -> Q^T u_p
        assert np.allclose(np.dot(Vw, uw.T), np.dot(V, u[0, a].T), rtol=1e-10, atol=1e-12)       # the same Gamma
        assert not np.allclose(np.dot(Vw, np.dot(u[0, a], Qt).T), np.dot(V, u[0, a].T), rtol=1e-3, atol=1e-3)
        t = PR.variances(p, uw, alpha[a], f, diag=True)
        gate('per-tau errors, alpha %g, functionals' % alpha[a], k_proto, out['functional_err'][0, a] ** 2, t['var'], t['prior'])
        sums('per-tau errors, values', out['functional_value'][0, a], t['value'], t['terms_value'])
        got = (out['A_err'][0, a] * delta) ** 2                        # (M, M, n_omega): var_a, and var_p / 2 off the diagonal
        got = np.array([got[0, 0], got[1, 1], 2.0 * got[0, 1]])
        assert np.array_equal(out['A_err'][0, a][0, 1], out['A_err'][0, a][1, 0])
        gate('per-tau errors, alpha %g, point-wise' % alpha[a], k_proto, got, t['diag_var'], t['diag_prior'])


# ---- against the scalar kernel ------------------------------------------------------------------------------------------------

def test_M1_is_mxe_posterior_var(k_proto):
    """the v of a TauMaxEnt run, 41 tau x 40 omega, 6 alphas, as the u of a 1 x 1 matrix: windows and point-wise errors of
    ``TauMaxEnt.posterior_errors`` within the sum of the two gates (the scalar kernel's: 1e-6 where r >= 1e-8)"""
    tau, omega, K, G = synthetic.single_G(41, 40)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = omega
    tm.set_G_tau_data(tau, G)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=50, n_points=6)
    tm.set_error(1e-2)
    res = tm.run()
    windows = [(-2, 0), (0, 2), (-6, 6)]
    sc = tm.posterior_errors(res, alpha='all', windows=windows, pointwise=True)
    Ks = tm.K
    v = np.asarray(res.v, dtype=float)
    assert v.shape == (6, len(Ks.S)) and len(Ks.S) <= 64
    fm = full_matrix_posterior_errors(v[None, :, None, :], Ks.U, Ks.S, Ks.V, np.asarray(tm.D.D, dtype=float), res.alpha, 1e-2,
                                      windows=windows, omega=tm.omega, pointwise=True)
    assert np.allclose(fm['A'][0, :, 0, 0], np.asarray(res.A), rtol=1e-9)
    assert np.allclose(fm['window_weight'][0, :, :, 0, 0], sc['window_weight'], rtol=1e-9)
    assert np.array_equal(fm['window_trace'], fm['window_weight'][..., 0, 0])
    for name, got, want, prior in (('windows', fm['window_err'][0, :, :, 0, 0], sc['window_err'], sc['window_prior_err']),
                                   ('point-wise', fm['A_err'][0, :, 0, 0], sc['A_err'], sc['A_prior_err'])):
        r = (want / prior) ** 2
        assert np.all(r >= R_MIN), (name, float(r.min()))
        rel = np.abs(got ** 2 - want ** 2) / want ** 2
        allowed = GATE + np.minimum(MARGIN * k_proto * EPS / r, GATE)
        print('M = 1 against the scalar kernel, %s: worst |dvar| / var %.3e, r >= %.3g' % (name, rel.max(), r.min()))
        assert np.all(rel <= allowed), name
    assert np.allclose(fm['window_prior_err'][0, :, :, 0, 0], sc['window_prior_err'], rtol=1e-9)


# ---- NaN paths ------------------------------------------------------------------------------------------------------------

def test_a_NaN_in_u_stays_in_its_job():
    shape = (3, True, 40, 5)
    c = case(shape)
    clean = run(c, shape, jobs=range(3), want_diag=True)
    u = np.array(c['u'][:3])
    u[1, 4, 2] = np.nan
    out = run(c, shape, jobs=range(3), want_diag=True, u=u)
    for k in out:
        assert np.all(np.isnan(out[k][1])), k
        assert np.array_equal(out[k][0], clean[k][0]) and np.array_equal(out[k][2], clean[k][2]), k
    u[1, 4, 2] = np.inf
    out = run(c, shape, jobs=range(3), want_diag=True, u=u)
    assert all(np.all(np.isnan(out[k][1])) and np.array_equal(out[k][0], clean[k][0]) for k in out)
    # a u that overflows H
    u[1] = c['u'][1]
    u[1, 0] = 1e4
    out = run(c, shape, jobs=range(3), want_diag=True, u=u)
    assert all(np.all(np.isnan(out[k][1])) and np.array_equal(out[k][2], clean[k][2]) for k in out)


def test_a_B_that_is_not_positive_definite_is_NaN():
    """4 frequencies and 40 singular directions: W has rank 4, and with alpha = 1e-30 beside c^2 W ~ 1e8 the matrix B is
    singular in binary64: 36 pivots are rounding noise around zero.  That job is NaN; its neighbours, with alpha far
    above the rounding of c W c, are finite and bit for bit what they are alone."""
    n_w, n_s = 4, 40
    rng = np.random.RandomState(2)
    V = rng.randn(n_w, n_s)
    c = 1e4 * np.ones(n_s)
    D = np.full(n_w, 0.25)
    u = 0.1 * rng.randn(3, 1, n_s)
    alpha = np.array([1e12, 1e-30, 1e12])
    F = np.ones((2, 1, n_w))
    F[1, 0, ::2] = -1.0
    out = device.fullmatrix_posterior_var(V, c, D, alpha, u, 1, False, F=F, want_diag=True)
    for k in out:
        assert np.all(np.isnan(out[k][1])), k
        assert np.all(np.isfinite(out[k][0])) and np.all(np.isfinite(out[k][2])), k
    for j in (0, 2):
        alone = device.fullmatrix_posterior_var(V, c, D, alpha[j:j + 1], u[j:j + 1], 1, False, F=F, want_diag=True)
        assert all(np.array_equal(alone[k][0], out[k][j]) for k in out), j


# ---- the class ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def solved():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    fm = FullMatrixMaxEnt()
    fm.set_verbosity(mx.VerbosityFlags.Quiet)
    fm.omega = mx.DataOmegaMesh(z['omega'])
    fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    fm.set_G_tau_data(z['tau'], z['G_tau_noise'])
    fm.set_error(float(z['noise']))
    return fm, fm.run(), z


def test_posterior_errors_of_the_fixture(solved):
    fm, res, z = solved
    n_w = len(z['omega'])
    windows = [(-2, 0), (0, 2)]
    out = fm.posterior_errors(res, windows=windows, pointwise=True)
    shapes = dict(window_weight=(2, 2, 2), window_err=(2, 2, 2), window_prior_err=(2, 2, 2), window_trace=(2,),
                  window_trace_err=(2,), window_trace_prior_err=(2,), A=(2, 2, n_w), A_err=(2, 2, n_w), A_prior_err=(2, 2, n_w),
                  alpha=(), alpha_index=())
    assert set(out) == set(shapes) | {'info'}
    for k, s in shapes.items():
        assert np.shape(out[k]) == s, (k, np.shape(out[k]))
    ia = res.analyzer_results[res.default_analyzer_name]['alpha_index']
    assert out['alpha_index'] == ia and out['alpha'] == res.alpha[ia] and out['info']['kernel_ms'] > 0 and not out['info']['nan_rows']
    for k in ('window', 'window_trace', 'A'):
        err, prior = out[k + '_err'], out[k + '_prior_err']
        assert np.all(np.isfinite(err)) and np.all(err >= 0) and np.all(err <= prior), k
    assert np.all(out['A_err'] > 0)
    assert np.allclose(out['window_trace'], out['window_weight'][:, 0, 0] + out['window_weight'][:, 1, 1], rtol=1e-13)
    assert np.allclose(out['A'], res.get_A_out(), rtol=1e-12, atol=1e-15)
    w = np.asarray(z['omega'])
    for n, (lo, hi) in enumerate(windows):
        inside = (w >= lo) & (w <= hi)
        assert np.allclose(out['window_weight'][n], np.sum(np.asarray(res.H)[:, :, ia, inside], axis=-1), rtol=1e-12, atol=1e-15)
    # a list echoes its indices and keeps the axis; 'all'; an analyzer's name; functionals
    many = fm.posterior_errors(res, alpha=[5, 2], windows=windows)
    assert np.array_equal(many['alpha_index'], [5, 2]) and np.array_equal(many['alpha'], res.alpha[[5, 2]])
    assert many['window_err'].shape == (2, 2, 2, 2) and many['window_trace'].shape == (2, 2)
    every = fm.posterior_errors(res, alpha='all', windows=windows)
    assert every['window_err'].shape == (8, 2, 2, 2) and np.array_equal(every['alpha_index'], np.arange(8))
    assert np.array_equal(every['window_err'][[5, 2]], many['window_err']) and np.array_equal(every['window_err'][ia], out['window_err'])
    named = fm.posterior_errors(res, alpha='Chi2CurvatureAnalyzer', windows=windows)
    assert named['alpha_index'] == res.analyzer_results['Chi2CurvatureAnalyzer']['alpha_index']
    Fm = np.zeros((2, 2, 2, n_w))
    Fm[0, 0, 0] = Fm[0, 1, 1] = (w >= -2) & (w <= 0)                   # the trace in the first window
    Fm[1, 0, 1] = Fm[1, 1, 0] = 0.5 * w                                # the first moment of Re A_01
    fun = fm.posterior_errors(res, functionals=Fm)
    assert fun['functional_value'].shape == (2,) and np.all(fun['functional_err'] <= fun['functional_prior_err'])
    assert fun['functional_value'][0] == out['window_trace'][0] and fun['functional_err'][0] == out['window_trace_err'][0]
    assert np.isclose(fun['functional_value'][1], np.sum(w * np.asarray(res.H)[0, 1, ia]), rtol=1e-10, atol=1e-14)
    with pytest.raises(ValueError, match='bryan'):
        fm.posterior_errors(res, alpha='bryan', windows=windows)
    with pytest.raises(ValueError, match='nothing to compute'):
        fm.posterior_errors(res)


def test_posterior_errors_refuse_element_errors(solved):
    fm0, res, z = solved
    fm = FullMatrixMaxEnt()
    fm.set_verbosity(mx.VerbosityFlags.Quiet)
    fm.omega = mx.DataOmegaMesh(z['omega'])
    fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    fm.set_G_tau_data(z['tau'], z['G_tau_noise'])
    fm.set_element_errors(np.full((2, 2), float(z['noise'])))
    with pytest.raises(NotImplementedError, match='set_element_errors'):
        fm.posterior_errors(res, windows=[(-2, 0)])
