"""The evidence of alpha of the whole-matrix continuation on the device (mxe_fullmatrix_logdet) against the
extended-precision truth (a) of tests/fullmatrix_evidence_ref.py.  Every test but the last hands a seeded random u to the C
interface or to ``full_matrix_log_probability``: no solve, so a fault of the kernel cannot hide behind convergence.

The gate (tests/fullmatrix_evidence_ref.py holds the shapes and the scales).  ``k_proto`` is measured here, on the CPU: the
device's formulas in binary64 numpy (LAPACK) on these very cases against the truth, k = max |d logdet| / (eps (d + logdet)).
The device may be off by 8 k_proto eps (d + logdet) -- 8 is the project's margin for another summation order -- and never by
more than 1e-6 max(1, logdet).  For N_g the scale is eps d, which is what the prototype shows (``ngood_scale`` says why it is
not eps d (1 + lam_max / alpha)), the cap 1e-6 d.  lam_max / alpha <= 1e8 is asserted for every case; no case is left out.

Measured (MI355X): k_proto 0.55 (logdet) and 0.72 (N_g); the worst device error over the shapes is 0.53 of its allowance for
logdet (d = 153) and 0.20 for N_g (d = 640), at large alpha 0.07 and 0.34."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, synthetic
from maxent_amd.full_matrix import FullMatrixMaxEnt, full_matrix_log_probability
from maxent_amd.positivity import matrix_positivity
import fullmatrix_evidence_ref as ER

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = np.finfo(float).eps
SHAPE_IDS = ['M%d%s_w%d_s%d' % (s[0], 'c' if s[1] else 'r', s[2], s[3]) for s in ER.SHAPES]


@pytest.fixture(scope='module')
def k_logdet():
    k = ER.k_proto_logdet()
    assert 0.1 < k < 1e3, k                                           # (the prototype itself is sane)
    return k


@pytest.fixture(scope='module')
def k_ngood():
    k = ER.k_proto_ngood()
    assert 0.1 < k < 1e3, k
    return k


def run(c, shape, jobs=(0,), alpha=None, u=None, want_ngood=True):
    p = c['p']
    jobs = list(jobs)
    return device.fullmatrix_logdet(p.V, p.c, p.D, ER.ALPHAS[jobs] if alpha is None else alpha, c['u'][jobs] if u is None else u,
                                    shape[0], shape[1], want_ngood=want_ngood)


@pytest.mark.parametrize('shape', ER.SHAPES, ids=SHAPE_IDS)
def test_against_the_truth(shape, k_logdet, k_ngood):
    c = ER.case(shape, want_ngood=True)
    t = c['truth']
    assert t['lam_max'] / ER.ALPHAS[0] <= ER.KAPPA_MAX
    out = run(c, shape)
    assert out['logdet'].shape == (1,) and out['n_good'].shape == (1,)
    e_l, a_l = abs(out['logdet'][0] - float(t['logdet'])), ER.logdet_allowed(k_logdet, t)
    e_n, a_n = abs(float(out['n_good'][0] - t['n_good'])), ER.ngood_allowed(k_ngood, t)
    print('%s: d %d, logdet %.15g off by %.3e = %.2f eps (d + logdet) (allowed %.3e: %.3f of it); N_g %.15g off by %.3e = %.2f eps d '
          '(allowed %.3e: %.3f of it)' % (shape, t['d'], out['logdet'][0], e_l, e_l / ER.logdet_scale(t), a_l, e_l / a_l,
                                           out['n_good'][0], e_n, e_n / ER.ngood_scale(t), a_n, e_n / a_n))
    assert np.isfinite(out['logdet'][0]) and e_l <= a_l
    assert np.isfinite(out['n_good'][0]) and e_n <= a_n
    assert 0.0 <= out['n_good'][0] <= t['d']


@pytest.mark.parametrize('shape', [(2, True, 37, 4), (1, False, 40, 17), (3, True, 21, 17)])
def test_large_alpha(shape, k_logdet, k_ngood):
    """alpha = 1e10 lam_max: logdet = tr(c W c) / alpha ~ 1e-10 << 1 is the sum of d terms log(1 + x), x ~ 1e-10, each known to
    eps: the same gate, now 8 k eps d.  log det B - d log alpha = d * 27.6 - d * 27.6 would leave eps * 27.6 d and more."""
    c = ER.case(shape)
    p, u = c['p'], c['u'][0]
    alpha = 1e10 * c['truth']['lam_max']
    t = ER.truth(p, u, alpha)
    assert 0 < float(t['logdet']) < 1e-6 and 0 < float(t['n_good']) < 1e-6
    out = device.fullmatrix_logdet(p.V, p.c, p.D, np.array([alpha]), u[None], shape[0], shape[1])
    e_l, a_l = abs(out['logdet'][0] - float(t['logdet'])), ER.logdet_allowed(k_logdet, t)
    e_n, a_n = abs(float(out['n_good'][0] - t['n_good'])), ER.ngood_allowed(k_ngood, t)
    print('%s alpha %.3g: logdet %.6e (truth %.6e) off by %.3f of the allowance %.3e; N_g %.6e (truth %.6e) off by %.3f of %.3e'
          % (shape, alpha, out['logdet'][0], float(t['logdet']), e_l / a_l, a_l, out['n_good'][0], float(t['n_good']), e_n / a_n, a_n))
    assert e_l <= a_l and e_n <= a_n


def test_M1_is_mxe_logdet(k_logdet):
    """one scalar alpha scan on the chain kernel, 41 tau x 40 omega, 6 alphas: ``mxe_logdet`` (``DeviceContext.logdet``) of its
    launch against ``mxe_fullmatrix_logdet`` with its v as the u of a 1 x 1 matrix, the same V, c = S / sigma, D and scaled
    alpha, that is on the same H.  Both numbers come straight from the device; they agree within the gate, once.
    Measured (MI355X): they differ by 0.3 ... 4.39 eps (d + logdet), 0.998 of the allowance 8 k_proto = 4.40 at worst -- the
    distance of two kernels, each of which may be a gate from the truth."""
    from maxent_amd import hostprep
    n_tau, n_alpha = 41, 6
    tau, omega, K, G = synthetic.single_G(n_tau, 40)
    K.reduce_singular_space(1e-10)
    U, S, V = (np.asarray(x, dtype=float) for x in (K.U, K.S, K.V))
    d = len(S)
    assert d <= 64
    D = np.asarray(synthetic.flat_D(omega), dtype=float)
    sigma = 1e-2
    alphas = np.geomspace(50.0, 0.05, n_alpha) * n_tau
    ctx = device.DeviceContext(U, S, V, device=0)
    try:
        ds = ctx.add_dataset(sigma * np.ones(n_tau))
        ctx.set_elements([ds], [G], D[None], [device.ENTROPY_NORMAL])
        v0 = hostprep.initial_v(V, D, omega.delta, device.ENTROPY_NORMAL)[None]
        out = ctx.solve_chains([0], alphas, v0)
        scalar = ctx.logdet()[0]
    finally:
        ctx.close()
    assert out['converged'].all() and out['v'].shape == (1, n_alpha, d) and np.all(np.isfinite(scalar))
    fm = device.fullmatrix_logdet(V, S / sigma, D, alphas, out['v'][0][:, None, :], 1, False)
    allowed = np.minimum(ER.MARGIN * k_logdet * EPS * (d + fm['logdet']), 1e-6 * np.maximum(1.0, fm['logdet']))
    err = np.abs(fm['logdet'] - scalar)
    print('M = 1 against mxe_logdet: d %d, logdet %s, |difference| in eps (d + logdet) %s, worst error / allowed %.3f'
          % (d, fm['logdet'], err / (EPS * (d + fm['logdet'])), float(np.max(err / allowed))))
    assert np.all(err <= allowed)
    assert np.all(fm['n_good'] > 0) and np.all(fm['n_good'] < d)


# ---- bits -------------------------------------------------------------------------------------------------------------------

BIT_SHAPES = [(2, True, 37, 4), (1, False, 40, 17), (3, True, 21, 17)]


@pytest.mark.parametrize('shape', BIT_SHAPES)
def test_the_bits_of_a_job(shape, monkeypatch):
    """a job's bits are the same alone or as job 3 of 5, with and without want_ngood, and with one scratch slice for all five
    jobs (one workgroup takes them one after the other) instead of five"""
    c = ER.case(shape)
    batch = run(c, shape, jobs=range(5))
    again = run(c, shape, jobs=range(5))
    assert all(np.array_equal(batch[k], again[k]) for k in batch) and set(batch) == {'logdet', 'n_good'}
    assert np.all(np.isfinite(batch['logdet'])) and np.all(np.isfinite(batch['n_good']))
    for j in (3, 0, 4):
        alone = run(c, shape, jobs=[j])
        assert alone['logdet'][0] == batch['logdet'][j] and alone['n_good'][0] == batch['n_good'][j], j
    assert len(set(batch['logdet'])) == 5
    plain = run(c, shape, jobs=range(5), want_ngood=False)
    assert set(plain) == {'logdet'} and np.array_equal(plain['logdet'], batch['logdet'])
    monkeypatch.setenv('MXE_FULLMATRIX_LOGDET_SLICES', '1')
    one = run(c, shape, jobs=range(5))
    assert all(np.array_equal(batch[k], one[k]) for k in batch)
    monkeypatch.setenv('MXE_FULLMATRIX_LOGDET_SLICES', '2')
    two = run(c, shape, jobs=range(5))
    assert all(np.array_equal(batch[k], two[k]) for k in batch)


# ---- NaN paths ------------------------------------------------------------------------------------------------------------

def test_a_NaN_in_u_stays_in_its_job(monkeypatch):
    shape = (3, True, 40, 5)
    c = ER.case(shape)
    clean = run(c, shape, jobs=range(3))
    u = np.array(c['u'][:3])
    for bad in (np.nan, np.inf):
        u[1, 4, 2] = bad
        out = run(c, shape, jobs=range(3), u=u)
        for k in out:
            assert np.isnan(out[k][1]) and out[k][0] == clean[k][0] and out[k][2] == clean[k][2], (k, bad)
    # a u that overflows H: that job alone is NaN, also when one workgroup takes all three
    u[1] = c['u'][1]
    u[1, 0] = 1e4
    monkeypatch.setenv('MXE_FULLMATRIX_LOGDET_SLICES', '1')
    out = run(c, shape, jobs=range(3), u=u)
    assert all(np.isnan(out[k][1]) and out[k][0] == clean[k][0] and out[k][2] == clean[k][2] for k in out)


def test_a_pivot_that_is_not_finite_is_NaN():
    """the exit of the Cholesky, reached for certain: the first column of V is constant and job 1 has u = 700 along it, so its
    H = D e^700 = 2.5e303 is finite (the evaluation passes), but c^2 W = 1e8 * 1e304 is not: the first pivot of its B is Inf,
    no positive finite number.  That job is NaN; its neighbours are finite and what they are alone.  (A pivot below zero
    cannot be made for certain: alpha I + c W c is positive definite, and which sign the rounding noise of a singular B takes
    is the compiler's business.)"""
    n_w, n_s = 4, 5
    rng = np.random.RandomState(2)
    V = rng.randn(n_w, n_s)
    V[:, 0] = 1.0
    c = 1e4 * np.ones(n_s)
    D = np.full(n_w, 0.25)
    u = 0.1 * rng.randn(3, 1, n_s)
    u[1, 0] = [700.0, 0.0, 0.0, 0.0, 0.0]
    alpha = np.array([2.0, 0.5, 2.0])
    with np.errstate(over='ignore'):
        H = D * np.exp(np.dot(V, u[1, 0]))
        assert np.all(np.isfinite(H)) and np.isinf(c[0] * c[0] * np.sum(H))
    out = device.fullmatrix_logdet(V, c, D, alpha, u, 1, False)
    for k in out:
        assert np.isnan(out[k][1]) and np.isfinite(out[k][0]) and np.isfinite(out[k][2]), k
    for j in (0, 2):
        alone = device.fullmatrix_logdet(V, c, D, alpha[j:j + 1], u[j:j + 1], 1, False)
        assert all(alone[k][0] == out[k][j] for k in out), j
    assert np.all(out['logdet'][[0, 2]] > 0)


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


def test_evidence_of_the_fixture(solved):
    fm, res, z = solved
    n_w = len(z['omega'])
    conv = np.asarray(res.converged)
    assert conv.sum() >= 6
    default, A_default = res.default_analyzer_name, np.array(res.get_A_out())
    ev = fm.evidence(res)
    print('fixture: kernel %.3f ms; logdet %s; N_g %s; log p %s; classic index %d, ratio %s; log evidence %.6f'
          % (ev['info']['kernel_ms'], ev['logdet'], ev['n_good'], ev['log_probability'], ev['alpha_index_classic'],
             ev['classic_ratio'], ev['log_evidence']))
    assert ev['info']['kernel'] == 'mxe_fullmatrix_logdet' and ev['info']['kernel_ms'] > 0 and not ev['info']['nan_rows']
    assert ev['log_probability'].shape == (8,) and np.all(np.isfinite(ev['log_probability'][conv]))
    idx = int(np.nanargmax(ev['log_probability']))
    assert ev['alpha_index_classic'] == idx
    A = np.asarray(res.A)
    assert np.array_equal(res.get_A_out('ClassicAnalyzer'), A[:, :, idx]) and np.array_equal(ev['A_classic'], A[:, :, idx])
    assert np.array_equal(res.probability, ev['log_probability'])
    assert res.default_analyzer_name == default and np.array_equal(res.get_A_out(), A_default)
    # A_bryan: Hermitian, and positive semi-definite as a convex mixture of positive semi-definite matrices must be
    Ab = ev['A_bryan']
    assert Ab.shape == (2, 2, n_w) and np.array_equal(Ab, np.conj(np.swapaxes(Ab, 0, 1)))
    assert np.isclose(ev['weights'].sum(), 1.0, rtol=1e-13) and np.all(ev['weights'] >= 0)
    pos = matrix_positivity(Ab, delta=np.asarray(fm.omega.delta, dtype=float))
    again = fm.positivity(res, alpha='BryanAnalyzer')
    assert pos['n_negative'] == 0 and again['n_negative'] == 0 and again['alpha'] == 'BryanAnalyzer'
    assert np.array_equal(pos['min_eigenvalue'], again['min_eigenvalue'])
    # the code that is already there takes the new names
    pe = fm.posterior_errors(res, alpha='ClassicAnalyzer', windows=[(-2, 0), (0, 2)])
    assert pe['alpha_index'] == idx and np.all(np.isfinite(pe['window_err'])) and np.all(pe['window_err'] > 0)
    # N_g rises monotonically as alpha falls (the mesh falls), within 0 ... d
    d = 3 * np.asarray(res.v).shape[-1]
    assert np.all(np.diff(np.asarray(res.alpha)) < 0) and np.all(np.diff(ev['n_good']) > 0)
    assert np.all(ev['n_good'] > 0) and np.all(ev['n_good'] < d)
    assert np.all(ev['logdet'] > 0) and np.all(np.diff(ev['logdet']) > 0)
    # the fence
    fm2 = FullMatrixMaxEnt()
    fm2.set_verbosity(mx.VerbosityFlags.Quiet)
    fm2.omega = mx.DataOmegaMesh(z['omega'])
    fm2.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    fm2.set_G_tau_data(z['tau'], z['G_tau_noise'])
    fm2.set_error(float(z['noise']))
    fm2.analyzers = [mx.BryanAnalyzer()]
    with pytest.raises(NotImplementedError, match='BryanAnalyzer'):
        fm2.run()
