"""Default-model scans, the part that needs no GPU: the longdouble restatement of ``mxe_evidence_reduce``
(tests/model_scan_ref.py) against a brute-force evaluation, the measure of the evidence integral, the Bryan weights, the
two new default models, every refusal of ``default_model_scan`` that comes before a launch, and the interpretation of the
evidence on the numpy oracle (``oracle/ref_numpy.py``: ``alpha_loop`` + ``log_probability``)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, model_scan, posterior
from oracle import ref_numpy as R
from model_scan_ref import evidence_reduce_ref, brute_force, scan_problem, EPS


def test_symbol_and_wrapper_are_there():
    assert 'mxe_evidence_reduce' in [s[0] for s in device.SYMBOLS]
    assert hasattr(device.DeviceContext, 'evidence_reduce')
    assert hasattr(mx.TauMaxEnt, 'default_model_scan') and hasattr(mx.ElementwiseMaxEnt, 'default_model_scan')
    assert hasattr(mx.MaxEntLoop, 'spec_with_model')


# ---- the reference itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reference_equals_brute_force(seed):
    rng = np.random.RandomState(seed)
    ns, na, nw = 4, 5, 3
    H = 0.5 + rng.rand(ns, na, nw)
    logp = 5.0 * rng.randn(ns, na)
    alpha = np.logspace(1, -1, na)
    log_quad = model_scan.log_measure(alpha)
    log_prior = np.log(np.array([0.1, 0.2, 0.3, 0.4]))
    for log_mix in (np.zeros(na), log_quad):
        ref = evidence_reduce_ref(H, [0, ns], logp, log_quad, log_mix, log_prior)
        bf = brute_force(H, logp, log_quad, log_mix, log_prior)
        assert ref['used'][0] == ns and ref['ngood'].tolist() == [na] * ns
        assert ref['kmax'].tolist() == np.argmax(logp, axis=1).tolist()
        np.testing.assert_allclose(np.asarray(ref['logZ'], dtype=float), bf['logZ'], rtol=0, atol=1e-13)
        for k in ('walpha', 'row', 'wmodel'):
            np.testing.assert_allclose(np.asarray(ref[k], dtype=float), bf[k], rtol=1e-13)
        np.testing.assert_allclose(np.asarray(ref['mean'][0], dtype=float), bf['mean'], rtol=1e-13)
        np.testing.assert_allclose(np.asarray(ref['between'][0], dtype=float), bf['between'], rtol=1e-11, atol=1e-28)
        assert abs(float(ref['wmodel'].sum()) - 1) < 1e-15 and np.all(np.abs(np.asarray(ref['walpha'].sum(axis=1), dtype=float) - 1) < 1e-15)


def test_reference_good_and_usable_rules():
    rng = np.random.RandomState(3)
    ns, na, nw = 5, 4, 6
    H = 0.5 + rng.rand(ns, na, nw)
    logp = rng.randn(ns, na)
    logp[0, 1], logp[0, 2], logp[0, 3] = np.nan, np.inf, -np.inf           # one good alpha is left
    logp[1] = np.nan                                                       # none
    H[2, np.argmax(logp[2])] = np.nan                                      # the row of the largest logp failed
    lq = np.zeros(na)
    ref = evidence_reduce_ref(H, [0, 2, 2, 5], logp, lq, F=np.ones((1, nw)))
    assert ref['ngood'].tolist() == [1, 0, na - 1, na, na] and ref['used'].tolist() == [1, 0, 3]
    assert ref['kmax'][0] == 0 and ref['kmax'][1] == -1 and ref['kmax'][2] != np.argmax(logp[2])
    assert ref['walpha'][0].tolist() == [1, 0, 0, 0] and np.all(ref['walpha'][1] == 0)
    assert ref['logZ'][1] == -np.inf and np.all(np.isnan(np.asarray(ref['row'][1], dtype=float))) and ref['wmodel'][1] == 0
    assert np.all(np.isnan(np.asarray(ref['mean'][1], dtype=float))) and np.all(np.isnan(np.asarray(ref['fcov'][1], dtype=float)))
    # modes 1 and 2: the failed row is CHOSEN there, the scan leaves its group; a negative pick too
    one = evidence_reduce_ref(H, [0, 2, 2, 5], logp, lq, row_mode=1)
    assert one['used'].tolist() == [1, 0, 2] and one['kmax'][2] == np.argmax(logp[2]) and one['wmodel'][2] == 0
    two = evidence_reduce_ref(H, [0, 2, 2, 5], logp, lq, row_mode=2, pick=[0, 0, 0, -1, 3])
    assert two['used'].tolist() == [1, 0, 1 + (np.argmax(logp[2]) != 0)] and two['logZ'][3] == -np.inf
    assert np.array_equal(np.asarray(two['row'][4], dtype=float), H[4, 3])
    # a model that is switched off counts as used and has the weight 0
    off = evidence_reduce_ref(H, [0, 2, 2, 5], logp, lq, log_prior=[0, 0, 0, -np.inf, 0])
    assert off['used'][2] == 3 and off['wmodel'][3] == 0 and abs(float(off['wmodel'][2] + off['wmodel'][4]) - 1) < 1e-15


# ---- measure and weights -----------------------------------------------------------------------------------------------------
def test_log_measure_is_the_trapezoid_on_a_descending_mesh():
    rng = np.random.RandomState(11)
    for alpha in (np.asarray(mx.LogAlphaMesh(1e-2, 1e3, 12), dtype=float) * 40, np.logspace(2, -3, 31)):
        assert np.all(np.diff(alpha) < 0)
        p = rng.rand(len(alpha)) + 0.1
        quad = np.sum(p * np.exp(model_scan.log_measure(alpha)))
        assert abs(quad - abs(np.trapezoid(p, alpha))) <= 8 * EPS * quad
        np.testing.assert_allclose(np.exp(model_scan.log_measure(alpha)), np.abs(mx.analyzers.get_delta(alpha)), rtol=4 * EPS)
    assert model_scan.log_measure([3.0]).tolist() == [0.0]
    with pytest.raises(ValueError):
        model_scan.log_measure([2.0, 2.0, 1.0, 1.0])


def test_weights_over_alpha_are_the_bryan_weights():
    rng = np.random.RandomState(5)
    na = 17
    alpha = np.logspace(2, -2, na)
    H = 0.5 + rng.rand(1, na, 4)
    logp = -60.0 + 30.0 * rng.rand(1, na)
    lq = model_scan.log_measure(alpha)
    good, p = posterior.bryan_weights(logp[0], alpha, True)
    ref = evidence_reduce_ref(H, [0, 1], logp, lq, lq)
    assert good.all()
    np.testing.assert_allclose(np.asarray(ref['walpha'][0], dtype=float), p, rtol=1e-13)
    logp[0, [2, 9]] = np.nan
    good, p = posterior.bryan_weights(logp[0], alpha, False)
    ref = evidence_reduce_ref(H, [0, 1], logp, lq)
    assert np.array_equal(good, np.asarray(ref['walpha'][0], dtype=float) > 0)
    np.testing.assert_allclose(np.asarray(ref['walpha'][0], dtype=float)[good], p, rtol=1e-13)
    np.testing.assert_allclose(np.asarray(ref['row'][0], dtype=float), np.dot(p, H[0][good]), rtol=1e-13)


# ---- the two new default models ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('make', [lambda w: mx.GaussianDefaultModel(w, center=0.3, width=1.5),
                                  lambda w: mx.LorentzianDefaultModel(w, center=-1.0, gamma=0.7),
                                  lambda w: mx.GaussianDefaultModel(w), lambda w: mx.LorentzianDefaultModel(w)])
def test_new_default_models(make):
    omega = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    m = make(omega)
    assert isinstance(m, mx.BaseDefaultModel) and len(m) == 60
    D = np.array(m.D)
    assert D.shape == (60,) and np.all(D > 0) and np.all(np.isfinite(D))
    assert abs(np.sum(D) - 1.0) <= 4 * EPS
    dens = D / omega.delta
    assert abs(np.asarray(omega)[np.argmax(dens)] - m.center) <= np.max(omega.delta)
    # the density is the shape it says it is: ratios to the value at the peak
    x = np.asarray(omega, dtype=float) - m.center
    shape = np.exp(-0.5 * (x / m.width) ** 2) if isinstance(m, mx.GaussianDefaultModel) and not isinstance(m, mx.LorentzianDefaultModel) \
        else 1.0 / (1.0 + (x / m.gamma) ** 2)
    np.testing.assert_allclose(dens / dens.max(), shape / shape.max(), rtol=1e-13)
    # parameter_change: D is kept until it is called, then tabulated again and normalised again
    if isinstance(m, mx.LorentzianDefaultModel):
        m.gamma = 2.0
    else:
        m.width = 0.4
    assert np.array_equal(m.D, D)
    m.parameter_change()
    assert not np.array_equal(m.D, D) and abs(np.sum(m.D) - 1.0) <= 4 * EPS and np.all(m.D > 0)


def test_new_default_models_refuse_nonsense():
    omega = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            mx.GaussianDefaultModel(omega, width=bad)
        with pytest.raises(ValueError):
            mx.LorentzianDefaultModel(omega, gamma=bad)
    with pytest.raises(ValueError):
        mx.GaussianDefaultModel(omega, center=np.nan)


# ---- refusals of default_model_scan that come before any launch -----------------------------------------------------------------
def _tm():
    tau, omega, A, G, models = scan_problem()
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e3, n_points=12)
    tm.set_G_tau_data(tau, G)
    tm.set_error(1e-3)
    return tm, models


def test_default_model_scan_refuses_before_a_launch():
    tm, models = _tm()
    D_before = tm.D
    flat = models[0]
    with pytest.raises(ValueError, match='at least one'):
        tm.default_model_scan([])
    with pytest.raises(ValueError, match='at least one'):
        tm.default_model_scan({})
    with pytest.raises(ValueError, match='points'):
        tm.default_model_scan([flat[:-1]])
    with pytest.raises(ValueError, match='omega mesh'):
        tm.default_model_scan([mx.FlatDefaultModel(mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=61))])
    with pytest.raises(ValueError, match='omega mesh'):
        tm.default_model_scan([mx.FlatDefaultModel(mx.LinearOmegaMesh(omega_min=-8, omega_max=8, n_points=60))])
    for bad in (0.0, -1e-3, np.nan, np.inf):
        D = flat.copy()
        D[7] = bad
        with pytest.raises(ValueError, match='positive'):
            tm.default_model_scan([flat, D])
        with pytest.raises(ValueError, match='positive'):
            tm.default_model_scan({'flat': flat, 'broken': D})
    with pytest.raises(ValueError, match='prior'):
        tm.default_model_scan([flat, flat], prior=[1.0])
    with pytest.raises(ValueError, match='prior'):
        tm.default_model_scan([flat, flat], prior=[1.0, -0.5])
    with pytest.raises(ValueError, match='prior'):
        tm.default_model_scan([flat, flat], prior=[0.0, 0.0])
    with pytest.raises(ValueError, match='prior'):
        tm.default_model_scan([flat, flat], prior=[np.nan, 1.0])
    with pytest.raises(ValueError):
        tm.default_model_scan([flat], alpha='NoSuchAnalyzer')
    with pytest.raises(ValueError):
        tm.default_model_scan([flat], alpha=12)
    assert tm.D is D_before

    class Mine(object):
        def minimize(self, function, v0):
            return v0
    tm.maxent_loop.minimizer = Mine()
    with pytest.raises(NotImplementedError):
        tm.default_model_scan([flat])


def test_prior_and_models_glue():
    assert model_scan.check_prior(None, 3) is None
    lp = model_scan.check_prior([1, 0, 3], 3)
    assert lp[1] == -np.inf and np.allclose(np.exp(lp), [0.25, 0, 0.75])
    omega = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    g = mx.GaussianDefaultModel(omega, width=2.0)
    names, Ds = model_scan.check_models({'g': g, 'flat': mx.FlatDefaultModel(omega).D}, omega)
    assert names == ['g', 'flat'] and np.array_equal(Ds[0], g.D) and Ds[0] is not g.D
    names, Ds = model_scan.check_models([g, g], omega)
    assert names == ['0', '1']
    assert model_scan.choose_rows('bryan', [], 12) == (0, None, None) and model_scan.choose_rows('classic', [], 12) == (1, None, None)
    assert model_scan.choose_rows('LineFitAnalyzer', [], 12) == (2, 0, None) and model_scan.choose_rows(-1, [], 12) == (2, None, 11)


def test_poorman_refuses():
    with pytest.raises(NotImplementedError):
        mx.PoormanMaxEnt.default_model_scan(None, [])


# ---- the interpretation, on the numpy oracle -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle_logZ():
    tau, omega, A, G, models = scan_problem()
    mesh = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    alpha_mesh = np.asarray(mx.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e3, n_points=12), dtype=float)
    out = []
    for D in models:
        p, delta, _, _ = R.make_tau_problem(tau, omega, G, 1e-3 * np.ones(len(tau)), beta=10.0, D=D)
        assert np.array_equal(delta, mesh.delta)
        sc = R.alpha_loop(p, delta, alpha_mesh)
        assert sc['converged'].all()
        logp = np.array([R.log_probability(p, a, v) for a, v in zip(sc['alpha'], sc['v'])])
        ref = evidence_reduce_ref(sc['H'][None], [0, 1], logp[None], model_scan.log_measure(sc['alpha']))
        out.append((float(ref['logZ'][0]), int(ref['kmax'][0]), logp))
    return out


def test_oracle_evidence_prefers_what_it_should(oracle_logZ):
    logZ = np.array([z for z, _, _ in oracle_logZ])
    print('oracle log Z (flat, Gaussians 0.5 1 2 4 8, truth):', np.round(logZ, 2))
    flat, gauss, truth = logZ[0], logZ[1:6], logZ[6]
    assert np.argmax(gauss) == 2                                  # width 2 of {0.5, 1, 2, 4, 8}
    assert gauss[2] - gauss[1] > 1.0 and gauss[2] - gauss[3] > 1.0
    assert truth - flat > 10.0 and np.argmax(logZ) == 6
    # log p of the true-spectrum model peaks at the largest alpha (the first of the mesh): its integral is truncated
    assert oracle_logZ[6][1] == 0
    # the reduction has to be a log-sum-exp: the range of log p within one scan
    assert max(np.ptp(lp) for _, _, lp in oracle_logZ) > 700
