"""The evidence of alpha of the whole-matrix continuation, the parts that need no GPU: the numpy truth
tests/fullmatrix_evidence_ref.py against a dense form of the other order, against the scalar formula and against a
block-diagonal problem, the host glue of ``full_matrix_log_probability`` and ``FullMatrixMaxEnt.evidence`` on a stand-in for the
device, every refusal, and the sensitivity of the gate of the device test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, full_matrix
from maxent_amd.full_matrix import FullMatrixMaxEnt, full_matrix_log_probability
from maxent_amd.model_scan import log_measure
from maxent_amd.probabilities import NormalLogProbability
import fullmatrix_ref as R
import fullmatrix_evidence_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    return dict((k, z[k]) for k in z.files)


# ---- the truth itself ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M,cx,n_w,n_s', [(1, False, 24, 5), (2, True, 30, 8), (3, False, 28, 7), (4, True, 20, 6)])
def test_the_order_d_form_is_the_dense_form(M, cx, n_w, n_s):
    """(a), of order d = P n_s in extended precision, against (c), slogdet of order n_omega P in binary64 with L^1/2 from
    eigh: Sylvester's identity.  They agree to 1e-12 (d + logdet) and 1e-11 d (measured: 1e-15 and 1e-14)."""
    p = ER.make_problem(M, cx, n_w, n_s, seed=11 + M, err=0.02)
    u, alpha = ER.random_u(p, 5 + M), 0.4
    t = ER.truth(p, u, alpha)
    ld, ng = ER.dense_logdet(p, u, alpha)
    e_l, e_n = abs(float(t['logdet']) - ld) / (t['d'] + ld), abs(float(t['n_good']) - ng) / t['d']
    print('M %d complex %d: logdet %.6g (off by %.2e of d + logdet), N_g %.6g of %d (off by %.2e d)'
          % (M, cx, ld, e_l, ng, t['d'], e_n))
    assert e_l <= 1e-12 and e_n <= 1e-11
    assert 0 < float(t['n_good']) < t['d'] and float(t['logdet']) > 0
    b = ER.prototype(p, u, alpha)
    assert abs(b['logdet'] - ld) <= 1e-12 * (t['d'] + ld) and abs(b['n_good'] - ng) <= 1e-11 * t['d']


def test_M1_is_the_scalar_formula():
    """P = 1: L_i = H_i, and the determinant is that of ``NormalLogProbability.evaluate`` with w = H"""
    p = ER.make_problem(1, False, 24, 5, seed=3, err=0.02)
    u = ER.random_u(p, 4)
    H = p.state(u)['Hc'][0]
    assert np.allclose(H, p.D * np.exp(np.dot(p.V, u[0])), rtol=1e-13)
    alpha = np.array([0.3, 40.0])
    Q = np.array([1.5, -2.0])
    lp = NormalLogProbability().evaluate(p.U, p.S, p.V, np.full(len(p.S), p.err), alpha, np.stack([H, H]), Q)
    for k in range(2):
        t = ER.truth(p, u, alpha[k], want_ngood=False)
        mine = NormalLogProbability().from_logdet(float(t['logdet']), alpha[k:k + 1], Q[k:k + 1], len(p.D))[0]
        assert abs(mine - lp[k]) <= 1e-12 * (abs(lp[k]) + t['d']), k


@pytest.mark.parametrize('cx', [False, True])
def test_block_diagonal_Gamma_decouples(cx):
    """the off-diagonal rows of u are zero: Gamma is diagonal, L_i is diagonal in p, with H_1, H_2 for the diagonal units and
    l_i = D_i (e^g1 - e^g2) / (g1 - g2) for the off-diagonal component (twice with ``use_complex``: its real and its imaginary
    part): the determinant is the product of those of the scalar problems with these weights"""
    p = ER.make_problem(2, cx, 26, 6, seed=8, err=0.02)
    u, alpha = ER.random_u(p, 2), 0.5
    u[2:] = 0.0
    t = ER.truth(p, u, alpha)

    def scalar(w):
        A = p.c[:, None] * np.dot(p.V.T * w, p.V) * p.c[None, :]
        lam = np.linalg.eigvalsh(0.5 * (A + A.T))
        return np.linalg.slogdet(np.eye(len(p.c)) + A / alpha)[1], float(np.sum(lam / (lam + alpha)))

    g1, g2 = np.dot(p.V, u[0]), np.dot(p.V, u[1])
    parts = [scalar(p.D * np.exp(g1)), scalar(p.D * np.exp(g2))] + [scalar(p.D * R.phi(g1, g2))] * (2 if cx else 1)
    ld, ng = sum(x[0] for x in parts), sum(x[1] for x in parts)
    assert abs(float(t['logdet']) - ld) <= 1e-12 * (t['d'] + ld)
    assert abs(float(t['n_good']) - ng) <= 1e-11 * t['d']
    assert parts[2][0] > 0.1                                          # (the off-diagonal component is no small part)


@pytest.mark.parametrize('M,cx,n_w,n_s', [(1, False, 24, 5), (3, True, 25, 4)])
def test_N_g_is_the_sum_over_the_eigenvalues(M, cx, n_w, n_s):
    p = ER.make_problem(M, cx, n_w, n_s, seed=2 + M, err=0.02)
    u = ER.random_u(p, 6)
    lam = np.linalg.eigvalsh(ER.curvature(p, u))
    for alpha in (0.05, 3.0, 1e6):
        t = ER.truth(p, u, alpha)
        want = float(np.sum(lam / (lam + alpha)))
        assert abs(float(t['n_good']) - want) <= 1e-11 * t['d'], alpha
        assert abs(ER.prototype(p, u, alpha)['n_good'] - want) <= 1e-9 * t['d'], alpha


# ---- the gate of the device test would see a wrong kernel ---------------------------------------------------------------------

def test_the_gate_sees_three_mistakes():
    """log det B without - d log alpha, c applied once, and W without its blocks p != q are each further from the truth than
    the device may be, on every shape of the device test (the last on every shape that has such blocks, P > 1)"""
    k = ER.k_proto_logdet()
    assert 0.1 < k < 1e3, k
    n_blocks = 0
    for shape in ER.SHAPES:
        c = ER.case(shape)
        t = c['truth']
        allowed = ER.logdet_allowed(k, t)
        wrong = ER.wrong_logdets(c['p'], c['u'][0], ER.ALPHAS[0])
        off = dict((name, abs(v - float(t['logdet'])) / allowed) for name, v in wrong.items() if v is not None)
        print('%s: allowed %.3e; the mistakes are off by %s allowances'
              % (shape, allowed, ', '.join('%s %.3g' % kv for kv in sorted(off.items()))))
        assert off['no_alpha'] > 1 and off['c_once'] > 1, (shape, off)
        assert ('blocks' in off) == (c['p'].P > 1)
        if 'blocks' in off:
            assert off['blocks'] > 1, (shape, off)
            n_blocks += 1
        assert abs(c['proto']['logdet'] - float(t['logdet'])) <= allowed / ER.MARGIN * (1 + 1e-12)
    assert n_blocks == 5


# ---- the entry point and the refusals ---------------------------------------------------------------------------------------

def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert 'mxe_fullmatrix_logdet' in names and 'int  mxe_fullmatrix_logdet(' in header
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_fullmatrix_logdet(' in source and '#include "mxe_fullmatrix_logdet.hip.h"' in source
    hdr = [line for line in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')) if line.startswith('HDR')]
    assert len(hdr) == 1 and 'mxe_fullmatrix_logdet.hip.h' in hdr[0].split()
    assert hasattr(device.load_library(), 'mxe_fullmatrix_logdet')
    assert mx.full_matrix_log_probability is full_matrix.full_matrix_log_probability
    assert 'evidence' in vars(FullMatrixMaxEnt) and 'evidence' not in full_matrix._REFUSED


def _cabi_args(**change):
    n_w, n_s, n_j, P = 6, 3, 2, 3
    a = dict(device=0, n_job=n_j, m=2, is_complex=0, n_omega=n_w, n_s=n_s, V=np.ones((n_w, n_s)), c=np.ones(n_s), D=np.ones(n_w),
             alpha=np.ones(n_j), u=np.zeros((n_j, P, n_s)), want_ngood=1, out_logdet=np.zeros(n_j), out_ngood=np.zeros(n_j))
    a.update(change)
    order = ('device', 'n_job', 'm', 'is_complex', 'n_omega', 'n_s', 'V', 'c', 'D', 'alpha', 'u', 'want_ngood', 'out_logdet',
             'out_ngood')
    return [device._p(a[k]) if isinstance(a[k], np.ndarray) else a[k] for k in order] + [None]


@pytest.mark.parametrize('change,code', [
    (dict(n_job=0), -1), (dict(m=0), -1), (dict(is_complex=2), -1), (dict(n_omega=0), -1), (dict(n_s=0), -1),
    (dict(want_ngood=2), -1), (dict(V=None), -1), (dict(u=None), -1), (dict(out_logdet=None), -1), (dict(out_ngood=None), -1),
    (dict(D=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])), -1), (dict(c=np.array([1.0, -1.0, 1.0])), -1),
    (dict(alpha=np.array([1.0, np.nan])), -1), (dict(alpha=np.array([1.0, 0.0])), -1), (dict(V=np.full((6, 3), np.inf)), -1),
    (dict(m=5), -5), (dict(n_s=65), -5),
])
def test_the_c_interface_refuses_before_the_device(change, code):
    """MXE_ERR_ARG (-1) and MXE_ERR_LIMIT (-5) come before a device is looked for: this runs without one"""
    lib = device.load_library()
    if change.get('n_s') == 65:
        change = dict(change, V=np.ones((6, 65)), c=np.ones(65), u=np.zeros((2, 3, 65)))
    assert lib.mxe_fullmatrix_logdet(*_cabi_args(**change)) == code


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(device, 'load_library', refuse)
    monkeypatch.setattr(device, 'device_count', refuse)


def test_fullmatrix_logdet_refuses_before_the_library(no_library):
    ok = dict(V=np.ones((6, 3)), c=np.ones(3), D=np.ones(6), alpha=np.ones(2), u=np.zeros((2, 3, 3)), m=2, use_complex=False)
    for change in (dict(m=5), dict(m=0), dict(V=np.ones(6)), dict(c=np.ones(4)), dict(D=np.ones(5)), dict(alpha=np.ones((2, 1))),
                   dict(u=np.zeros((1, 3, 3))), dict(u=np.zeros((2, 4, 3))), dict(D=np.array([1.0, 1, 1, 1, 1, np.nan])),
                   dict(alpha=np.array([1.0, 0.0])), dict(c=np.array([1.0, 0.0, 1.0])), dict(use_complex=True)):
        with pytest.raises(ValueError):
            device.fullmatrix_logdet(**dict(ok, **change))
    with pytest.raises(ValueError, match='reduce_singular_space'):
        device.fullmatrix_logdet(**dict(ok, V=np.ones((6, 65)), c=np.ones(65), u=np.zeros((2, 3, 65))))
    # a u that is not finite is no refusal: the library is reached (here: the stand-in that refuses)
    with pytest.raises(AssertionError, match='the library was touched'):
        device.fullmatrix_logdet(**dict(ok, u=np.full((2, 3, 3), np.nan)))


def test_full_matrix_log_probability_refuses(no_library):
    n_t, n_w, n_s = 12, 9, 4
    rng = np.random.RandomState(1)
    U, S, V = np.linalg.qr(rng.randn(n_t, n_s))[0], np.ones(n_s), np.linalg.qr(rng.randn(n_w, n_s))[0]
    ok = dict(u=np.zeros((1, 2, 3, n_s)), U=U, S=S, V=V, D=np.ones(n_w) / n_w, alpha=np.array([1.0, 2.0]), err=0.1,
              Q=np.zeros((1, 2)))
    call = lambda **change: full_matrix_log_probability(**dict(ok, **change))
    for change in (dict(u=np.zeros((2, 3, n_s))), dict(alpha=np.ones(3)), dict(u=np.zeros((1, 2, 2, n_s))),
                   dict(u=np.zeros((1, 2, 3, n_s + 1))), dict(err=np.ones((2, 2, n_t))), dict(err=-1.0), dict(err=np.ones(n_t - 1)),
                   dict(Q=np.zeros(2)), dict(Q=np.zeros((2, 1))), dict(S_entropy=np.zeros(2)), dict(alpha=np.array([1.0, 1.0])),
                   dict(alpha=np.array([1.0, -2.0]))):
        with pytest.raises(ValueError):
            call(**change)
    with pytest.raises(NotImplementedError, match='matrix-valued'):
        call(D=np.ones((2, 2, n_w)))
    with pytest.raises(AssertionError, match='the library was touched'):
        call()


# ---- the glue, on a stand-in for the device -------------------------------------------------------------------------------------

def truth_logdet(V, c, D, alpha, u, m, use_complex, want_ngood=True, device=0, timing=None):
    """``device.fullmatrix_logdet`` from the extended-precision truth; a u with a NaN gives NaN, as on the device"""
    n_s = len(c)
    p = R.Problem(np.eye(n_s), c, V, np.zeros((m, m, n_s)), 1.0, D, use_complex)
    out = dict(logdet=np.full(len(alpha), np.nan), n_good=np.full(len(alpha), np.nan))
    for j in range(len(alpha)):
        if np.all(np.isfinite(u[j])):
            t = ER.truth(p, u[j], alpha[j])
            out['logdet'][j], out['n_good'][j] = float(t['logdet']), float(t['n_good'])
    if timing is not None:
        timing['ms'] = 0.25
    return out


def small_job(n_prob=2, n_alpha=5, use_complex=False, seed=1):
    n_t, n_w, n_s, P = 12, 9, 4, 4 if use_complex else 3
    rng = np.random.RandomState(seed)
    U, S, V = np.linalg.qr(rng.randn(n_t, n_s))[0], 10.0 ** -np.arange(n_s), np.linalg.qr(rng.randn(n_w, n_s))[0]
    return dict(u=0.4 * rng.randn(n_prob, n_alpha, P, n_s), U=U, S=S, V=V, D=np.ones(n_w) / n_w,
                alpha=np.geomspace(50.0, 0.05, n_alpha), err=0.05, Q=rng.rand(n_prob, n_alpha) * 3, use_complex=use_complex)


@pytest.mark.parametrize('cx', [False, True])
def test_full_matrix_log_probability_on_the_stand_in(monkeypatch, cx):
    monkeypatch.setattr(device, 'fullmatrix_logdet', truth_logdet)
    job = small_job(use_complex=cx)
    S_ent = -np.abs(np.random.RandomState(4).randn(2, 5))
    out = full_matrix_log_probability(S_entropy=S_ent, **job)
    al, n_w, P = job['alpha'], 9, job['u'].shape[2]
    assert set(out) == {'alpha', 'logdet', 'n_good', 'log_probability', 'alpha_index_classic', 'weights', 'classic_ratio',
                        'log_evidence', 'alpha_at_edge', 'info'}
    for k in ('logdet', 'n_good', 'log_probability', 'weights', 'classic_ratio'):
        assert out[k].shape == (2, 5), k
    for k in ('alpha_index_classic', 'log_evidence', 'alpha_at_edge'):
        assert out[k].shape == (2,), k
    assert out['info'] == dict(kernel='mxe_fullmatrix_logdet', kernel_ms=0.25, nan_jobs=[])
    assert np.array_equal(out['alpha'], al)
    p = R.Problem(np.eye(4), job['S'] / job['err'], job['V'], np.zeros((2, 2, 4)), 1.0, job['D'], cx)
    for n in range(2):
        for a in range(5):
            assert out['logdet'][n, a] == float(ER.truth(p, job['u'][n, a], al[a], want_ngood=False)['logdet'])
    lp = -0.5 * out['logdet'] - job['Q'] - np.log(al)
    assert np.allclose(out['log_probability'], lp, rtol=1e-14, atol=0)
    assert np.array_equal(out['alpha_index_classic'], np.argmax(lp, axis=1))
    w = np.exp(lp - lp.max(axis=1, keepdims=True))
    assert np.allclose(out['weights'], w / w.sum(axis=1, keepdims=True), rtol=1e-13) and np.allclose(out['weights'].sum(axis=1), 1)
    assert np.allclose(out['classic_ratio'], -2 * al * S_ent / out['n_good'], rtol=1e-14)
    assert np.allclose(out['log_evidence'], np.log(np.sum(np.exp(lp + log_measure(al)), axis=1)), rtol=1e-12)
    assert np.array_equal(out['alpha_at_edge'], np.isin(np.argmax(lp, axis=1), (0, 4)))
    assert 'classic_ratio' not in full_matrix_log_probability(**job)
    # a problem alone is the problem in the batch; one alpha: the measure is one
    one = full_matrix_log_probability(**dict(job, u=job['u'][1:], Q=job['Q'][1:]))
    assert np.array_equal(one['log_probability'][0], out['log_probability'][1]) and one['log_evidence'][0] == out['log_evidence'][1]
    single = full_matrix_log_probability(**dict(job, u=job['u'][:, 2:3], Q=job['Q'][:, 2:3], alpha=al[2:3]))
    assert np.allclose(single['log_evidence'], single['log_probability'][:, 0], rtol=1e-14) and np.all(single['alpha_at_edge'])
    # a custom probability sees P n_omega unknowns
    seen = []
    prob = NormalLogProbability(log_norm_S=lambda a, n: seen.append(n) or 0.0, log_prior_alpha=lambda a: -2.0 * np.log(a))
    cust = full_matrix_log_probability(probability=prob, **job)
    assert set(seen) == {P * n_w}
    assert np.allclose(cust['log_probability'], -0.5 * out['logdet'] - job['Q'] - (P * n_w / 2.0 + 2.0) * np.log(al), rtol=1e-13)


def test_a_NaN_row_is_skipped(monkeypatch):
    monkeypatch.setattr(device, 'fullmatrix_logdet', truth_logdet)
    job = small_job()
    clean = full_matrix_log_probability(**job)
    best = int(clean['alpha_index_classic'][0])
    u = np.array(job['u'])
    u[0, best, 1, 2] = np.nan                                        # the classic alpha of problem 0
    u[1] = np.nan                                                    # and every alpha of problem 1
    out = full_matrix_log_probability(**dict(job, u=u))
    assert out['info']['nan_jobs'] == [(0, best)] + [(1, a) for a in range(5)]
    lp = np.delete(clean['log_probability'][0], best)
    keep = np.delete(np.arange(5), best)
    assert np.isnan(out['log_probability'][0, best]) and np.array_equal(out['log_probability'][0, keep], lp)
    assert out['alpha_index_classic'][0] == keep[np.argmax(lp)] and out['weights'][0, best] == 0.0
    assert np.allclose(out['weights'][0, keep], np.exp(lp - lp.max()) / np.sum(np.exp(lp - lp.max())), rtol=1e-13)
    assert np.isclose(out['log_evidence'][0], np.log(np.sum(np.exp(lp + log_measure(job['alpha'])[keep]))), rtol=1e-12)
    assert out['alpha_index_classic'][1] == -1 and np.all(np.isnan(out['weights'][1])) and np.isnan(out['log_evidence'][1])
    assert not out['alpha_at_edge'][1]


def solve_stand_in(V, c, D, alpha, ghat, cperp, m, use_complex, u0=None, maxiter=1000, tol_h=1e-9, device=0, timing=None):
    """``device.fullmatrix_solve`` without a solve: a seeded random u per alpha and everything of it from the numpy truth"""
    n_s, n_a = len(c), len(alpha)
    p = R.Problem(np.eye(n_s), c, V, np.zeros((m, m, n_s)), 1.0, D, use_complex)
    u = 0.3 * np.random.RandomState(9).randn(1, n_a, p.P, n_s) / (1.0 + np.arange(n_s))
    st = [p.state(u[0, a]) for a in range(n_a)]
    H = np.stack([np.moveaxis(s['Hm'], 0, -1) for s in st], axis=2)[None]              # (1, M, M, n_alpha, n_omega)
    S = np.array([[s['S'] for s in st]])
    chi2 = np.array([[40.0 + 3.0 / a for a in alpha]])
    if timing is not None:
        timing['ms'] = 1.0
    return dict(u=u, H=H if use_complex else H.real, chi2=chi2, S=S, Q=0.5 * chi2 - np.asarray(alpha) * S,
                n_iter=np.full((1, n_a), 3, dtype=np.int32), converged=np.ones((1, n_a), dtype=bool))


def loaded(fixture, **kw):
    fm = FullMatrixMaxEnt(**kw)
    fm.set_verbosity(mx.VerbosityFlags.Quiet)
    fm.omega = mx.DataOmegaMesh(fixture['omega'][::4])
    fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=6)
    fm.set_G_tau_data(fixture['tau'], fixture['G_tau_noise'])
    fm.set_error(float(fixture['noise']))
    fm.reduce_singular_space = 1e-6
    return fm


def test_evidence_attaches_what_it_says(fixture, monkeypatch):
    monkeypatch.setattr(device, 'fullmatrix_solve', solve_stand_in)
    monkeypatch.setattr(device, 'fullmatrix_logdet', truth_logdet)
    fm = loaded(fixture)
    res = fm.run()
    n_w = len(fixture['omega'][::4])
    assert np.all(np.isnan(res.probability)) and set(res.analyzer_results) >= {'LineFitAnalyzer'}
    before, default = set(res.analyzer_results), res.default_analyzer_name
    A_default = np.array(res.get_A_out())
    ev = fm.evidence(res, attach=False)
    assert np.all(np.isnan(res.probability)) and set(res.analyzer_results) == before          # nothing was attached
    assert set(ev) == {'alpha', 'logdet', 'n_good', 'log_probability', 'alpha_index_classic', 'weights', 'classic_ratio',
                       'log_evidence', 'alpha_at_edge', 'A_classic', 'A_bryan', 'info'}
    for k in ('logdet', 'n_good', 'log_probability', 'weights', 'classic_ratio', 'alpha'):
        assert np.shape(ev[k]) == (6,), k
    for k in ('alpha_index_classic', 'log_evidence', 'alpha_at_edge'):
        assert np.shape(ev[k]) == (), k
    assert ev['A_classic'].shape == (2, 2, n_w) and ev['A_bryan'].shape == (2, 2, n_w)
    assert ev['info'] == dict(kernel='mxe_fullmatrix_logdet', kernel_ms=0.25, nan_rows=[])
    assert np.array_equal(ev['alpha'], res.alpha)
    lp = -0.5 * ev['logdet'] - np.asarray(res.Q) - np.log(np.asarray(res.alpha))
    assert np.allclose(ev['log_probability'], lp, rtol=1e-14)
    idx = int(np.argmax(lp))
    A = np.asarray(res.A)
    assert ev['alpha_index_classic'] == idx and np.array_equal(ev['A_classic'], A[:, :, idx])
    assert np.array_equal(ev['A_bryan'], np.einsum('k,abki->abi', ev['weights'], A))
    assert np.allclose(ev['A_bryan'], sum(ev['weights'][k] * A[:, :, k] for k in range(6)), rtol=1e-13, atol=1e-300)
    assert np.allclose(ev['classic_ratio'], -2 * np.asarray(res.alpha) * np.asarray(res.S) / ev['n_good'], rtol=1e-14)
    assert np.all(ev['n_good'] > 0) and np.all(np.diff(ev['n_good']) > 0)          # the mesh falls: N_g rises as alpha falls
    # attach (the default)
    ev2 = fm.evidence(res)
    assert all(np.array_equal(ev[k], ev2[k]) for k in ev if k != 'info')
    assert np.array_equal(res.probability, ev['log_probability'])
    assert set(res.analyzer_results) == before | {'ClassicAnalyzer', 'BryanAnalyzer'}
    cl, br = res.analyzer_results['ClassicAnalyzer'], res.analyzer_results['BryanAnalyzer']
    assert cl['name'] == 'ClassicAnalyzer' and cl['alpha_index'] == idx and isinstance(cl['info'], str)
    assert br['name'] == 'BryanAnalyzer' and 'alpha_index' not in br and isinstance(br['info'], str)
    assert np.array_equal(res.get_A_out('ClassicAnalyzer'), A[:, :, idx])
    assert np.array_equal(res.get_A_out('BryanAnalyzer'), ev['A_bryan'])
    assert res.default_analyzer_name == default and np.array_equal(res.get_A_out(), A_default)
    # what the classic analyzer of the scalar path makes of the attached probability
    own = mx.ClassicAnalyzer().analyze(res)
    assert own['alpha_index'] == idx and np.array_equal(own['A_out'], cl['A_out'])
    # the code that is already there takes the names
    from maxent_amd.posterior import choose_alpha
    assert choose_alpha('ClassicAnalyzer', 6, res.analyzer_results, default) == ([idx], 'one')
    # the default result of evidence() is that of run()
    assert np.array_equal(fm.evidence()['logdet'], ev['logdet'])


def test_evidence_skips_a_NaN_row(fixture, monkeypatch):
    monkeypatch.setattr(device, 'fullmatrix_solve', solve_stand_in)
    fm = loaded(fixture)
    res = fm.run()

    def with_a_NaN(V, c, D, alpha, u, *a, **k):
        u = np.array(u)
        u[2, 0, 0] = np.nan
        return truth_logdet(V, c, D, alpha, u, *a, **k)
    monkeypatch.setattr(device, 'fullmatrix_logdet', truth_logdet)
    clean = fm.evidence(res, attach=False)
    monkeypatch.setattr(device, 'fullmatrix_logdet', with_a_NaN)
    ev = fm.evidence(res)
    assert ev['info']['nan_rows'] == [2] and np.isnan(ev['log_probability'][2]) and ev['weights'][2] == 0.0
    keep = [0, 1, 3, 4, 5]
    assert np.isclose(ev['weights'][keep].sum(), 1.0) and np.all(np.isfinite(ev['A_bryan']))
    assert np.array_equal(ev['log_probability'][keep], clean['log_probability'][keep])
    assert ev['alpha_index_classic'] == keep[int(np.argmax(clean['log_probability'][keep]))]
    assert np.isnan(res.probability[2]) and res.analyzer_results['ClassicAnalyzer']['alpha_index'] == ev['alpha_index_classic']


def test_evidence_of_a_result_that_is_NaN_at_every_alpha(fixture, monkeypatch):
    monkeypatch.setattr(device, 'fullmatrix_solve', solve_stand_in)
    monkeypatch.setattr(device, 'fullmatrix_logdet', lambda V, c, D, alpha, u, *a, **k: truth_logdet(V, c, D, alpha, u * np.nan, *a, **k))
    fm = loaded(fixture)
    res = fm.run()
    before = set(res.analyzer_results)
    with pytest.raises(ValueError, match='NaN at every alpha'):
        fm.evidence(res)
    assert np.all(np.isnan(res.probability)) and set(res.analyzer_results) == before          # nothing was attached


def test_evidence_refuses(fixture, no_library, monkeypatch):
    fm = loaded(fixture)
    fm.set_element_errors(np.full((2, 2), float(fixture['noise'])))
    with pytest.raises(NotImplementedError, match='set_element_errors'):
        fm.evidence(result=object())
    # a result of another alpha mesh
    monkeypatch.setattr(device, 'fullmatrix_solve', solve_stand_in)
    fm = loaded(fixture)
    res = fm.run()
    fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=7)
    with pytest.raises(ValueError, match='alpha mesh'):
        fm.evidence(res)
    # the fence: run() still refuses the probability-based analyzers, the constructor probability=
    fm = loaded(fixture)
    fm.analyzers = [mx.BryanAnalyzer()]
    with pytest.raises(NotImplementedError, match='BryanAnalyzer'):
        fm.run()
    with pytest.raises(NotImplementedError, match='probability'):
        FullMatrixMaxEnt(probability='normal')
    assert 'default_model_scan' in full_matrix._REFUSED
