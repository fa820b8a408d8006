"""Whole-matrix continuation with one error bar per matrix element on the device (mxe_fullmatrix_solve_metric).

The truth is numpy's (tests/fullmatrix_metric_ref.py: ``MetricProblem``); the jobs are those of tests/fullmatrix_cases.py
under the seeded error pattern ``fullmatrix_metric_ref.pattern``; tests/test_fullmatrix_metric_host.py checks, with numpy
alone, the conditions these tests rest on.  Single steps (``maxiter``, ``u0``: the docstring of ``full_matrix_continue``)
are judged as in tests/test_gpu_fullmatrix_steps.py: the backward error of the device's step against the truth's J and F
within ``step_gate`` of the metric problem -- 100 max(eta_ref, eta_pert), both from the truth, nothing from the device --
and max |delta_dev - delta_ref| / max |delta_ref| <= 1e-6, the project's parity gate.  They are the tests that see a wrong
tile of A_p W, R for R^T, or a missed padding; the converged H would not (a slightly wrong J reaches the same fixed point)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd.full_matrix import FullMatrixMaxEnt, full_matrix_continue
import fullmatrix_cases as C
import fullmatrix_metric_ref as MR

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GATE = 1e-6
EPS = np.finfo(float).eps

STEP_CASES = [
    (4, True, 64, 70, 80, False),      # d = 1024, the LDS maximum
    (3, True, 33, 40, 48, False),      # d % 16 = 9: the last column tile of A_p W is part of a tile
    (3, True, 17, 21, 24, False),      # n_s % 16 = 1: the zero-padded row tiles and sums of A_p W
    (2, False, 16, 20, 24, False),     # one full tile
    (3, False, 1, 5, 6, False),        # n_s = 1 (at its A1_FACTOR)
    (1, False, 17, 300, 24, False),    # M = 1: one component
]
END_TO_END_CASES = [(3, True, 17, 21, 24, False), (2, False, 16, 20, 24, False)]


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLD, 'elementwise.npz'))
    return dict((k, z[k]) for k in z.files)


def device(case, alpha, **kwargs):
    _, a = MR.problem(case)
    if 'u0' in kwargs:
        kwargs['u0'] = np.asarray(kwargs['u0'])[None]
    return full_matrix_continue(a['G'][None], a['U'], a['S'], a['V'], a['D'], np.atleast_1d(np.asarray(alpha, dtype=float)),
                                use_complex=a['use_complex'], element_err=a['sigma'], **kwargs)


def matrix_H(st, use_complex):
    H = np.moveaxis(st['Hm'], 0, -1)
    return H if use_complex else H.real


def rel(H, Href):
    return float(np.max(np.abs(H - Href)) / np.max(np.abs(Href)))


def check_step(name, step, delta_dev):
    """the two gates on a step of the device against the step of the truth"""
    eta = C.backward_error(step['J'], step['F'], delta_dev)
    fwd = float(np.max(np.abs(delta_dev - step['delta'])) / np.max(np.abs(step['delta'])))
    print(C.gate_row(name, step, eta, fwd))
    assert eta <= step['gate']
    assert fwd <= GATE


@pytest.mark.parametrize('case', STEP_CASES, ids=C.case_id)
def test_one_accepted_step(case):
    """u0 = the truth's converged u at a0 = 2 a1, maxiter = 1 at a1: u0 - u is the solution of J delta = F"""
    s = MR.accepted_step(case)
    out = device(case, s['alpha'], u0=s['u0'], maxiter=1)
    assert out['n_iter'][0, 0] == 1
    assert np.all(np.isfinite(out['u']))
    check_step(C.case_id(case), s, (s['u0'] - out['u'][0, 0]).ravel())


@pytest.mark.parametrize('index', range(len(C.REJECT_CASES)))
def test_a_rejected_step_leaves_the_start(index):
    """the full step from a bad start makes Q rise; with maxiter = 1 there is no halving: the kernel evaluates u0 again"""
    s = MR.rejected_step(index)
    case = s['case']
    out = device(case, s['alpha'], u0=s['u0'], maxiter=1)
    assert np.array_equal(out['u'][0, 0], s['u0'])                         # bit for bit
    assert out['n_iter'][0, 0] == 1 and not out['converged'][0, 0]
    e = rel(out['H'][0][:, :, 0], matrix_H(s['st'], case[1]))
    print('%s rejected: H(u0) %.2e, chi2 %.15g (%.15g), S %.15g (%.15g)'
          % (C.case_id(case), e, out['chi2'][0, 0], s['st']['chi2'], out['S'][0, 0], s['st']['S']))
    assert e <= GATE
    assert np.isclose(out['chi2'][0, 0], s['st']['chi2'], rtol=1e-9, atol=0)
    assert np.isclose(out['S'][0, 0], s['st']['S'], rtol=1e-9, atol=0)
    assert np.isclose(out['Q'][0, 0], s['Q0'], rtol=1e-9, atol=0)


@pytest.mark.parametrize('index', range(len(C.REJECT_CASES)))
def test_a_halved_step(index):
    """maxiter = 2: the rejected full step, then the same direction half as far, which lowers Q: u = u0 - delta / 2"""
    s = MR.rejected_step(index)
    out = device(s['case'], s['alpha'], u0=s['u0'], maxiter=2)
    assert out['n_iter'][0, 0] == 2 and not out['converged'][0, 0]         # (a halved step never ends an alpha)
    check_step(C.case_id(s['case']) + ' halved', s, 2.0 * (s['u0'] - out['u'][0, 0]).ravel())


@pytest.mark.parametrize('case', END_TO_END_CASES, ids=C.case_id)
def test_end_to_end(case):
    """two alphas from zero against ``MetricProblem.alpha_scan``"""
    ref = MR.reference_scan(case)
    out = device(case, C.case_alphas(case))
    print('%s end to end: n_iter %s (the truth: %s), %.2f ms' % (C.case_id(case), out['n_iter'][0], ref['n_iter'], out['ms']))
    assert out['converged'].all()
    H = out['H'][0]
    Href = ref['H'] if case[1] else ref['H'].real
    for a in range(2):
        e = rel(H[:, :, a], Href[:, :, a])
        print('    alpha %d: max |H - H_truth| / max |H_truth| %.2e' % (a, e))
        assert e <= GATE
    assert np.array_equal(H, np.conj(np.swapaxes(H, 0, 1)))                # exactly Hermitian
    lam = np.linalg.eigvalsh(np.moveaxis(H, (0, 1), (-2, -1)))
    print('    smallest eigenvalue of H %.3e, bound %.3e' % (lam.min(), -16 * EPS * np.max(np.abs(H))))
    assert lam.min() >= -16 * EPS * np.max(np.abs(H))
    assert np.allclose(out['chi2'][0], ref['chi2'], rtol=1e-6) and np.allclose(out['S'][0], ref['S'], rtol=1e-6)


def test_equal_element_errors_against_the_one_error_kernel(fixture):
    """the same problem on the two kernels: other sums (a dense R for a diagonal c), the same minimum"""
    z = fixture
    args = (z['G_tau_noise'][None], z['U'], z['S'], z['V'], z['D'], z['ew_alpha'])
    sigma = float(z['noise'])
    one = full_matrix_continue(*args, err=sigma)
    met = full_matrix_continue(*args, element_err=np.full((2, 2, 201), sigma))
    assert one['converged'].all() and met['converged'].all()
    for a in range(8):
        e = rel(met['H'][0][:, :, a], one['H'][0][:, :, a])
        print('equal errors, alpha %d: max |H_metric - H_one| / max |H_one| %.2e' % (a, e))
        assert e <= 1e-9
    assert np.allclose(met['chi2'], one['chi2'], rtol=1e-9) and np.allclose(met['u'], one['u'], rtol=0, atol=1e-7)
    print('equal errors: kernel %.2f ms (one error), %.2f ms (per element)' % (one['ms'], met['ms']))


def test_block_diagonal_data_decouple_with_their_own_errors(fixture):
    """off-diagonal data zero, sigma_11 = sigma, sigma_22 = 2.5 sigma: the two M = 1 jobs of the one-error path"""
    z = fixture
    G = z['G_tau_noise'].copy()
    G[0, 1] = G[1, 0] = 0.0
    sigma = float(z['noise'])
    err = np.array([[sigma, 3.0 * sigma], [3.0 * sigma, 2.5 * sigma]])
    rest = (z['U'], z['S'], z['V'], z['D'], z['ew_alpha'])
    out = full_matrix_continue(G[None], *rest, element_err=err)
    assert out['converged'].all()
    H = out['H'][0]
    for k, s in ((0, sigma), (1, 2.5 * sigma)):
        one = full_matrix_continue(G[k, k][None, None, None], *rest, err=s)
        assert one['converged'].all()
        e = max(rel(H[k, k, a], one['H'][0, 0, 0, a]) for a in range(8))
        print('decoupling: element (%d, %d) against the M = 1 job at its own error: %.3e' % (k, k, e))
        assert e <= 1e-9
    assert np.all(H[0, 1] == 0.0) and np.all(H[1, 0] == 0.0)


def test_a_problem_does_not_see_its_batch(fixture):
    z = fixture
    G0 = z['G_tau_noise']
    G1 = G0.copy()
    G1[0, 1] = G1[1, 0] = 0.0
    G2 = G0[::-1, ::-1].copy() * 0.8
    rest = (z['U'], z['S'], z['V'], z['D'], z['ew_alpha'][:4])
    sigma = MR.pattern(2, 201)
    batch = full_matrix_continue(np.stack([G0, G1, G2]), *rest, element_err=sigma)
    assert batch['converged'].all()
    for n, G in enumerate((G0, G1, G2)):
        one = full_matrix_continue(G[None], *rest, element_err=sigma)
        for name in ('u', 'H', 'chi2', 'S', 'Q', 'n_iter', 'converged'):
            assert np.array_equal(batch[name][n], one[name][0]), (n, name)


def test_the_class_with_element_errors(fixture):
    z = fixture
    sigma = MR.pattern(2, 201)

    def loaded():
        fm = FullMatrixMaxEnt()
        fm.set_verbosity(mx.VerbosityFlags.Quiet)
        fm.omega = mx.DataOmegaMesh(z['omega'])
        fm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
        fm.set_G_tau_data(z['tau'], z['G_tau_noise'])
        return fm
    fm = loaded()
    fm.set_element_errors(sigma)
    res = fm.run()
    assert fm.last_info['kernel'] == 'mxe_fullmatrix_solve_metric' and np.all(res.converged)
    f1 = loaded()
    f1.set_error(float(z['noise']))
    r1 = f1.run()
    assert f1.last_info['kernel'] == 'mxe_fullmatrix_solve'
    # the layout of the one-error run
    for name in ('A', 'H', 'chi2', 'S', 'Q', 'v', 'alpha', 'G_rec', 'n_iter', 'converged'):
        a, b = np.asarray(getattr(res, name)), np.asarray(getattr(r1, name))
        assert a.shape == b.shape and a.dtype == b.dtype, name
    assert np.array_equal(res.alpha, r1.alpha) and res.get_A_out().shape == (2, 2, 80)
    assert sorted(res.analyzer_results) == sorted(r1.analyzer_results)
    H = np.asarray(res.H)
    assert np.array_equal(H, np.swapaxes(H, 0, 1))
    pos = fm.positivity(res, alpha='all')
    assert np.all(pos['n_negative'] == 0)
    # chi2 is the Frobenius misfit of the symmetrised data under the element errors
    Gs = 0.5 * (z['G_tau_noise'] + np.swapaxes(z['G_tau_noise'], 0, 1))
    direct = np.sum((Gs[:, :, None, :] - np.asarray(res.G_rec)) ** 2 / sigma[:, :, None, :] ** 2, axis=(0, 1, 3))
    print('the class: chi2 %s\n     direct sum %s' % (np.asarray(res.chi2), direct))
    assert np.allclose(res.chi2, direct, rtol=1e-9, atol=0)
    assert np.allclose(res.Q, 0.5 * res.chi2 - res.alpha * res.S, rtol=1e-12)
    assert not np.allclose(res.chi2, r1.chi2, rtol=1e-2)                   # (another problem than the one-error one)
