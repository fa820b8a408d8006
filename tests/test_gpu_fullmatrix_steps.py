"""One Newton step of the whole-matrix solver on the device (mxe_fullmatrix_solve), at its size limits.

The converged H says nothing about the Newton matrix: an iteration with a slightly wrong J reaches the same fixed point
with more steps or more damping.  ``full_matrix_continue(..., u0=, maxiter=)`` shows single steps (its docstring): with
``maxiter=1`` an accepted full step returns u0 - delta with J delta = F, which is the device's assembly of J and F and
its blocked LU, observable directly; a rejected one returns u0; ``maxiter=2`` shows a halved step.  The truth of every
step is numpy's (tests/fullmatrix_cases.py over tests/fullmatrix_ref.py); tests/test_fullmatrix_steps_host.py checks, with
numpy alone, the conditions these tests rest on.

Two gates on a step delta_dev = u0 - u_dev.  The backward error against the reference's J and F,
eta = ||J delta - F||_inf / (||J||_inf ||delta||_inf + ||F||_inf), within 100 max(eta_ref, eta_pert): eta_ref is LAPACK's
own on the same system, eta_pert that of the step solved at u0 (1 +- eps) -- both from the reference, never from the
device; a structural error of J or of the solve shows at 1e-6 or more (the mutations of the host test), rounding at a
small multiple of eps.  And the project's parity gate, max |delta_dev - delta_ref| / max |delta_ref| <= 1e-6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from maxent_amd.full_matrix import full_matrix_continue
import fullmatrix_ref as R
import fullmatrix_cases as C

pytestmark = pytest.mark.gpu

GATE = 1e-6
EPS = np.finfo(float).eps


def device(case, alpha, **kwargs):
    _, a = C.problem(case)
    if 'u0' in kwargs:
        kwargs['u0'] = np.asarray(kwargs['u0'])[None]
    return full_matrix_continue(a['G'][None], a['U'], a['S'], a['V'], a['D'], np.atleast_1d(np.asarray(alpha, dtype=float)),
                                a['err'], use_complex=a['use_complex'], **kwargs)


def matrix_H(st, use_complex):
    """H (M, M, n_omega) of a state of the reference"""
    H = np.moveaxis(st['Hm'], 0, -1)
    return H if use_complex else H.real


def rel(H, Href):
    return float(np.max(np.abs(H - Href)) / np.max(np.abs(Href)))


def check_step(name, step, delta_dev):
    """the two gates on a step of the device against the step of the reference"""
    eta = C.backward_error(step['J'], step['F'], delta_dev)
    fwd = float(np.max(np.abs(delta_dev - step['delta'])) / np.max(np.abs(step['delta'])))
    print(C.gate_row(name, step, eta, fwd))
    assert eta <= step['gate']
    assert fwd <= GATE


@pytest.mark.parametrize('case', C.ACCEPT_CASES, ids=C.case_id)
def test_one_accepted_step(case):
    """u0 = the reference's converged u at 2 a1, maxiter = 1 at a1: u0 - u is the solution of J delta = F"""
    s = C.accepted_step(case)
    out = device(case, s['alpha'], u0=s['u0'], maxiter=1)
    assert out['n_iter'][0, 0] == 1
    assert np.all(np.isfinite(out['u']))
    check_step(C.case_id(case), s, (s['u0'] - out['u'][0, 0]).ravel())


@pytest.mark.parametrize('index', range(len(C.REJECT_CASES)))
def test_a_rejected_step_leaves_the_start(index):
    """the full step from a bad start makes Q rise; with maxiter = 1 there is no halving: the kernel evaluates u0 again"""
    s = C.rejected_step(index)
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
    s = C.rejected_step(index)
    out = device(s['case'], s['alpha'], u0=s['u0'], maxiter=2)
    assert out['n_iter'][0, 0] == 2 and not out['converged'][0, 0]         # (a halved step never ends an alpha)
    check_step(C.case_id(s['case']) + ' halved', s, 2.0 * (s['u0'] - out['u'][0, 0]).ravel())


@pytest.mark.parametrize('index', range(len(C.REJECT_CASES)))
def test_from_a_bad_start_to_the_same_minimum(index):
    s = C.rejected_step(index)
    case = s['case']
    p, _ = C.problem(case)
    u, n, ok = R.newton(p, s['alpha'], s['u0'])
    uc, nc, okc = R.newton(p, s['alpha'], np.zeros_like(s['u0']))
    assert ok and okc
    out = device(case, s['alpha'], u0=s['u0'])
    print('%s from a bad start: n_iter %d (the reference: %d accepted steps; from zero %d)'
          % (C.case_id(case), out['n_iter'][0, 0], n, nc))
    assert out['converged'][0, 0]
    H = out['H'][0][:, :, 0]
    for what, ur in (('that start', u), ('zero', uc)):
        e = rel(H, matrix_H(p.state(ur), case[1]))
        print('    max |H - H_ref| / max |H_ref|, the reference from %s: %.2e' % (what, e))
        assert e <= GATE


@pytest.mark.parametrize('case', C.LIMIT_CASES, ids=C.case_id)
def test_end_to_end_at_the_limit(case):
    """n_s = 64, M = 4: two alphas from zero"""
    ref = C.reference_scan(case)
    out = device(case, C.case_alphas(case))
    print('%s end to end: n_iter %s (the reference: %s), %.1f ms' % (C.case_id(case), out['n_iter'][0], ref['n_iter'], out['ms']))
    assert out['converged'].all()
    H = out['H'][0]
    Href = ref['H'] if case[1] else ref['H'].real
    for a in range(2):
        e = rel(H[:, :, a], Href[:, :, a])
        print('    alpha %d: max |H - H_ref| / max |H_ref| %.2e' % (a, e))
        assert e <= GATE
    assert np.array_equal(H, np.conj(np.swapaxes(H, 0, 1)))                # exactly Hermitian
    lam = np.linalg.eigvalsh(np.moveaxis(H, (0, 1), (-2, -1)))
    print('    smallest eigenvalue of H %.3e, bound %.3e' % (lam.min(), -16 * EPS * np.max(np.abs(H))))
    assert lam.min() >= -16 * EPS * np.max(np.abs(H))
    # the device stops on a step-size rule at tol_h = 1e-9, the reference on a residual of 1e-11: with quadratic convergence
    # that is one step either way; a Newton matrix that is off needs more
    assert np.all(out['n_iter'][0] <= ref['n_iter'] + 3)
