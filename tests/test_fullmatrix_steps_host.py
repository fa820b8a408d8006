"""The single-step tests of the whole-matrix solver, the part that needs no GPU: tests/fullmatrix_cases.py is checked with
the numpy truth alone, and so is every condition tests/test_gpu_fullmatrix_steps.py rests on -- that the reference accepts
(or rejects, or halves) the step the device is expected to accept (reject, halve) by a clear margin, that partial pivoting
moves rows in at least one case, and that the gate on the backward error sees the errors it is there for."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fullmatrix_ref as R
import fullmatrix_cases as C

MARGIN = 1e-3                       # a clear change of Q, relative to |Q|; the device's slack is 2^-44 of chi2 / 2 + alpha |S|
PIVOT_CASE = (3, True, 17, 21, 24, False)
MUTATION_CASES = [PIVOT_CASE, C.ACCEPT_CASES[0]]


def test_the_cases_are_the_sizes_they_claim():
    seen = set()
    for case in C.ACCEPT_CASES:
        M, cx, n_s, n_w, n_t, deg = case
        p, args = C.problem(case)
        assert p.P == (M * M if cx else M * (M + 1) // 2) and p.ghat.shape == (p.P, n_s)
        assert args['U'].shape == (n_t, n_s) and args['V'].shape == (n_w, n_s) and args['G'].shape == (M, M, n_t)
        assert np.iscomplexobj(args['G']) == cx and np.array_equal(args['G'], np.conj(np.swapaxes(args['G'], 0, 1)))
        assert np.allclose(np.dot(args['U'].T, args['U']), np.eye(n_s), atol=1e-13)
        assert np.allclose(np.dot(args['V'].T, args['V']), np.eye(n_s), atol=1e-13)
        assert args['S'][0] == 1.0 and (n_s == 1 or np.isclose(args['S'][-1], 1e-4))
        seen.add(p.P * n_s)
    # the orders that matter: the LDS maximum, both sides of 272 (a whole pass of 256 columns to the right of the
    # first panel), below one panel, a last panel of one column
    assert max(seen) == 1024 and 297 in seen and 153 in seen and min(seen) == 6 and 17 in seen
    p1, a1 = C.synthetic_problem(2, True, 5, 9, 8, 4)
    p2, a2 = C.synthetic_problem(2, True, 5, 9, 8, 4)
    assert np.array_equal(a1['G'], a2['G']) and np.array_equal(p1.ghat, p2.ghat)         # seeded


def test_backward_error_and_newton_step():
    rng = np.random.RandomState(0)
    J = rng.randn(30, 30) + 6.0 * np.eye(30)
    x = rng.randn(30)
    F = np.dot(J, x)
    assert C.backward_error(J, F, x) <= 4 * C.EPS
    assert C.backward_error(J, F, np.linalg.solve(J, F)) <= 4 * C.EPS
    # a relative change t of one row of J is a backward error of about t / d
    Jm = J.copy()
    Jm[3] *= 1.0 + 1e-3
    eta = C.backward_error(J, F, np.linalg.solve(Jm, F))
    assert 1e-6 < eta < 1e-3
    case = (2, True, 17, 21, 24, False)
    p, _ = C.problem(case)
    u0 = C.reference_scan(case)['u'][0]
    a1 = C.case_alphas(case)[1]
    s = C.newton_step(p, a1, u0)
    assert np.allclose(np.dot(s['J'], s['delta']), s['F'], rtol=0, atol=1e-12 * np.max(np.abs(s['F'])))
    assert np.array_equal(s['F'], p.F(a1, u0).ravel()) and np.array_equal(s['J'], p.J(a1, u0))
    assert s['Q0'] == p.Q(a1, u0)
    assert s['dQ'][0] == (p.Q(a1, u0 - s['delta'].reshape(u0.shape)) - s['Q0']) / abs(s['Q0'])
    assert s['dQ'][1] == (p.Q(a1, u0 - 0.5 * s['delta'].reshape(u0.shape)) - s['Q0']) / abs(s['Q0'])


@pytest.mark.parametrize('case', C.ACCEPT_CASES, ids=C.case_id)
def test_the_reference_accepts_the_full_step(case):
    """u0: the reference's converged u at a0 = 2 a1; the undamped step at a1 lowers Q by more than MARGIN |Q|, and the
    gate of the device test is printed"""
    ref = C.reference_scan(case)
    s = C.accepted_step(case)
    print(C.gate_row(C.case_id(case), s), ' dQ / |Q| at the full step %.2e,  reference n_iter %s' % (s['dQ'][0], ref['n_iter']))
    assert s['dQ'][0] < -MARGIN
    assert 0.0 < s['eta_ref'] <= 16 * C.EPS                    # LAPACK's own: a small multiple of eps
    assert s['eta_pert'] > 0.0 and s['gate'] == 100.0 * max(s['eta_ref'], s['eta_pert'])
    assert s['gate'] < 1e-8                                    # far below any structural error (the mutations: >= 1e-7)
    if case[5]:
        gaps = np.diff(s['st']['g'], axis=1)
        print('near-degenerate: eigenvalue gaps of Gamma(u0) %.1e to %.1e' % (gaps.min(), gaps.max()))
        assert 1e-12 < gaps.min() and gaps.max() < 1e-7        # every omega: phi by its series, eigenvectors ill-defined


def test_pivoting_moves_rows_in_one_accepted_case():
    s = C.accepted_step(PIVOT_CASE)
    d = s['F'].size
    Pm, _, _ = scipy.linalg.lu(s['J'])
    moved = int(np.sum(np.argmax(Pm, axis=0) != np.arange(d)))
    print('rows moved by partial pivoting: %d of %d' % (moved, d))
    assert moved >= d // 4


@pytest.mark.parametrize('index', range(len(C.REJECT_CASES)))
def test_the_reference_rejects_the_full_step_and_accepts_the_half(index):
    s = C.rejected_step(index)
    print(C.gate_row(C.case_id(s['case']), s), ' dQ / |Q| at 1, 1/2, 1/4: %.3g %.3g %.3g' % tuple(s['dQ']))
    assert s['dQ'][0] > MARGIN and s['dQ'][1] < -MARGIN
    assert s['gate'] < 1e-8
    # from this start and from zero the reference ends at the same minimum
    p, _ = C.problem(s['case'])
    u, _, ok = R.newton(p, s['alpha'], s['u0'])
    uc, _, okc = R.newton(p, s['alpha'], np.zeros_like(s['u0']))
    assert ok and okc and np.max(np.abs(u - uc)) <= 1e-9 * max(1.0, np.max(np.abs(uc)))


def mutations(case):
    """the step of the case solved with a Newton matrix that is wrong in one of the ways the device could be"""
    p, _ = C.problem(case)
    s = C.accepted_step(case)
    J, F, alpha = s['J'], s['F'], s['alpha']
    d, n_s = F.size, case[2]
    out = {}
    # a 16 x 16 tile of the block (p, q) = (0, 1) of c^2 W not written (alpha I is added elsewhere: it stays)
    Jm = J.copy()
    t = min(16, n_s)
    Jm[0:t, n_s:n_s + t] -= (J - alpha * np.eye(d))[0:t, n_s:n_s + t]
    out['a tile of Jb zero'] = np.linalg.solve(Jm, F)
    # the last omega missing from the Gram sums
    L = p.L(s['st'])
    W = np.einsum('is,ipq,it->psqt', p.V[:-1], L[:-1], p.V[:-1])
    Jm = alpha * np.eye(d) + (p.c[None, :, None, None] ** 2 * W).reshape(d, d)
    out['the last omega dropped'] = np.linalg.solve(Jm, F)
    # two rows of U swapped after the factorisation
    Pm, Lm, Um = scipy.linalg.lu(J)
    r = d // 2
    Um[[r, r + 1]] = Um[[r + 1, r]]
    y = scipy.linalg.solve_triangular(Lm, np.dot(Pm.T, F), lower=True, unit_diagonal=True)
    with np.errstate(all='ignore'):
        out['two rows of U swapped'] = np.linalg.solve(Um, y)
    return s, out


@pytest.mark.parametrize('case', MUTATION_CASES, ids=C.case_id)
def test_the_gate_sees_a_wrong_newton_matrix(case):
    s, out = mutations(case)
    for name, delta in out.items():
        eta = C.backward_error(s['J'], s['F'], delta)
        print('%s, %s: eta %.2e, gate %.2e' % (C.case_id(case), name, eta, s['gate']))
        assert not eta <= s['gate'], name
