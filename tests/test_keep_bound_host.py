"""What ``batch_solver.directions_to_keep`` promises when it lets the device solve with 64 or 128 of the kernel's singular
directions, measured on the CPU: the extended-precision fixed point of the kept directions against the one of ALL directions
(oracle/hp_truth.py, at alpha / eta), on the problems of tests/keep_cases.py, whose dropped directions sit just below, just
above and far above the edge of the decision, for both entropies and eta = chi2_factor in {1, 100, 1e4}.  No GPU.

With a bound formed from alpha instead of alpha / eta -- the function before it took ``chi2_factor`` -- the 'far' cases of
eta = 100 and eta = 1e4 are let through and miss the claim (96 x 120, normal entropy: max |delta u| 3.3e-6 and 7.2e-4 against
the 1e-7 of ``KEEP_BOUND``; relative L2 in H 1.7e-7 and 2.0e-5)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_cases as kc                                       # noqa: E402
from maxent_amd import batch_solver as bs                     # noqa: E402

KEEP_BOUND = bs.KEEP_BOUND
H_GATE = 1e-7               # relative L2 in H between the two fixed points: a tenth of the product's parity gate


def decide(c):
    """the decision for the case's job.  (A ``directions_to_keep`` that takes no eta is asked without it, as its callers asked:
    the measurements below then show what it let through, instead of a TypeError.)"""
    import inspect
    kw = dict(chi2_factor=c.eta) if 'chi2_factor' in inspect.signature(bs.directions_to_keep).parameters else {}
    return bs.directions_to_keep(kc.problem(c)['K'], [kc.spec(c)], None, **kw)


def test_keep_bound_is_the_documented_edge():
    assert KEEP_BOUND == 1e-7 and bs.DEVICE_DIRECTIONS == 64


@pytest.mark.parametrize('c', kc.CASES, ids=kc.case_id)
def test_the_cases_sit_where_they_are_designed_to_sit(c):
    """the function's own bound, written out again in keep_cases.own_bound: within a factor 2 below the edge, within a factor 2
    above it, at least ten times above it; with 128 to keep, 64 are never enough"""
    b = kc.own_bound(c)
    print('%s: bound %.3e' % (kc.case_id(c), b))
    if c.position == 'below':
        assert 0.5 * KEEP_BOUND <= b <= KEEP_BOUND
    elif c.position == 'above':
        assert KEEP_BOUND < b <= 2 * KEEP_BOUND
    else:
        assert b >= 10 * KEEP_BOUND
    if c.keep == 128:
        assert kc.own_bound(c, keep=64) >= 10 * KEEP_BOUND
    assert len(kc.problem(c)['K'].S) == kc.SHAPES[c.keep][0] > c.keep
    al = kc.ladder(c)
    assert len(al) == kc.N_LADDER and np.all(np.diff(al) < 0) and al[-1] == c.alpha


@pytest.mark.parametrize('c', kc.CASES, ids=kc.case_id)
def test_a_truncation_that_is_returned_keeps_its_promise(c):
    """Whenever a number comes back: the fixed points of the kept and of all directions differ by max |delta u| <= KEEP_BOUND
    (the docstring's claim) and by <= 1e-7 relative L2 in H, the first-order residual of the dropped directions at the truncated
    H is <= KEEP_BOUND, and |V_k^T H_truth| stays below the function's guess h1.  Where the bound is above the edge: None."""
    keep = decide(c)
    for ia in (0, -1) if keep is not None else ():
        v, H, u = kc.truth(c, ia)
        vt, Ht, ut = kc.truncated(c, ia, keep=keep)
        assert v.shape == (kc.SHAPES[c.keep][0],) and vt.shape == (keep,)
        du = float(np.abs(u - ut).max())
        dH = float(np.linalg.norm(H - Ht) / np.linalg.norm(H))
        res = kc.dropped_residual(c, Ht, keep=keep, ia=ia)
        hk = float(np.abs(np.asarray(kc.problem(c)['K'].V).T @ H).max())
        print('%s alpha[%d]: bound %.3e, max |delta u| %.3e, rel L2 of H %.3e, residual %.3e, max |V_k^T H| %.3e'
              % (kc.case_id(c), ia, kc.own_bound(c) * kc.ladder(c)[-1] / kc.ladder(c)[ia], du, dH, res, hk))
        assert du <= KEEP_BOUND
        assert dH <= H_GATE
        assert res <= KEEP_BOUND
        assert hk <= kc.h1_guess(c)
    assert keep == kc.expected_decision(c), (kc.case_id(c), keep, kc.own_bound(c))


@pytest.mark.parametrize('c', kc.CASES, ids=kc.case_id)
def test_specs_and_arrays_decide_alike(c):
    K = kc.problem(c)['K']
    want = kc.expected_decision(c)
    assert bs.directions_to_keep(K, [kc.spec(c), kc.spec(c)], None, chi2_factor=c.eta) == want
    assert bs.directions_to_keep(K, None, kc.arrays(c), chi2_factor=c.eta) == want
    # the smallest alpha of the job decides, wherever it stands
    up = kc.ladder(c)[::-1].copy()
    assert bs.directions_to_keep(K, [kc.spec(c, alpha=up)], None, chi2_factor=c.eta) == want
    assert bs.directions_to_keep(K, None, kc.arrays(c, alpha=up), chi2_factor=c.eta) == want


@pytest.mark.parametrize('keep', sorted(kc.SHAPES))
def test_eta_enters_as_alpha_over_eta(keep):
    """eta = 1 by default; alpha and eta scaled together change nothing; eta alone moves the 'below' case over the edge"""
    c = kc.find(keep, 'normal', 1.0, 'below')
    K = kc.problem(c)['K']
    assert bs.directions_to_keep(K, [kc.spec(c)], None) == keep
    assert bs.directions_to_keep(K, [kc.spec(c)], None, chi2_factor=1.0) == keep
    assert bs.directions_to_keep(K, [kc.spec(c, alpha=64.0 * kc.ladder(c))], None, chi2_factor=64.0) == keep
    assert bs.directions_to_keep(K, None, kc.arrays(c, alpha=64.0 * kc.ladder(c)), chi2_factor=64.0) == keep
    for eta in (2.0, 100.0, 1e4):
        assert bs.directions_to_keep(K, [kc.spec(c)], None, chi2_factor=eta) is None
        assert bs.directions_to_keep(K, None, kc.arrays(c), chi2_factor=eta) is None
    assert bs.directions_to_keep(K, [kc.spec(c)], None, chi2_factor=0.5) == keep
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert bs.directions_to_keep(K, [kc.spec(c)], None, chi2_factor=bad) is None


@pytest.mark.parametrize('eta', kc.ETAS)
def test_the_refusals_hold_with_eta(eta, monkeypatch):
    """a rotated kernel's U_rot, error bars that vary over the data points and MAXENT_AMD_ALL_DIRECTIONS keep every direction,
    whatever eta (here at an alpha so large that the bound itself would let 64 pass)"""
    c = kc.find(64, 'normal', 1.0, 'below')
    K = kc.problem(c)['K']
    al = 1e3 * eta * kc.ladder(c)
    sp, ar = kc.spec(c, alpha=al), kc.arrays(c, alpha=al)
    n_data = len(sp['G'])
    assert bs.directions_to_keep(K, [sp], None, chi2_factor=eta) == 64
    assert bs.directions_to_keep(K, None, ar, chi2_factor=eta) == 64
    assert bs.directions_to_keep(K, [dict(sp, U_rot=np.eye(n_data))], None, chi2_factor=eta) is None
    vary = kc.SIGMA * (1.0 + 0.1 * np.arange(n_data) / n_data)
    assert bs.directions_to_keep(K, [dict(sp, err=vary)], None, chi2_factor=eta) is None
    assert bs.directions_to_keep(K, None, dict(ar, err=vary[None, :]), chi2_factor=eta) is None
    monkeypatch.setenv('MAXENT_AMD_ALL_DIRECTIONS', '1')
    assert bs.directions_to_keep(K, [sp], None, chi2_factor=eta) is None
    assert bs.directions_to_keep(K, None, ar, chi2_factor=eta) is None
