"""Every reachable build of the one-chain kernel, chain_kernel<NW, NAB, TS, GST> (maxent_amd/csrc/mxe_kernel.hip.h),
at the shapes where its code changes -- against extended precision, not against another kernel.  The one-chain kernel is what
the other GPU tests accept the lock-step kernels, chain_kernel_lv, the two-pass mode and the finishing pass by; its own truth
tests ran on the synthetic fermionic job only (n_s = 51 ... 56, 18 ... 29 coupled directions: the 24- and 32-row classes of the
register solves).  tests/one_chain_cases.py lists the cases and the edge each stands for:

    <NW, 2, double>, NW = 1, 2, 4   the 16-row class, 16 | 17, 24 | 25, 32 | 33 (register solve | gj_solve_4w with four waves,
                                    fused chol_solve with one or two), 48 | 49 (block edge of gj_solve_4w, three | four tiles of
                                    gram_mfma), 63 (last fused row), 64 (n_act == NP: unfused chol_solve)
    <1, 4, double>                  65 (fused, 6 super-block pairs of the VALU gram_sweep), 96 | 97 (6 | 10 pairs: two sweeps of
                                    three, three sweeps and a single), 128 (unfused) -- state in LDS and in device memory
    <4, 2, double / float, device-memory state>, <NW, 2, float>

1. ONE Newton step.  A damped Newton iteration corrects its own solver: an elimination that mishandles a row, a Gram tile
summed from the wrong place, still reaches the fixed point, in more iterations, and passes every gate on H.  So the kernel
takes ONE iteration (maxiter = 1) from a start vector of the host's -- the numpy model's v of the alpha before -- with the
whole n_s block coupled (decouple_tol = 0), on a spectrum where every direction counts, and v0 - v is compared with the step
in extended precision (tests/newton_step_ref.py).  tests/test_newton_step_ref_host.py asserts what this relies on: the step is
within Bryan's bound (so it is neither shortened nor damped), the reference is good to 1e-14, one row left out of the solve
moves the step by >= 1e-6 of its length -- the gate on a binary64 build is 1e-9 --, and the gate of a binary32 build, ten
times what its stream arithmetic costs on the host, is a tenth of that change at most.

2. The scans of the same shapes, twelve alphas warm, against the extended-precision fixed point reached from the oracle's
iterates (tests/anchor.py), with the default decouple_tol and with 0 ("full n_s block", include/maxent_hip.h), at the project's
own gates: 1e-6 on H and on the device audit in binary64, 1e-4 in binary32.

3. The reference's stopping rule (tol_d: max |W g|) on blocks of 33 and 97 rows, where symv runs over more than 32.

What none of this reaches: the damped solutions of gj_solve_spec (waves 1 ... 3 solve for mu_1, mu_1 g, mu_1 g^2) are used only
when a trial is refused, which these inputs are built to avoid; they stay covered through cold starts that converge."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor                                                # noqa: E402
import newton_step_ref as N                                  # noqa: E402
import one_chain_cases as C                                  # noqa: E402
from maxent_amd import device                                # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
assert device.PRECISION_F32 == 1
WORST = {}                               # build -> worst step error / gate so far (printed with every case)


def context(j):
    ctx = device.DeviceContext(j.U, j.S, j.V)
    ds = ctx.add_dataset(j.err)
    ctx.set_elements([ds, ds], j.G, np.tile(j.D, (2, 1)), KINDS)
    return ctx


def launch(ctx, alphas, v0, **opts):
    """one launch, no finishing pass (it would solve the alphas again): the records of the launch alone"""
    ctx.upload_chains([0, 1], alphas, v0, device.default_opts(**opts))
    ctx.launch()
    out = ctx.fetch(want_v=True, want_H=True)
    out['H'] = np.array(out['H'])
    out['kernel'] = ctx.last_launch_info()['kernel']
    out['n_act'] = ctx.fetch_n_act()
    return out


def host_values_gate(j, e, v, H, chi2, S, f32, label):
    """H, chi2 and S of the record against the host's at the returned v (as test_chain_matches_kernel_model_and_truth does)"""
    Hr, chi2r, Sr = j.values_at(e, v)
    tol_H, tol = (1e-4, 2e-3) if f32 else (1e-10, 1e-8)
    assert np.all(np.isfinite(H)) and np.isfinite(chi2) and np.isfinite(S), label
    assert np.linalg.norm(Hr - H) / np.linalg.norm(Hr) < tol_H, (label, np.linalg.norm(Hr - H) / np.linalg.norm(Hr))
    assert abs(chi2r - chi2) / chi2 < tol, (label, chi2r, chi2)
    assert abs(Sr - S) < tol * max(1.0, abs(S)), (label, Sr, S)


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_one_newton_step_of_every_build(case):
    name, opts, n_omega, n_s = case
    f32 = 'float' in name
    j = C.job(n_omega, n_s)
    ctx = context(j)
    worst = 0.0
    try:
        for ia in C.STEP_ROWS:
            refs = [C.step_ref(n_omega, n_s, e, ia) for e in range(2)]
            v0 = np.stack([r['v0'] for r in refs])
            o = launch(ctx, j.alphas[ia:ia + 1], v0, maxiter=1, decouple_tol=0.0, alpha_split=1, **opts)
            assert o['kernel'] == name, (o['kernel'], name)
            for e in range(2):
                label = '%s n_omega=%d n_s=%d %s alpha[%d]' % (name, n_omega, n_s, C.ENTROPIES[e], ia)
                assert o['n_act'][e, 0] == n_s, (label, o['n_act'][e, 0])
                assert o['n_evals'][e, 0] == 2, (label, o['n_evals'][e, 0])      # the start + one trial, accepted at mu = 0
                assert o['n_iter'][e, 0] == 1, (label, o['n_iter'][e, 0])
                delta = v0[e] - o['v'][e, 0]
                err = N.rel_err(delta, refs[e]['delta'])
                gate = C.f32_step_gate(n_omega, n_s, e, ia) if f32 else C.F64_STEP_GATE
                worst = max(worst, err / gate)
                print('%s: step error %.2e of |delta|, gate %.2e' % (label, err, gate))
                assert np.isfinite(err) and err < gate, (label, err, gate)
                host_values_gate(j, e, o['v'][e, 0], o['H'][e, 0], o['chi2'][e, 0], o['S'][e, 0], f32, label)
    finally:
        ctx.close()
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print('%s n_omega=%d n_s=%d: worst step error / gate %.3g (this build so far: %.3g)' % (name, n_omega, n_s, worst, WORST[name]))


@functools.lru_cache(maxsize=None)
def truths(n_omega, n_s):
    """{element: {alpha index: H of the extended-precision fixed point}}, from the oracle's own scan -- which has to converge"""
    j = C.job(n_omega, n_s)
    out = {}
    for e, ent in enumerate(C.ENTROPIES):
        out[e], ref = anchor.truth_rows(j.problem(e), j.delta, j.alphas, j.n_tau, C.TRUTH_ROWS, ent)
        assert ref['converged'].all(), ('the oracle does not converge on this problem', n_omega, n_s, ent)
    return out


def truth_error(n_omega, n_s, o):
    return max(anchor.rel_l2_checked(o['H'][e, ia], Ht) for e, rows in truths(n_omega, n_s).items() for ia, Ht in rows.items())


def scan(ctx, j, **opts):
    v0 = np.stack([j.initial_v(e) for e in range(2)])
    o = launch(ctx, j.alphas, v0, alpha_split=1, **opts)
    o['audit'] = ctx.audit()['corr']
    return o


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


@pytest.mark.parametrize('case', C.SCAN_CASES, ids=C.case_id)
def test_scans_of_every_build_against_truth(case):
    """twelve alphas in one warm chain per element, with the default decouple_tol and with 0"""
    name, opts, n_omega, n_s = case
    f32 = 'float' in name
    label = '%s n_omega=%d n_s=%d' % (name, n_omega, n_s)
    j = C.job(n_omega, n_s)
    ctx = context(j)
    try:
        a = scan(ctx, j, **opts)
        b = scan(ctx, j, decouple_tol=0.0, **opts)
        d = scan(ctx, j, chains_per_wg=1, waves_per_chain=opts['waves_per_chain']) if f32 else None      # the binary64 build
    finally:
        ctx.close()
    tol = 1e-4 if f32 else 1e-6
    models = [C.model(n_omega, n_s, e) for e in range(2)]
    print('%s: iterations (normal, plus-minus) %s / %s with decouple_tol = 0, evaluations %s / %s; the model: %s, %s; n_act of the default run %d ... %d'
          % (label, a['n_iter'].sum(axis=1), b['n_iter'].sum(axis=1), a['n_evals'].sum(axis=1), b['n_evals'].sum(axis=1),
             [sum(s[0] for s in st) for _, st in models], [sum(s[1] for s in st) + 1 for _, st in models], a['n_act'].min(), a['n_act'].max()))
    for which, o in (('default decouple_tol', a), ('decouple_tol = 0', b)):
        assert o['kernel'] == name, (o['kernel'], name)
        for key in ('H', 'chi2', 'S', 'Q', 'v'):
            assert np.isfinite(o[key]).all(), (label, which, key)
        e_truth, audit = truth_error(n_omega, n_s, o), o['audit'].max()
        print('   %s: converged %d of %d, H against truth %.2e, audit %.2e' % (which, o['converged'].sum(), o['converged'].size, e_truth, audit))
        if not f32:
            assert o['converged'].all(), (label, which, np.argwhere(o['converged'] == 0))
        assert e_truth < tol, (label, which, e_truth)
        assert np.isfinite(o['audit']).all() and audit < tol, (label, which, audit)
    if f32:
        assert d['kernel'] == 'mxe::chain_kernel<%d, 2, double>' % opts['waves_per_chain'], d['kernel']
        for o in (a, b):
            np.testing.assert_allclose(o['chi2'], d['chi2'], rtol=2e-3)
    else:
        assert (b['n_act'] == n_s).all(), (label, b['n_act'])
        e_H, e_chi2 = rel_l2(a['H'], b['H']).max(), np.abs(a['chi2'] / b['chi2'] - 1).max()
        print('   the two runs: H %.2e, chi2 %.2e' % (e_H, e_chi2))
        assert e_H < 1e-7, (label, e_H)
        assert e_chi2 < 1e-6, (label, e_chi2)


TOL_D = 1e-7


@pytest.mark.parametrize('case', [C.find_case('mxe::chain_kernel<4, 2, double>', 200, 33),
                                  C.find_case('mxe::chain_kernel<1, 4, double>', 128, 97)], ids=C.case_id)
def test_reference_stopping_rule_on_a_large_block(case):
    """tol_h = 0, tol_d = 1e-7, miniter = 3, decouple_tol = 0: an alpha ends when max |W g| over the WHOLE block is below
    tol_d -- symv over 33 rows (four waves) and over 97 (one wave, two rows per lane), which no other GPU test runs.  Every
    alpha converges with at least three iterations, max |W g| recomputed in extended precision at every returned v is below
    tol_d, and H is within 1e-6 of the truth.

    What this does NOT prove: Newton converges quadratically, so the returned point usually lies far below tol_d (the ratio is
    printed), and a symv that under-reads a row would be seen only where it ends an alpha an iterate early -- with miniter = 3
    on a warm chain the iterate before is already converged.  It shows that the rule runs at these sizes, ends every alpha, and
    ends none at a point that violates it."""
    name, opts, n_omega, n_s = case
    j = C.job(n_omega, n_s)
    ctx = context(j)
    try:
        o = scan(ctx, j, tol_h=0.0, tol_d=TOL_D, miniter=3, decouple_tol=0.0, **opts)
    finally:
        ctx.close()
    assert o['kernel'] == name, (o['kernel'], name)
    assert o['converged'].all(), np.argwhere(o['converged'] == 0)
    assert (o['n_iter'] >= 3).all(), o['n_iter']
    assert (o['n_act'] == n_s).all(), o['n_act']
    V, c, D = j.V.astype(N.LD), j.c.astype(N.LD), j.D.astype(N.LD)
    worst = 0.0
    for e, kind in enumerate(C.ENTROPIES):
        ghat = j.ghat[e].astype(N.LD)
        for ia, alpha in enumerate(j.alphas):
            v = o['v'][e, ia].astype(N.LD)
            u = V.dot(v)
            H, w = (D * np.exp(u),) * 2 if kind == 'normal' else (D * (np.exp(u) - np.exp(-u)), D * (np.exp(u) + np.exp(-u)))
            g = c * (c * V.T.dot(H) - ghat) + N.LD(alpha) * v
            worst = max(worst, float(np.abs((V.T * w).dot(V).dot(g)).max()))
    e_truth = truth_error(n_omega, n_s, o)
    print('%s n_omega=%d n_s=%d: iterations %s, max |W g| %.2e (tol_d %.0e), H against truth %.2e'
          % (name, n_omega, n_s, o['n_iter'].sum(axis=1), worst, TOL_D, e_truth))
    assert worst < TOL_D * (1 + 1e-6), worst
    assert e_truth < 1e-6, e_truth
