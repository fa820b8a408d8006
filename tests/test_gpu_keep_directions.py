"""The problems of tests/keep_cases.py through the product path on the device: where ``batch_solver.directions_to_keep`` lets
the device solve with 64 or 128 singular directions, the H that comes back is held against the extended-precision fixed point
of ALL directions; where the bound -- with eta = chi2_factor in it -- forbids the truncation, every direction is staged, or the
job is refused where there are more than the device takes.  tests/test_keep_bound_host.py checks on the CPU where each case
sits; nothing here is tuned to what the device returns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor                                                # noqa: E402
import keep_cases as kc                                      # noqa: E402
import maxent_amd as mx                                     # noqa: E402
from maxent_amd import batch_solver, device                  # noqa: E402

pytestmark = pytest.mark.gpu

GATE = 1e-6                 # the product's parity gate: relative L2 of H against the extended-precision fixed point
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


@pytest.fixture
def decisions(monkeypatch):
    """what ``directions_to_keep`` was asked and what it answered, call by call"""
    seen = []
    real = batch_solver.directions_to_keep

    def spy(K, specs=None, arrays=None, *args, **kwargs):
        got = real(K, specs, arrays, *args, **kwargs)
        seen.append(dict(args=args, kwargs=kwargs, arrays=arrays is not None, n_s=len(K.S), rotated=K.rotation is not None, got=got))
        return got
    monkeypatch.setattr(batch_solver, 'directions_to_keep', spy)
    return seen


def kernel_of(c):
    """a DataKernel of the case's matrix of its own (what is staged for it is nobody else's)"""
    p = kc.problem(c)
    return mx.DataKernel(np.arange(float(len(p['G']))), p['omega'], np.array(p['Kmat']))


def loop_of(c):
    """MaxEntLoop + DataKernel, the case's ladder of alphas, its entropy and its eta"""
    p = kc.problem(c)
    loop = mx.MaxEntLoop(cost_function=c.entropy, alpha_mesh=mx.DataAlphaMesh(kc.ladder(c) / len(p['G'])))
    loop.cost_function.chi2_factor = c.eta
    loop.set_verbosity(mx.VerbosityFlags.Quiet)
    loop.K = kernel_of(c)
    loop.D = mx.FlatDefaultModel(p['omega'])
    loop.G = p['G']
    loop.err = p['err']
    return loop


def check_against_all_directions(c, H, what):
    """H (n_alpha, n_omega) at the first and the last alpha against the fixed point of ALL directions"""
    worst = 0.0
    for ia in (0, -1):
        e = anchor.rel_l2_checked(H[ia], kc.truth(c, ia)[1])
        print('%s %s alpha[%d]: rel L2 to the all-direction truth %.3e' % (kc.case_id(c), what, ia, e))
        assert e < GATE, (kc.case_id(c), what, ia, e)
        worst = max(worst, e)
    return worst


def check_launch(info, c):
    print('%s: kernel %s, keep %s, audit %.3e over %d problems' % (kc.case_id(c), info['kernel'], info['keep'], info['audit_max'],
                                                                  info['audit_problems']))
    assert info['audit_problems'] >= kc.N_LADDER and info['audit_max'] < GATE


@pytest.mark.parametrize('entropy', kc.ENTROPIES)
def test_sixty_four_directions_at_the_edge_of_the_bound(entropy, decisions):
    """eta = 1, the dropped 32 directions within a factor 2 below the edge: the lock-step kernel runs on 64 directions, says so
    in ``last_launch``, returns zeros in the others, and H passes the gate against the truth of all 96"""
    c = kc.find(64, entropy, 1.0, 'below')
    loop = loop_of(c)
    res = loop.run()
    info = loop.last_launch
    assert [d['got'] for d in decisions] == [64] and decisions[0]['kwargs'] == dict(chi2_factor=1.0) and not decisions[0]['arrays']
    assert np.all(res.converged)
    check_launch(info, c)
    assert info['kernel'].startswith('mxe::chain_kernel_mc<'), info['kernel']
    assert info['keep'] == 64
    v, H = np.asarray(res.v), np.asarray(res.H)
    assert v.shape == (kc.N_LADDER, 96) and np.all(v[..., 64:] == 0.0) and np.any(v[..., :64] != 0.0)
    check_against_all_directions(c, H, 'MaxEntLoop')
    for ia in (0, -1):
        r = kc.dropped_residual(c, H[ia], keep=64, ia=ia)
        print('%s alpha[%d]: first-order residual of the dropped directions %.3e' % (kc.case_id(c), ia, r))
        assert r <= kc.KEEP_BOUND


@pytest.mark.parametrize('eta,alpha', [(100.0, 1.0), (1e4, 100.0)])
@pytest.mark.parametrize('entropy', kc.ENTROPIES)
def test_eta_takes_the_truncation_back(entropy, eta, alpha, decisions):
    """the problem of the test above at eta = 100 and 1e4: the bound is a hundred times over the edge, all 96 directions are
    staged for the one-chain kernel and H passes the same gate (with 64 directions -- what a bound without eta returned for
    both -- u is 3e-6 away: test_keep_bound_host.py).

    eta = 1e4 runs at alpha = 100, moved along the invariant of tests/keep_cases.py: with the ladder ending at alpha = 1
    (alpha / eta = 1e-4, the bound 1e4 times over the edge) the one-chain kernel did not converge below alpha / eta = 3e-3 on
    these 96 directions (MI355X: the last four of the eight alphas), which is a matter of its own and not of the decision;
    tests/test_keep_bound_host.py keeps that case, on the CPU."""
    c = kc.find(64, entropy, eta, 'far', alpha=alpha)
    assert c.plateau == kc.find(64, entropy, 1.0, 'below').plateau and kc.own_bound(c) > 50 * kc.KEEP_BOUND
    loop = loop_of(c)
    res = loop.run()
    info = loop.last_launch
    assert [d['got'] for d in decisions] == [None] and decisions[0]['kwargs'] == dict(chi2_factor=eta)
    assert np.all(res.converged)
    check_launch(info, c)
    assert info['kernel'].startswith('mxe::chain_kernel<'), info['kernel']
    assert info['keep'] is None
    v = np.asarray(res.v)
    assert v.shape == (kc.N_LADDER, 96) and np.any(v[..., 64:] != 0.0)
    check_against_all_directions(c, np.asarray(res.H), 'MaxEntLoop')


def test_elementwise_arrays_form(decisions):
    """a 2 x 2 matrix job through ElementwiseMaxEnt: the job reaches ``directions_to_keep`` as arrays, diagonal (normal) and
    off-diagonal (plus-minus) elements share one launch of the lock-step kernel on 64 directions"""
    cn, cp = kc.find(64, 'normal', 1.0, 'below'), kc.find(64, 'plusminus', 1.0, 'below')
    pn, pp = kc.problem(cn), kc.problem(cp)
    assert np.array_equal(pn['Kmat'], pp['Kmat'])           # (one kernel, the data of the two entropies)
    n_data = len(pn['G'])
    grid = np.arange(float(n_data))
    Gmat = np.empty((2, 2, n_data))
    Gmat[0, 0] = Gmat[1, 1] = pn['G']
    Gmat[0, 1] = Gmat[1, 0] = pp['G']
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = pn['omega']
    ew.K = kernel_of(cn)
    ew.set_G_tau_data(grid, Gmat)
    ew.alpha_mesh = mx.DataAlphaMesh(kc.ladder(cn) / n_data)
    ew.set_error(kc.SIGMA)
    res = ew.run()
    assert type(ew.maxent_diagonal.K) is mx.DataKernel and len(ew.maxent_diagonal.K.S) == 96
    assert decisions and all(d['got'] == 64 and d['kwargs'] == dict(chi2_factor=1.0) for d in decisions)
    assert any(d['arrays'] for d in decisions)
    assert np.all(res.converged)
    for info in ew.last_launches:
        check_launch(info, cn)
        assert info['kernel'].startswith('mxe::chain_kernel_mc<'), info['kernel']
        assert info['keep'] == 64
    v, H = np.array(res.v), np.array(res.H)
    assert v.shape == (2, 2, kc.N_LADDER, 96) and np.all(v[..., 64:] == 0.0) and np.any(v[..., :64] != 0.0)
    for (i, j), c in (((0, 0), cn), ((1, 1), cn), ((0, 1), cp), ((1, 0), cp)):
        check_against_all_directions(c, H[i, j], 'ElementwiseMaxEnt (%d, %d)' % (i, j))
        assert kc.dropped_residual(c, H[i, j, -1], keep=64) <= kc.KEEP_BOUND


@pytest.mark.parametrize('entropy', kc.ENTROPIES)
def test_a_hundred_and_twenty_eight_directions_or_a_refusal(entropy, decisions, monkeypatch):
    """160 singular values, 64 too few, the 32 behind the 128th just below the edge: 128 are staged and H passes the gate against
    the truth of all 160.  All directions -- asked for by MAXENT_AMD_ALL_DIRECTIONS, or forced by eta = 1e4 -- are more than the
    device takes: the documented refusal, not another answer."""
    c = kc.find(128, entropy, 1.0, 'below')
    loop = loop_of(c)
    res = loop.run()
    info = loop.last_launch
    assert [d['got'] for d in decisions] == [128]
    assert np.all(res.converged)
    check_launch(info, c)
    assert info['keep'] == 128
    v, H = np.asarray(res.v), np.asarray(res.H)
    assert v.shape == (kc.N_LADDER, 160) and np.all(v[..., 128:] == 0.0) and np.any(v[..., 64:128] != 0.0)
    check_against_all_directions(c, H, 'MaxEntLoop')
    for ia in (0, -1):
        assert kc.dropped_residual(c, H[ia], keep=128, ia=ia) <= kc.KEEP_BOUND
    far = kc.find(128, entropy, 1e4, 'far', alpha=1.0)
    assert far.plateau == c.plateau
    loop.cost_function.chi2_factor = far.eta
    with pytest.raises(device.MaxEntDeviceError, match='160 singular values above its threshold and the device solves with at most 128'):
        loop.run()
    assert decisions[-1]['got'] is None and decisions[-1]['kwargs'] == dict(chi2_factor=1e4)
    loop.cost_function.chi2_factor = 1.0
    monkeypatch.setenv('MAXENT_AMD_ALL_DIRECTIONS', '1')
    with pytest.raises(device.MaxEntDeviceError, match='160 singular values above its threshold and the device solves with at most 128'):
        loop.run()
    assert decisions[-1]['got'] is None and len(decisions) == 3


def test_model_scan_hands_eta_on(decisions):
    """the problem of tests/test_gpu_model_scan.py (40 imaginary times, 60 frequencies, 12 alphas) under two default models"""
    from model_scan_ref import scan_problem
    tau, omega, A, G, Ds = scan_problem()
    tm = mx.TauMaxEnt(cost_function=mx.MaxEntCostFunction(chi2_factor=2.5))
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-8, omega_max=8, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e3, n_points=12)
    tm.set_G_tau_data(tau, G)
    tm.set_error(1e-3)
    delta = np.asarray(tm.omega.delta)
    out = tm.default_model_scan([mx.DataDefaultModel(D / delta, tm.omega) for D in (Ds[0], Ds[3])], alpha='classic')
    assert out['info']['launches'] == 1
    assert decisions and all(d['kwargs'] == dict(chi2_factor=2.5) and not d['args'] for d in decisions)


def test_resampling_hands_eta_on(decisions):
    """the G(tau) bins of tests/golden/bins.npz (tests/test_gpu_resample.py: 60 frequencies, 8 alphas), 8 jackknife blocks"""
    g = np.load(os.path.join(GOLD, 'bins.npz'))
    tm = mx.TauMaxEnt(cov_threshold=float(g['cov_threshold']), cost_function=mx.MaxEntCostFunction(chi2_factor=2.5))
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=60)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=0.05, alpha_max=500, n_points=8)
    bins = g['s_bins']
    tm.set_G_tau_bins(g['s_tau'], bins)
    out = tm.resample_errors(bins, method='jackknife', block=len(bins) // 8)
    assert out['info']['launches'] == 1 and out['n_resamples'] == 8
    assert decisions and all(d['kwargs'] == dict(chi2_factor=2.5) and not d['args'] for d in decisions)
