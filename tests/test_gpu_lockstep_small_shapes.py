"""The lock-step kernel at the smallest shapes at which its fused loop and its elimination can go wrong, against the one-chain
binary64 kernel: the 3 x 3 mixed normal / plus-minus job of
tests/test_gpu_chain_kernel.py::test_four_chain_kernel_equals_single_chain_kernel with that test's mesh and bounds."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxent_amd as mx                                      # noqa: E402
from maxent_amd import device, synthetic, hostprep           # noqa: E402

pytestmark = pytest.mark.gpu

# The elimination (gj2_solve64_f32) has one instantiation per class of the active block, n_act <= 16, 20, 24, 28, 32, in the build
# for at most 32 singular directions.  n_act = #{k: c_k^2 w_max > theta alpha} with c = S / sigma, theta = 1e-5; evaluated on the
# CPU with the oracle (ref_numpy.alpha_loop, w_max of its H) on the mesh of that test, 1e-2 ... 1e4, this job (51 directions, of
# which the device stages the leading ones) gives n_act = 18 ... 29 for every element -- the classes 20, 24, 28, 32 --, and cut to
# its first 16 directions the class 16.
CLASSES = (16, 20, 24, 28, 32)


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


@functools.lru_cache(maxsize=None)
def job(n_omega):
    tau, omega, K, Gmat, _ = synthetic.matrix_G(3, 120, n_omega)
    K.reduce_singular_space(1e-14)
    return omega, K, Gmat


def solve_three_ways(n_omega, keep):
    omega, K, Gmat = job(n_omega)
    D = synthetic.flat_D(omega)
    err = synthetic.SIGMA * np.ones(120)
    alphas = np.array(synthetic.alpha_mesh(40)) * 120
    elems = [(i, j) for i in range(3) for j in range(3)]
    kinds = [device.ENTROPY_NORMAL if i == j else device.ENTROPY_PLUSMINUS for i, j in elems]
    v0 = np.stack([hostprep.initial_v(K.V, D, omega.delta, k) for k in kinds])
    ctx = device.DeviceContext(K.U, K.S, K.V, keep=keep)
    ds = ctx.add_dataset(err)
    ctx.set_elements([ds] * 9, [Gmat[i, j] for i, j in elems], np.tile(D, (9, 1)), kinds)
    a = ctx.solve_chains(np.arange(9), alphas, v0, device.default_opts(chains_per_wg=1, alpha_split=1))
    outs = []
    for split in (1, 4):
        o = ctx.solve_chains(np.arange(9), alphas, v0, device.default_opts(chains_per_wg=4, alpha_split=split))
        outs.append((o, ctx.fetch_n_act().copy(), ctx.last_launch_info()['kernel']))
    ctx.close()
    return a, outs


def check(a, outs):
    assert a['converged'].all()
    for o, n_act, kernel in outs:
        assert o['converged'].all()
        eH = rel_l2(o['H'], a['H']).max()
        d = o['n_iter'].astype(int) - a['n_iter'].astype(int)
        print(kernel, 'H', eH, 'chi2', np.abs(o['chi2'] / a['chi2'] - 1).max(), 'Q', np.abs(o['Q'] / a['Q'] - 1).max(),
              'iterations', d.min(), d.max(), d.mean(), 'n_act', n_act.min(), n_act.max())
        assert eH < 1e-8
        np.testing.assert_allclose(o['chi2'], a['chi2'], rtol=1e-7)
        np.testing.assert_allclose(o['Q'], a['Q'], rtol=1e-10)
    # same Newton iteration in both kernels up to the precision of the Gram matrix and the order of the sums: iteration counts
    # differ by one at most -- for the scans in one piece, as in that test (alpha_split = 4 starts three pieces of every scan cold,
    # where the one-chain scan comes warm from the alpha before: up to 9 iterations more at those alphas, none elsewhere)
    o, _, _ = outs[0]
    d = o['n_iter'].astype(int) - a['n_iter'].astype(int)
    assert d.min() >= -1 and d.max() <= 1 and abs(d.mean()) < 0.1


@pytest.mark.parametrize('n_omega', [128, 129, 300])
def test_lockstep_kernel_equals_one_chain_kernel_in_every_class_of_the_elimination(n_omega):
    """n_omega = 128: exactly one trip of the fused loop per wave; 129: padded to 256, the look-ahead reads past the end; 300.
    n_act of the results shows that every class of the elimination ran."""
    seen = set()
    for keep in (None, 16):
        a, outs = solve_three_ways(n_omega, keep)
        for o, n_act, kernel in outs:
            assert 'chain_kernel_mc<32' in kernel, kernel
            seen |= {min(c for c in CLASSES if n <= c) for n in n_act.ravel() if n > 0}
        check(a, outs)
    assert seen == set(CLASSES), sorted(seen)


def test_three_alphas_a_decade_apart_end_as_in_the_one_chain_kernel():
    """n_tau = 100, n_omega = 200, three alphas a decade apart: the warm starts overshoot and trial points whose weights grow by
    many powers of two (Gram operands at the end of the binary16 range) are rejected; what converges is finite and the one-chain
    kernel's answer, with the same flags."""
    n_tau, n_omega = 100, 200
    tau, omega, K, G = synthetic.single_G(n_tau, n_omega)
    K.reduce_singular_space(1e-14)
    D = synthetic.flat_D(omega)
    err = synthetic.SIGMA * np.ones(n_tau)
    alphas = np.array(mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e1, n_points=3)) * n_tau
    kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
    v0 = np.stack([hostprep.initial_v(K.V, D, omega.delta, k) for k in kinds])
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(err)
    ctx.set_elements([ds, ds], [G, G], np.stack([D, D]), kinds)
    a = ctx.solve_chains([0, 1], alphas, v0, device.default_opts(chains_per_wg=1, alpha_split=1))
    outs = [ctx.solve_chains([0, 1], alphas, v0, device.default_opts(chains_per_wg=4, alpha_split=s)) for s in (1, 3)]
    outs.append(ctx.solve_chains([0, 1], alphas, v0))
    ctx.close()
    for o in outs:
        assert (o['converged'] == a['converged']).all()
        ok = o['converged'].astype(bool)
        assert ok.any()
        for key in ('H', 'chi2', 'Q'):
            assert np.isfinite(o[key][ok]).all()
        e = rel_l2(o['H'][ok], a['H'][ok]).max()
        print('H against the one-chain kernel', e, 'evaluations', o['n_evals'].max())
        assert e < 1e-7
