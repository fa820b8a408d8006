"""The three consumers of factor_B (mxe_factor.hip.h) -- mxe_logdet, mxe_posterior_var, mxe_posterior_sample -- on ONE
context and ONE set of H rows (those of a launch, read on the device), against numpy.

Shapes (n_omega, n_s): n_omega = 37 is no multiple of 4 or 16; n_s = 5, 16, 17 are a short tile, a full tile and a tile
plus one row; (69, 64) fills the 64-row build (n_s <= n_omega for an orthonormal V': 69 is the mesh there, again no
multiple of 4); (100, 70) runs the 128-row build.  Two elements (normal, plus-minus) at two alphas: four problems.
17 functionals (a second block of 16 with one row in it) and the first of them alone; 17 samples and the first alone.

Gates, each the one its quantity already has: logdet against slogdet as test_logdet_kernel_matches_numpy_slogdet
(1e-8 relative); Gamma_ii and f^T Gamma f against the dense longdouble Gamma by the gate of test_gpu_posterior_errors.py;
the samples with handed-in normals by the gate of test_gpu_posterior_samples.py.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_posterior_samples_host import truth_samples                  # noqa: E402
from test_gpu_posterior_errors import gate as var_gate                 # noqa: E402
from test_gpu_posterior_samples import gate as sample_gate             # noqa: E402
from maxent_amd import device, hostprep, posterior                     # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(37, 5), (37, 16), (37, 17), (69, 64), (100, 70)]
ALPHAS = np.array([3.0e3, 30.0])
N_SAMPLES = 17
SIGMA = 1e-3
BAD = 1                                  # the problem whose H row gets a NaN


class Run(object):
    """the problem of one shape and what the device gave for it, before and after a NaN went into row BAD of H"""

    def __init__(self, n_omega, ns):
        n_tau, beta, half_width = ns + 8, 10.0, 5.0
        tau = np.linspace(0.0, beta, n_tau)
        w = np.linspace(-half_width, half_width, n_omega)
        K = np.exp(-np.outer(tau, w) - np.logaddexp(0.0, -beta * w)[None, :])
        U, _, Vt = np.linalg.svd(K, full_matrices=False)
        # the singular vectors of a fermionic kernel with singular values that keep every direction in play
        self.U, self.S, self.V = U[:, :ns].copy(), np.logspace(0.0, -6.0, ns), Vt[:ns].T.copy()
        self.K = np.dot(self.U * self.S, self.V.T)
        dw = w[1] - w[0]
        H = (0.6 * np.exp(-(w - 1.0) ** 2 / 0.5) + 0.4 * np.exp(-(w + 1.5) ** 2 / 0.8) + 1e-4) * dw
        self.D = np.full(n_omega, dw / (2 * half_width))
        self.kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
        edges = np.linspace(-4.8, 4.8, 13)
        windows = [(-3.0, 0.0), (0.0, 2.0), (2.0, 4.5)] + list(zip(edges[:-1], edges[1:]))
        self.F = np.concatenate([np.ones((1, n_omega)), posterior.window_rows(w, windows), w[None, :]])       # n_f = 17
        self.el = np.repeat(np.arange(2), len(ALPHAS))
        self.al = np.tile(ALPHAS, 2)
        P = len(self.el)
        self.z = np.stack([posterior.sample_normals(9, s, N_SAMPLES, n_omega + ns) for s in range(P)])
        ctx = device.DeviceContext(self.U, self.S, self.V)
        try:
            ds = ctx.add_dataset(SIGMA * np.ones(n_tau))
            ctx.set_elements([ds, ds], [np.dot(self.K, H), np.dot(self.K, H * np.sin(1.3 * w))], np.tile(self.D, (2, 1)), self.kinds)
            v0 = np.stack([hostprep.initial_v(self.V, self.D, dw, k) for k in self.kinds])
            out = ctx.solve_chains(np.arange(2), ALPHAS, v0)
            self.H = out['H'].reshape(P, n_omega)
            assert np.all(np.isfinite(self.H))
            rows = np.arange(P)
            self.before = self.consumers(ctx, rows)
            hip = ctypes.CDLL('libamdhip64.so')
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            nan = np.array([np.nan])
            assert hip.hipMemcpy(ctx.result_device_ptrs()['H'] + (BAD * n_omega + 7) * 8, nan.ctypes.data_as(ctypes.c_void_p), 8, 1) == 0
            self.after = self.consumers(ctx, rows)
            self.without = self.consumers(ctx, rows[rows != BAD])
        finally:
            ctx.close()

    def consumers(self, ctx, rows):
        """what the three give for the problems ``rows`` of the launch (logdet: for all of them)"""
        el, al, z = self.el[rows], self.al[rows], self.z[rows]
        got = dict(logdet=ctx.logdet().ravel())
        got.update(ctx.posterior_var(el, al, problem_index=rows, F=self.F, want_diag=True))
        one = ctx.posterior_var(el, al, problem_index=rows, F=self.F[:1], want_diag=True)
        got.update(var1=one['var'], prior1=one['prior'], diag1=one['diag'])
        got['samples'] = ctx.posterior_sample(el, al, problem_index=rows, n_samples=N_SAMPLES, z=z)
        got['samples1'] = ctx.posterior_sample(el, al, problem_index=rows, n_samples=1, z=z[:, :1])
        return got


@functools.lru_cache(maxsize=None)
def run_of(shape):
    return Run(*shape)


@pytest.mark.parametrize('shape', SHAPES)
def test_three_consumers_of_one_factor_against_numpy(shape):
    r = run_of(shape)
    got = r.before
    c = r.S / SIGMA
    for p in range(len(r.el)):
        H, a, kind = r.H[p], r.al[p], r.kinds[r.el[p]]
        w = posterior.entropy_weights(H, r.D, kind)
        label = 'n_omega=%d n_s=%d problem %d' % (shape + (p,))
        sign, ref = np.linalg.slogdet(np.eye(len(c)) + (c * c)[:, None] * np.dot(r.V.T * w[None, :], r.V) / a)
        print('%s: logdet %.15g, slogdet %.15g' % (label, got['logdet'][p], ref))
        assert sign > 0 and abs(got['logdet'][p] - ref) < 1e-8 * max(1.0, abs(ref)), (label, got['logdet'][p], ref)
        d_t, gamma = truth_samples(r.K, SIGMA, w, a, r.V, c, r.z[p])
        F = np.asarray(r.F, dtype=np.longdouble)
        var_gate(label + ' diag', got['diag'][p], np.diag(gamma), w / a)
        var_t, prior_t = np.einsum('fi,ij,fj->f', F, gamma, F), np.dot(F ** 2, w) / a
        var_gate(label + ' var', got['var'][p], var_t, prior_t)
        np.testing.assert_allclose(got['prior'][p], np.dot(r.F ** 2, w) / a, rtol=1e-12)
        sample_gate(label, r, got['samples'][p], d_t, gamma, a, w)
        var_gate(label + ' diag, n_f = 1', got['diag1'][p], np.diag(gamma), w / a)
        var_gate(label + ' var, n_f = 1', got['var1'][p], var_t[:1], prior_t[:1])
        np.testing.assert_allclose(got['prior1'][p], np.dot(r.F[:1] ** 2, w) / a, rtol=1e-12)
        sample_gate(label + ' n_samples = 1', r, got['samples1'][p], d_t[:1], gamma, a, w)


@pytest.mark.parametrize('shape', SHAPES)
def test_nan_row_gives_nan_from_all_three_and_leaves_the_others_alone(shape):
    r = run_of(shape)
    keep = [p for p in range(len(r.el)) if p != BAD]
    for name in sorted(r.before):
        before, after, without = r.before[name], r.after[name], r.without[name]
        assert np.all(np.isfinite(before)), name
        assert np.all(np.isnan(after[BAD])), name
        assert np.array_equal(before[keep].view(np.uint64), after[keep].view(np.uint64)), name
        if name != 'logdet':                         # (mxe_logdet takes the whole launch)
            assert without.shape == after[keep].shape, name
            assert np.array_equal(without.view(np.uint64), after[keep].view(np.uint64)), name
