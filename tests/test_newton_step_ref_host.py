"""The conditions on the INPUTS of tests/test_gpu_one_chain_builds.py::test_one_newton_step_of_every_build (CPU only): that test
lets every build of the one-chain kernel take ONE iteration from a start vector of the host's and compares the step with the
extended-precision one (tests/newton_step_ref.py).  It says what it is meant to say only where, for every shape and both
entropies, at the alpha indices 6 and 11 of the mesh and from the model's v of the alpha before
(oracle/sform.alpha_chain, binary64 -- never the device):

1. delta^T W delta <= 0.5 step_max sum(D) (x 2: plus-minus): the kernel neither shortens nor damps the step -- it IS the
   undamped Newton step (measured: at most 0.23 of step_max sum(D));
2. the binary64 step of numpy is within 1e-12 |delta| of the extended-precision one (measured: <= 1.2e-14): the reference is
   five decades better than the gate on a binary64 build (1e-9);
3. at alpha index 11 the step with the LAST direction decoupled differs from the true one by >= 1e-6 |delta| -- a thousand
   times that gate (measured: 1.2e-6 at n_omega = 6300, 1.1e-5 at 3000, >= 7.7e-5 at n_omega <= 300): the smallest
   structural fault of a solve, one row left out, cannot pass;
4. binary32 builds: their gate, ten times the error of the 'f32 stream' step (the arithmetic of Stream<float> on the host), is
   at most a tenth of that same change (measured, n_omega <= 300: stream error <= 4.4e-6, gate / change <= 0.06).

Condition 4 does NOT hold with the last direction at (n_omega, n_s) = (6300, 64), the one shape of
chain_kernel<4, 2, float, device-memory state>: the stream error there is 2.1e-6 / 9.7e-7 (normal / plus-minus) and the change
6.6e-6 / 1.2e-6.  Every entry of W falls as 1 / n_omega (D = 1 / n_omega, the columns of V have unit length), so the coupling
c_k^2 W_kk / alpha of the weak directions does too, and that build needs n_omega > 6144 (its omega-space state has to miss
the LDS: mxe_shapes.h lds_bytes); at 6145 the figures are 3.5e-6 and 3.0e-6.  No n_omega reaches the build and meets the
condition.  The case stays, with the gate of every binary32 case, and what that gate does resolve there is asserted in its
place: a decoupled direction k for EVERY k < 32 (measured: gate / change <= 0.1 for k <= 33).  The solve of that build at 64 rows
is the unfused chol_solve, whose last row the (128, 64) case of chain_kernel<4, 2, float> covers under condition 4 itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newton_step_ref as N                                  # noqa: E402
import one_chain_cases as C                                  # noqa: E402

LAST = C.N_ALPHA - 1
F32_LONG_MESH = (6300, 64)          # condition 4 with the last direction cannot be met by this build (above)
F32_LONG_MESH_DIRECTIONS = 32


def test_the_reference_step_solves_its_system():
    """newton_step against its definition, written out once more: a random symmetric problem small enough to check by hand
    (residual of the system in extended precision), the dropped direction takes the diagonal step, the three precisions agree
    to their roundings"""
    rng = np.random.RandomState(3)
    n_omega, n_s = 40, 7
    V = np.linalg.qr(rng.randn(n_omega, n_s))[0]
    c, ghat, D, v = 10.0 ** rng.uniform(0, 2, n_s), rng.randn(n_s), np.full(n_omega, 1.0 / n_omega), 0.3 * rng.randn(n_s)
    alpha = 5.0
    for kind in C.ENTROPIES:
        delta, q = N.newton_step(V, c, ghat, D, kind, alpha, v, N.LD)
        assert delta.dtype == N.LD
        u = V.astype(N.LD).dot(v.astype(N.LD))
        H = D * np.exp(u) if kind == 'normal' else D * (np.exp(u) - np.exp(-u))
        w = H if kind == 'normal' else D * (np.exp(u) + np.exp(-u))
        W = (V.T.astype(N.LD) * w).dot(V.astype(N.LD))
        cl = c.astype(N.LD)
        g = cl * (cl * V.T.astype(N.LD).dot(H) - ghat) + alpha * v         # gradient; the step solves (c^2 W + alpha) delta = g
        res = cl * cl * W.dot(delta) + alpha * delta - g
        assert np.linalg.norm(res) < 1e-16 * np.linalg.norm(g)
        assert abs(q - float(delta.dot(W.dot(delta)))) <= 1e-15 * q
        d64, _ = N.newton_step(V, c, ghat, D, kind, alpha, v, np.float64)
        d32, _ = N.newton_step(V, c, ghat, D, kind, alpha, v, 'f32 stream')
        assert d64.dtype == np.float64 and d32.dtype == np.float64
        assert N.rel_err(d64, delta) < 1e-13 and 1e-9 < N.rel_err(d32, delta) < 1e-5
        k = 4
        dk, _ = N.newton_step(V, c, ghat, D, kind, alpha, v, N.LD, drop=k)
        assert abs(dk[k] - g[k] / alpha) < 1e-17 * abs(g[k] / alpha)        # delta_k = c_k (rho_k + alpha v_k / c_k) / alpha
        assert N.rel_err(dk, delta) > 1e-4


@pytest.mark.parametrize('n_omega,n_s', C.SHAPES)
def test_conditions_on_the_inputs_of_the_one_step_test(n_omega, n_s):
    j = C.job(n_omega, n_s)
    f32 = (n_omega, n_s) in C.F32_STEP_SHAPES
    for e, kind in enumerate(C.ENTROPIES):
        m, stats = C.model(n_omega, n_s, e)
        assert m['converged'].all(), ('the model does not converge', kind, m['converged'])
        for ia in C.STEP_ROWS:
            r = C.step_ref(n_omega, n_s, e, ia)
            bound = r['q'] / (C.STEP_MAX * j.sum_D(e))
            e64 = C.step_err(n_omega, n_s, e, ia, np.float64)
            line = 'n_omega=%d n_s=%d %s alpha[%d]: delta^T W delta / (step_max sum D) %.3f; binary64 step %.1e' % (
                n_omega, n_s, kind, ia, bound, e64)
            assert 0.0 < bound <= 0.5, line                                                  # 1.
            assert e64 < 1e-12, line                                                         # 2.
            if f32:
                line += '; f32 stream %.2e' % C.step_err(n_omega, n_s, e, ia, 'f32 stream')
            if ia == LAST:
                change = C.step_err(n_omega, n_s, e, ia, np.float64, n_s - 1)
                line += '; last direction dropped %.2e' % change
                assert change >= 1e-6, line                                                  # 3.
                if f32:
                    gate = C.f32_step_gate(n_omega, n_s, e, ia)
                    if (n_omega, n_s) != F32_LONG_MESH:
                        assert gate <= 0.1 * change, line                                    # 4.
                    else:
                        worst = min(C.step_err(n_omega, n_s, e, ia, np.float64, k) for k in range(F32_LONG_MESH_DIRECTIONS))
                        line += '; smallest change of a dropped direction k < %d: %.2e' % (F32_LONG_MESH_DIRECTIONS, worst)
                        assert gate <= 0.1 * worst, line                                     # 4., as far as it can hold there
            print(line)


def test_every_reachable_build_has_a_case():
    """the ten one-chain builds a launch can reach (tests/test_kernel_build_host.py: <2, 4> and <4, 4> are not)"""
    assert len(C.BUILDS) == 10 and len(C.CASES) == 59 and len(C.SCAN_CASES) == 56
    assert C.F32_STEP_SHAPES == sorted([(128, 16), (200, 33), (300, 63), (128, 64), (6300, 64)])
