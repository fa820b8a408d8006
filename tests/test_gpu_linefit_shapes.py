"""The device line fit (mxe_select_launch / mxe_select3_launch) on the shapes at which its code takes another path, against
the host analyzers: maxent_amd.analyzers.fit_piecewise / curv and the entropy rule, as in
tests/test_gpu_multi.py::test_device_analyzers_pick_the_alphas_the_host_analyzers_pick_on_the_reference_curves."""
import ctypes

import numpy as np
import pytest

from maxent_amd import device, hostprep, synthetic
from maxent_amd.analyzers import curv, fit_piecewise

pytestmark = pytest.mark.gpu

N_TAU, N_OMEGA = 30, 37          # (the row length is no multiple of the 256 threads that copy it)


def curves(alpha, seed):
    """chi2 and S of the scans, side by side: [n_scan][n_alpha].

    0  a clean kink of log chi2 over log alpha
    1, 2, 3  the same with NaN at the first, the last, the middle alpha
    4  two break points that tie: with chi2[m] NaN the break points m and m + 1 split the points that count in the same way,
       so the host's exact misfits are equal to the last bit and np.nanargmin takes the lower one
    5  every break point ties at a misfit of exactly 0 (chi2 = 1: log chi2 = 0 in any arithmetic): both lines are y = 0, there
       is no intersection and no pick
    6  every value NaN
    """
    n = len(alpha)
    rng = np.random.RandomState(seed)
    x = np.log(alpha)
    xk = x[(2 * n) // 5] if n > 2 else x[0]
    y = 1.0 + 1.3 * np.maximum(x - xk, 0.0) + 0.02 * (x - x.min()) + 0.01 * rng.rand(n)
    C = np.tile(np.exp(y), (7, 1))
    S = np.tile(-0.3 * (x - x[n // 3]) ** 2 + 0.01 * rng.rand(n), (7, 1))
    C[1, 0] = np.nan
    C[2, n - 1] = np.nan
    C[3, n // 2] = np.nan
    C[4, (2 * n) // 5] = np.nan
    C[5] = 1.0
    C[6] = np.nan
    S[1, 0] = np.nan
    S[3, n // 2] = np.nan
    S[6] = np.nan
    return C, S


def host_picks(alpha, C, S, deg, gamma):
    n = len(alpha)
    want = np.full((3, len(C)), -1, dtype=int)
    for c in range(len(C)):
        with np.errstate(all='ignore'):
            try:
                want[0, c] = fit_piecewise(np.log(alpha), np.log(C[c]), deg)[0] if n > 4 else -1
            except ValueError:
                pass
            cv = curv(gamma * np.log10(alpha), np.log10(C[c]))[0]
            d = np.full(n, np.nan)
            d[1:-1] = (S[c, 2:] - S[c, :-2]) / (np.log(alpha[2:]) - np.log(alpha[:-2]))
        want[1, c] = -1 if np.all(np.isnan(cv)) else int(np.nanargmax(cv))
        want[2, c] = -1 if np.all(np.isnan(d)) else int(np.nanargmin(d ** 2))
    return want


@pytest.fixture(scope='module')
def staged():
    tau, omega, K, G = synthetic.single_G(N_TAU, N_OMEGA)
    K.reduce_singular_space(1e-14)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(N_TAU))
    D = synthetic.flat_D(omega)
    ctx.set_elements([ds] * 7, [G] * 7, np.tile(D, (7, 1)), [device.ENTROPY_NORMAL] * 7)
    v0 = hostprep.initial_v(K.V, D, omega.delta, device.ENTROPY_NORMAL)
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    yield ctx, np.tile(v0, (7, 1)), hip
    ctx.close()


def check_mesh(ctx, v0, hip, alpha, seed):
    n = len(alpha)
    ctx.upload_chains(np.arange(7), alpha, v0)
    ctx.launch()
    ctx.sync()
    C, S = curves(alpha, seed)
    ptrs = ctx.result_device_ptrs()
    assert hip.hipMemcpy(ptrs['chi2'], C.ctypes.data_as(ctypes.c_void_p), C.nbytes, 1) == 0
    assert hip.hipMemcpy(ptrs['S'], S.ctypes.data_as(ctypes.c_void_p), S.nbytes, 1) == 0
    H = ctx.fetch()['H']
    for deg, gamma in ((0, 0.2), (1, 0.35)):
        want = host_picks(alpha, C, S, deg, gamma)
        ctx.select_launch(deg)
        idx1, rows1 = ctx.select_fetch()
        ctx.select3_launch(deg, gamma)
        idx3, rows3 = ctx.select3_fetch()
        assert np.array_equal(idx3, want), (n, deg, idx3, want)
        assert np.array_equal(idx1, idx3[0]), (n, deg, idx1, idx3[0])
        if n <= 4:
            assert np.all(idx1 == -1)
        assert want[0, 5] == -1 and want[0, 6] == -1 and want[1, 6] == -1 and want[2, 6] == -1
        for c in range(7):
            for a in range(3):
                k = idx3[a, c]
                if k >= 0:
                    assert np.array_equal(rows3[a, c], H[c, k], equal_nan=True), (n, deg, a, c)
                else:
                    assert np.all(np.isnan(rows3[a, c])), (n, deg, a, c)
            assert np.array_equal(rows1[c], rows3[0, c], equal_nan=True), (n, deg, c)


@pytest.mark.parametrize('n_alpha', [4, 5, 8, 9, 63, 64, 65, 100, 130])
def test_device_picks_equal_the_host_analyzers_at_every_shape_and_after_a_second_upload(staged, n_alpha):
    """n_alpha 4: no fit (index -1, NaN row); 5: one break point; 8, 9: the n > 8 switch of the ranking; 63, 64, 65: the chunk
    edge of the running sums and of the candidate ballot; 100: the benchmark's size; 130: three chunks.  Both p2_deg.  A second
    upload on the same context with another mesh (other values, other spacing) gives the host's answers for THAT mesh: the table
    of alpha logarithms behind mxe_chains_upload is not stale."""
    ctx, v0, hip = staged
    alpha = np.array(synthetic.alpha_mesh(n_alpha)) * N_TAU
    check_mesh(ctx, v0, hip, alpha, seed=n_alpha)
    lo, hi = alpha.min(), alpha.max()
    t = (np.log(alpha) - np.log(lo)) / (np.log(hi) - np.log(lo))
    alpha2 = 0.5 * lo * (3.0 * hi / lo) ** (t ** 1.6)            # same order, other ends, not log-uniform
    check_mesh(ctx, v0, hip, alpha2, seed=1000 + n_alpha)
