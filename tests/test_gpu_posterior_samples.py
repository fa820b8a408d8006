"""Posterior samples on the device (mxe_posterior_sample, mxe_normals) against the numpy mirror of the generator and the
extended-precision truth of test_posterior_samples_host.py.

Gates.  Normals: |dz| <= 1e-13 (both sides evaluate the same rounded arguments; a few ulp of log, sqrt, sin and cos times
|z| < 8.7 are 2e-14).  Samples with handed-in normals: |delta_i - truth_i| <= 1e-6 sqrt(Gamma_ii) for every sample and
point, and |f^T delta - f^T truth| <= 1e-6 sqrt(f^T Gamma f) for the norm, three windows and the first moment wherever
var / prior >= 1e-8 (the project's gate for the Woodbury difference, as in test_gpu_posterior_errors.py).  Where the
basis (V', c) is the library's own (per-tau errors, a covariance) the unit vectors are handed in as z, which gives a
factor F of the covariance whatever the signs and the order of the basis; every column obeys the first gate, so by
Cauchy-Schwarz |(F F^T - Gamma)_ij| <= 2e-6 sqrt(n_z) sqrt(Gamma_ii Gamma_jj) (+ second order).  Statistics with 4096
device-generated samples: variance within 5 sqrt(2 / 4095) of mxe_posterior_var's, mean within 5 standard errors of 0.
Worst measured figures are printed (``-s``) and recorded in DESIGN.md section 4q.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_posterior_samples_host import truth_samples, prototype       # noqa: E402
import maxent_amd as mx                                                # noqa: E402
from maxent_amd import device, synthetic, posterior                    # noqa: E402

pytestmark = pytest.mark.gpu

GATE, R_MIN = 1e-6, 1e-8
STAT_SEED = 2026


class Problem(object):
    """a kernel with its SVD (numpy), one normal and one plus-minus element staged with the scalar error sigma"""

    def __init__(self, n_tau, n_omega, sigma=1e-3, keep=None, beta=10.0, half_width=5.0):
        tau = np.linspace(0.0, beta, n_tau)
        w = np.linspace(-half_width, half_width, n_omega)
        # exp(-tau w) / (1 + exp(-beta w)), without overflow
        K = np.exp(-np.outer(tau, w) - np.logaddexp(0.0, -beta * w)[None, :])
        U, S, Vt = np.linalg.svd(K, full_matrices=False)
        ns = int(np.sum(S > 1e-14 * S[0]))
        ns = ns if keep is None else min(ns, keep)
        self.U, self.S, self.V = U[:, :ns].copy(), S[:ns].copy(), Vt[:ns].T.copy()
        self.K = np.dot(self.U * self.S, self.V.T)                    # the kernel the device sees
        self.omega, self.n_tau, self.n_omega, self.ns, self.sigma = w, n_tau, n_omega, ns, sigma
        dw = w[1] - w[0]
        self.H = (0.6 * np.exp(-(w - 1.0) ** 2 / 0.5) + 0.4 * np.exp(-(w + 1.5) ** 2 / 0.8) + 1e-4) * dw
        self.Hpm = self.H * np.sin(1.3 * w)                          # (a plus-minus image changes sign)
        self.D = np.full(n_omega, dw / (2 * half_width))
        self.F = np.concatenate([np.ones((1, n_omega)), posterior.window_rows(w, [(-3.0, 0.0), (0.0, 2.0), (2.0, 4.5)]), w[None, :]])

    def context(self, err=None):
        ctx = device.DeviceContext(self.U, self.S, self.V)
        ds = ctx.add_dataset(self.sigma * np.ones(self.n_tau) if err is None else err)
        G = np.dot(self.K, self.H)
        ctx.set_elements([ds, ds], [G, G], np.tile(self.D, (2, 1)), [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS])
        return ctx

    def weights(self, kind):
        return self.H if kind == 0 else np.sqrt(self.Hpm ** 2 + 4.0 * self.D ** 2)

    def image(self, kind):
        return self.H if kind == 0 else self.Hpm


@pytest.fixture(scope='module')
def small():
    p = Problem(24, 37, keep=11)          # rank below 16, 37 = 2 tiles + 5 points
    assert p.ns < 16
    return p


@pytest.fixture(scope='module')
def cfg1():
    return Problem(100, 200)


def gate(label, pr, d, d_t, gamma, alpha, w, eta=1.0):
    """the two gates of the module docstring on the samples d (n_samples, n_omega) against the truth"""
    d, d_t, gamma = np.asarray(d, dtype=np.longdouble), np.asarray(d_t), np.asarray(gamma)
    assert np.all(np.isfinite(d.astype(float))), label
    sd = np.sqrt(np.diag(gamma))
    point = np.abs(d - d_t) / sd[None, :]
    F = np.asarray(pr.F, dtype=np.longdouble)
    var = np.einsum('fi,ij,fj->f', F, gamma, F)
    prior = np.dot(F ** 2, np.asarray(w, dtype=np.longdouble)) / np.longdouble(alpha)
    inside = var / prior >= R_MIN
    fun = np.abs(np.dot(d - d_t, F.T)) / np.sqrt(var)[None, :]
    i = np.unravel_index(np.argmax(point), point.shape)
    print('%s: worst point-wise %.2e sqrt(Gamma_ii) (sample %d, omega index %d, Gamma_ii alpha / w_i = %.2e), worst functional '
          '%.2e sqrt(var) (%d of %d inside r >= %.0e)' % (label, float(point[i]), i[0], i[1],
          float(gamma[i[1], i[1]] * alpha / w[i[1]]), float(fun[:, inside].max()) if inside.any() else 0.0,
          int(inside.sum()), len(inside), R_MIN))
    assert float(point.max()) <= GATE, (label, float(point.max()))
    assert inside.any() and float(fun[:, inside].max()) <= GATE, label
    return float(point.max())


def test_device_normals_against_the_numpy_mirror():
    for seed, stream, n_s, n in ((0, 0, 3, 8), (20261018, 2 ** 40 + 17, 33, 217), (2 ** 64 - 1, 2 ** 64 - 1, 1, 1), (7, 1, 5, 4099)):
        z = device.normals(seed, stream, n_s, n)
        ref = posterior.sample_normals(seed, stream, n_s, n)
        print('normals (%d, %d): worst |dz| %.2e' % (n_s, n, np.abs(z - ref).max()))
        assert z.shape == ref.shape and np.abs(z - ref).max() <= 1e-13


@pytest.mark.parametrize('n_samples', [1, 16, 17, 33])
def test_exactness_with_handed_in_normals_small(small, n_samples):
    pr = small
    ctx = pr.context()
    alphas = np.array([0.3, 30.0, 3.0e3])
    el = np.array([0, 1, 0])
    z = np.stack([posterior.sample_normals(5, s, n_samples, pr.n_omega + pr.ns) for s in range(3)])
    H = np.stack([pr.image(k) for k in el])
    got = ctx.posterior_sample(el, alphas, H=H, n_samples=n_samples, z=z)
    scaled = ctx.posterior_sample(el, alphas, H=H, n_samples=n_samples, z=z, chi2_factor=2.5)
    ctx.close()
    assert got.shape == (3, n_samples, pr.n_omega)
    for p in range(3):
        w = pr.weights(el[p])
        for eta, res in ((1.0, got), (2.5, scaled)):
            d_t, gamma = truth_samples(pr.K, pr.sigma, w, alphas[p], pr.V, pr.S / pr.sigma, z[p], eta=eta)
            gate('small n_samples=%d problem %d eta=%g' % (n_samples, p, eta), pr, res[p], d_t, gamma, alphas[p], w, eta)


def test_exactness_cfg1_size(cfg1):
    pr = cfg1
    assert 16 < pr.ns <= 64
    ctx = pr.context()
    alphas = np.array([2.0, 2.0e2])
    z = np.stack([posterior.sample_normals(6, s, 17, pr.n_omega + pr.ns) for s in range(2)])
    got = ctx.posterior_sample([0, 1], alphas, H=np.stack([pr.H, pr.Hpm]), n_samples=17, z=z)
    ctx.close()
    for p in range(2):
        w = pr.weights(p)
        d_t, gamma = truth_samples(pr.K, pr.sigma, w, alphas[p], pr.V, pr.S / pr.sigma, z[p])
        gate('cfg1 size problem %d' % p, pr, got[p], d_t, gamma, alphas[p], w)


def test_exactness_128_row_build():
    n_tau, n_omega = 1000, 300
    tau, omega, K, G = synthetic.single_G(n_tau, n_omega)
    K.reduce_singular_space(1e-14)
    assert 64 < len(K.S) <= 128
    U, S, V = np.array(K.U), np.array(K.S), np.array(K.V)
    w = np.asarray(omega)
    H = (synthetic.two_gaussian_spectrum(w) + 1e-4) * np.asarray(omega.delta)
    ctx = device.DeviceContext(U, S, V)
    ds = ctx.add_dataset(synthetic.SIGMA * np.ones(n_tau))
    ctx.set_elements([ds], [G], synthetic.flat_D(omega)[np.newaxis, :], [device.ENTROPY_NORMAL])
    z = posterior.sample_normals(8, 0, 17, n_omega + len(S))[np.newaxis]
    alpha = 50.0
    got = ctx.posterior_sample([0], [alpha], H=H[np.newaxis], n_samples=17, z=z)
    ctx.close()
    d_t, gamma = truth_samples(np.dot(U * S, V.T), synthetic.SIGMA, H, alpha, V, S / synthetic.SIGMA, z[0])

    class _F(object):
        F = np.concatenate([np.ones((1, n_omega)), posterior.window_rows(w, [(-3.0, 0.0), (0.0, 2.0), (4.0, 9.0)]), w[None, :]])
    gate('128-row build', _F, got[0], d_t, gamma, alpha, H)


def test_per_tau_errors_give_a_factor_of_the_covariance(small):
    pr = small
    err = pr.sigma * (1.0 + np.random.RandomState(4).rand(pr.n_tau))
    ctx = pr.context(err)
    nz = pr.n_omega + pr.ns
    alpha = 5.0
    for kind in (0, 1):
        F = ctx.posterior_sample([kind], [alpha], H=pr.image(kind)[np.newaxis], n_samples=nz, z=np.eye(nz)[np.newaxis])[0].T
        w = pr.weights(kind)
        _, gamma = truth_samples(pr.K, err, w, alpha, np.zeros((pr.n_omega, 1)), np.zeros(1), np.zeros((1, pr.n_omega + 1)))
        sd = np.sqrt(np.diag(gamma)).astype(float)
        worst = np.max(np.abs(np.dot(F, F.T) - gamma.astype(float)) / np.outer(sd, sd))
        print('per-tau errors, kind %d: worst |F F^T - Gamma|_ij / sqrt(Gamma_ii Gamma_jj) %.2e' % (kind, worst))
        assert worst <= 2.0 * GATE * np.sqrt(nz)
    ctx.close()


def test_generated_equals_handed_in_and_bits_do_not_depend_on_the_batch(small):
    pr = small
    ctx = pr.context()
    nz = pr.n_omega + pr.ns
    seed, stream = 31, 2 ** 33 + 5
    alone = ctx.posterior_sample([0], [7.0], H=pr.H[np.newaxis], n_samples=33, seed=seed, stream=[stream])
    z = device.normals(seed, stream, 33, nz)
    given = ctx.posterior_sample([0], [7.0], H=pr.H[np.newaxis], n_samples=33, z=z[np.newaxis])
    assert np.array_equal(alone, given)
    # cut out of a larger n_samples, and out of a smaller one
    more = ctx.posterior_sample([0], [7.0], H=pr.H[np.newaxis], n_samples=50, seed=seed, stream=[stream])
    one = ctx.posterior_sample([0], [7.0], H=pr.H[np.newaxis], n_samples=1, seed=seed, stream=[stream])
    assert np.array_equal(more[0, :33], alone[0]) and np.array_equal(one[0, 0], alone[0, 0])
    # a batch of 7 in shuffled order
    el = np.array([1, 0, 1, 0, 0, 1, 0])
    al = np.array([0.5, 3.0, 7.0, 7.0, 90.0, 2.0e3, 11.0])
    st = np.array([9, 8, 7, stream, 5, 4, 3], dtype=np.uint64)
    Hs = np.stack([pr.image(k) for k in el])
    batch = ctx.posterior_sample(el, al, H=Hs, n_samples=33, seed=seed, stream=st)
    assert np.array_equal(batch[3], alone[0])
    order = np.array([4, 2, 6, 0, 3, 5, 1])
    shuffled = ctx.posterior_sample(el[order], al[order], H=Hs[order], n_samples=33, seed=seed, stream=st[order])
    assert np.array_equal(shuffled, batch[order])
    assert not np.array_equal(batch[0], batch[2])                      # (another stream, another alpha)
    ctx.close()


def test_statistics_of_4096_generated_samples(small):
    pr = small
    alpha, n = 5.0, 4096
    # the seed passes these bounds with the numpy prototype fed the mirror's normals (checked without a device)
    zs = posterior.sample_normals(STAT_SEED, 3, n, pr.n_omega + pr.ns)
    proto = np.dot(prototype(pr.V, pr.S / pr.sigma, pr.H, alpha, zs), pr.F.T)
    ctx = pr.context()
    d = ctx.posterior_sample([0], [alpha], H=pr.H[np.newaxis], n_samples=n, seed=STAT_SEED, stream=[3])[0]
    var = ctx.posterior_var([0], [alpha], H=pr.H[np.newaxis], F=pr.F)['var'][0]
    ctx.close()
    for name, x in (('prototype', proto), ('device', np.dot(d, pr.F.T))):
        for j in range(len(pr.F)):
            mean, v = x[:, j].mean(), x[:, j].var(ddof=1)
            print('%s functional %d: mean %.2e standard errors, variance ratio - 1 = %+.3f' %
                  (name, j, mean / np.sqrt(var[j] / n), v / var[j] - 1))
            assert abs(v / var[j] - 1) <= 5.0 * np.sqrt(2.0 / (n - 1)), (name, j)
            assert abs(mean) <= 5.0 * np.sqrt(var[j] / n), (name, j)


def test_failure_handling_and_the_rows_of_the_last_launch(small):
    pr = small
    ctx = pr.context()
    with pytest.raises(device.MaxEntDeviceError, match='call order'):      # MXE_ERR_STATE: nothing launched yet
        ctx.posterior_sample([0], [1.0], n_samples=2)
    al = np.array([1.0, 10.0, 100.0])
    H = np.tile(pr.H, (3, 1))
    good = ctx.posterior_sample([0, 0, 0], al, H=H, n_samples=17, seed=1)
    Hn = H.copy()
    Hn[1, 5] = np.nan
    mixed = ctx.posterior_sample([0, 0, 0], al, H=Hn, n_samples=17, seed=1)       # (returns: MXE_OK)
    assert np.all(np.isnan(mixed[1])) and np.array_equal(mixed[[0, 2]], good[[0, 2]])
    Hz = H.copy()
    Hz[:, [0, 20, 36]] = 0.0                                                   # H underflowed: w_i = 0
    zero = ctx.posterior_sample([0, 0, 0], al, H=Hz, n_samples=17, seed=1)
    assert np.all(zero[:, :, [0, 20, 36]] == 0.0) and np.all(np.isfinite(zero)) and np.all(zero[:, :, 1] != 0.0)
    with pytest.raises(device.MaxEntDeviceError, match='invalid argument'):
        ctx._check(ctx._lib.mxe_posterior_sample(ctx._h, 1, device._p(np.zeros(1, np.int32)), device._p(np.ones(1)),
                                                 device._p(pr.H.copy()), None, 1.0, 0, 0, None, None, device._p(np.zeros(37)),
                                                 None), 'mxe_posterior_sample')
    with pytest.raises(ValueError, match='shape'):
        ctx.posterior_sample([0], [1.0], H=pr.H[np.newaxis], n_samples=2, z=np.zeros((1, 2, 5)))
    with pytest.raises(ValueError, match='not finite'):
        ctx.posterior_sample([0], [1.0], H=pr.H[np.newaxis], n_samples=1, z=np.full((1, 1, pr.n_omega + pr.ns), np.inf))
    # the rows of the last launch where they lie against the same rows handed in
    from maxent_amd import hostprep
    alphas = np.array([1.0, 10.0, 100.0, 1000.0]) * pr.n_tau
    v0 = np.stack([hostprep.initial_v(pr.V, pr.D, np.full(pr.n_omega, pr.omega[1] - pr.omega[0]), k)
                   for k in (device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS)])
    sol = ctx.solve_chains(np.arange(2), alphas, v0)
    pick = np.array([6, 1, 3])
    el, a = pick // 4, alphas[pick % 4]
    there = ctx.posterior_sample(el, a, problem_index=pick, n_samples=17, seed=2, stream=[1, 2, 3])
    rows = np.asarray(sol['H']).reshape(8, -1)[pick].copy()
    given = ctx.posterior_sample(el, a, H=rows, n_samples=17, seed=2, stream=[1, 2, 3])
    ctx.close()
    assert np.array_equal(there, given, equal_nan=True) and np.all(np.isfinite(given))


def quiet(obj):
    obj.set_verbosity(mx.VerbosityFlags.Quiet)
    return obj


def test_api_tau_maxent_and_elementwise():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 60, 120)
    ew = quiet(mx.ElementwiseMaxEnt())
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.alpha_mesh = synthetic.alpha_mesh(8)
    ew.set_error(synthetic.SIGMA)
    res = ew.run()
    out = ew.posterior_samples(res, n_samples=20, seed=4, alpha=3)
    assert out['H_samples'].shape == (2, 2, 20, 120) and out['seed'] == 4
    assert np.array_equal(out['H_samples'][1, 0], out['H_samples'][0, 1])             # hermitian partner mirrored
    np.testing.assert_array_equal(out['H'][0, 0], np.asarray(res.H[0][0][3]))
    np.testing.assert_allclose(out['A_samples'], out['H_samples'] / np.asarray(omega.delta), rtol=1e-15)
    assert not np.array_equal(out['H_samples'][0, 0] - out['H'][0, 0][None], out['H_samples'][1, 1] - out['H'][1, 1][None])
    with pytest.raises(ValueError, match='plus-minus'):
        ew.posterior_samples(res, n_samples=2, transform='log')
    every = ew.posterior_samples(res, n_samples=5, seed=4, alpha='all')
    assert every['H_samples'].shape == (2, 2, 8, 5, 120)
    assert np.array_equal(every['H_samples'][:, :, 3], out['H_samples'][:, :, :5])
    # the same element through TauMaxEnt: the same stream id (element (0, 0): flat index 0), the same bits
    tm = quiet(mx.TauMaxEnt(probability='normal'))
    tm.omega = omega
    tm.set_G_tau_data(tau, Gmat[0, 0])
    tm.set_error(synthetic.SIGMA)
    tm.alpha_mesh = synthetic.alpha_mesh(8)
    rt = tm.run()
    Ht = np.asarray(rt.H)
    one = tm.posterior_samples(rt, n_samples=20, seed=4, alpha=3)
    assert one['H_samples'].shape == (20, 120) and int(one['alpha_index']) == 3
    np.testing.assert_array_equal(one['H'], Ht[3])
    if np.array_equal(Ht[3], np.asarray(res.H[0][0][3])):
        assert np.array_equal(one['H_samples'], out['H_samples'][0, 0])
    spec = tm.maxent_loop.make_spec()
    d = posterior.device_samples(tm.K, [spec], [np.asarray(res.H[0][0][3])[None]], [np.asarray(rt.alpha)[[3]]], [[3]], 20, 4)[0][0]
    assert np.array_equal(np.asarray(res.H[0][0][3])[None] + d, out['H_samples'][0, 0])
    # 'linear' is H + delta; 'log' is positive and uses the same delta
    log = tm.posterior_samples(rt, n_samples=20, seed=4, alpha=3, transform='log')
    assert np.all(log['H_samples'] > 0)
    dl = one['H_samples'] - Ht[3][None]
    np.testing.assert_allclose(log['H_samples'], Ht[3][None] * np.exp(dl / Ht[3][None]), rtol=1e-9)
    # handed-in normals
    nz = 120 + len(np.array(tm.K.S))
    zz = posterior.sample_normals(4, 3, 20, nz)
    hand = tm.posterior_samples(rt, n_samples=20, alpha=3, z=zz)
    np.testing.assert_allclose(hand['H_samples'], one['H_samples'], rtol=0, atol=1e-11 * np.abs(dl).max())
    with pytest.raises(ValueError, match='z: the shape'):
        tm.posterior_samples(rt, n_samples=20, alpha=3, z=zz[:, :-1])
    # Bryan: the allotted alphas are returned; every sample is a draw around its own alpha's minimiser
    br = tm.posterior_samples(rt, n_samples=64, seed=4, alpha='bryan')
    assert br['alpha_index_samples'].shape == (64,) and br['H_samples'].shape == (64, 120)
    again = tm.posterior_samples(rt, n_samples=64, seed=4, alpha='bryan')
    assert np.array_equal(br['H_samples'], again['H_samples']) and np.array_equal(br['alpha_index_samples'], again['alpha_index_samples'])
    s0, a0 = 10, int(br['alpha_index_samples'][10])
    ref = tm.posterior_samples(rt, n_samples=64, seed=4, alpha=a0)
    assert np.array_equal(br['H_samples'][s0], ref['H_samples'][s0])
    # a NaN row is reported
    import pickle
    broken = pickle.loads(pickle.dumps(rt.data))
    Hb = np.array(broken.H)
    Hb[3, 7] = np.nan
    broken._saved['H'] = Hb
    bad = tm.posterior_samples(broken, n_samples=4, alpha=[2, 3])
    assert bad['info']['nan_rows'] == [3] and np.all(np.isnan(bad['H_samples'][1])) and np.all(np.isfinite(bad['H_samples'][0]))


def test_api_preblur_and_covariance():
    tau, omega, K, G = synthetic.single_G(60, 120)
    tm = quiet(mx.TauMaxEnt(cost_function='plusminus'))
    tm.omega = omega
    tm.set_G_tau_data(tau, G)
    t = np.linspace(0, synthetic.BETA, 60)
    cov = synthetic.SIGMA ** 2 * (np.eye(60) + 0.3 * np.exp(-np.abs(t[:, None] - t[None, :])))
    tm.set_cov(cov)
    tm.alpha_mesh = synthetic.alpha_mesh(6)
    b = 0.1
    tm.A_of_H = mx.PreblurA_of_H(b=b, omega=tm.omega)
    tm.K = mx.PreblurKernel(K=tm.K, b=b)
    res = tm.run()
    nz = 120 + len(np.array(tm.K.S))
    out = tm.posterior_samples(res, n_samples=nz, alpha=2, z=np.eye(nz))
    B = np.asarray(tm.A_of_H.matrix())
    np.testing.assert_allclose(out['A_samples'], np.dot(out['H_samples'], B.T), rtol=1e-12, atol=1e-12 * np.abs(out['A_samples']).max())
    # the unit vectors give a factor of the covariance in the rotated space of the data set
    F = (out['H_samples'] - out['H'][None]).T
    H = np.asarray(res.H[2])
    w = np.sqrt(H ** 2 + 4.0 * np.asarray(tm.D.D) ** 2)
    _, gamma = truth_samples(np.array(tm.K.K), np.asarray(tm.err), w, float(res.alpha[2]), np.zeros((120, 1)), np.zeros(1),
                             np.zeros((1, 121)))
    sd = np.sqrt(np.diag(gamma)).astype(float)
    # (H + delta - H rounds delta to an ulp of H: 1.1e-16 |H_i| per entry, beside the gate on delta itself)
    worst = np.max(np.abs(np.dot(F, F.T) - gamma.astype(float)) / np.outer(sd, sd))
    print('covariance + preblur: worst |F F^T - Gamma|_ij / sqrt(Gamma_ii Gamma_jj) %.2e' % worst)
    assert worst <= 2.0 * GATE * np.sqrt(nz)
