"""LegendreKernel on the host: the fill against 40-digit truth (tests/golden/make_golden_legendre.py), the convention
(TRIQS's GfLegendre normalisation) checked against the imaginary-time kernel, subsets and permutations of the orders,
argument refusals, the fill cache, the facade's switch between kernels and the helpers of maxent_util.  No GPU.
"""
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import kernels

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 2.0 ** -52
GRIDS = ['w200', 'w201z', 'wmid', 'wwide', 'wsmall', 'even', 'shuffled', 'l0']


def load(name):
    with np.load(os.path.join(GOLD, name + '.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def kk():
    return load('legendre_kernels')


def check_fill(got, truth, l, w, what):
    """relative error <= (8 + l) 2^-52 where |truth| >= 2^-1000, |K| < 2^-990 elsewhere, exact values at omega = 0.
    The bound follows the conditioning of e^{-a} i_l(a) in a = beta |omega| / 2, whose rounding the fill cannot avoid:
    roughly 1 + l (l + 1) / (2a) for large a, l for small a.  Returns the worst error in units of the bound."""
    assert got.shape == truth.shape and np.all(np.isfinite(got))
    big = np.abs(truth) >= 2.0 ** -1000
    bound = (8.0 + l)[:, None] * EPS * np.abs(truth)
    err = np.abs(got - truth)
    worst = (err[big] / bound[big]).max()
    i, j = np.unravel_index(np.argmax(np.where(big, err / np.where(big, bound, 1.0), 0.0)), err.shape)
    print('fill %s: worst error %.3f of the bound (%.1f x 2^-52 at l = %d, omega = %g)'
          % (what, worst, err[i, j] / abs(truth[i, j]) / EPS, l[i], w[j]))
    assert np.all(err[big] <= bound[big])
    assert np.all(np.abs(got[~big]) < 2.0 ** -990)
    zero = w == 0.0
    if zero.any():
        assert np.all(got[l == 0][:, zero] == truth[l == 0][:, zero]) and np.all(got[l != 0][:, zero] == 0.0)
    return worst


@pytest.mark.parametrize('name', GRIDS)
def test_host_fill_against_the_truth(kk, name):
    l, w, beta = kk['l_' + name], kk['w_' + name], float(kk['beta'])
    K = mx.LegendreKernel(l, mx.DataOmegaMesh(w), beta=beta)
    assert K.K.shape == (len(l), len(w)) and K.K.dtype == float
    check_fill(np.asarray(K.K), kk['K_' + name], l, w, name)
    np.testing.assert_array_equal(K.K_delta, np.asarray(K.K) * mx.DataOmegaMesh(w).delta[None, :])
    if name == 'w201z':
        assert K.K[0, 100] == -beta / 2 and not np.any(K.K[1:, 100])


def test_nothing_overflows_for_any_beta_omega():
    """a = beta |omega| / 2 = 1e4, where cosh overflows and exp(-2a) underflows: finite, K(0, omega) = -tanh / omega"""
    w = np.array([-500.0, -1.0, 0.0, 1e-300, 1.0, 500.0])
    with np.errstate(all='raise', under='ignore'):
        K = np.asarray(mx.LegendreKernel(np.arange(40), mx.DataOmegaMesh(w), beta=40.0).K)
    assert np.all(np.isfinite(K))
    np.testing.assert_allclose(K[0, [0, 1, 4, 5]], -np.tanh(20.0 * w[[0, 1, 4, 5]]) / w[[0, 1, 4, 5]], rtol=8 * EPS)
    assert K[0, 2] == -20.0 and K[0, 3] == -20.0 and not np.any(K[1:, 2])


def test_convention_against_the_imaginary_time_kernel():
    """independent of mpmath: sum_l sqrt(2l+1)/beta P_l(x(tau)) K(l, omega) = K_tau(tau, omega), and at tau = 0+,
    where P_l(-1) = (-1)^l, -(2/beta) sum_{l even} sqrt(2l+1) K(l, omega) = -(K_tau(0) + K_tau(beta)) = 1"""
    beta = 10.0
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=50)
    l = np.arange(120)
    K = np.asarray(mx.LegendreKernel(l, omega, beta=beta).K)
    tau = np.linspace(0, 10, 41)
    x = 2 * tau / beta - 1
    P = np.polynomial.legendre.legvander(x, 119)                        # (n_tau, 120)
    rec = (P * (np.sqrt(2 * l + 1) / beta)[None, :]) @ K
    Kt = np.asarray(mx.TauKernel(tau, omega, beta=10).K)
    assert np.abs(rec - Kt)[1:-1].max() <= 1e-12
    even = l[::2]
    assert np.abs(-(2 / beta) * (np.sqrt(2 * even + 1)[:, None] * K[::2]).sum(axis=0) - 1).max() <= 1e-10
    w = np.asarray(omega)
    np.testing.assert_allclose(K[0], -np.tanh(beta * w / 2) / w, rtol=8 * EPS)


def test_subsets_and_permutations_are_rows_of_the_contiguous_fill(kk):
    omega = mx.DataOmegaMesh(kk['w_w200'])
    beta = float(kk['beta'])
    full = np.asarray(mx.LegendreKernel(np.arange(30), omega, beta=beta).K)
    for name in ('even', 'shuffled'):
        l = kk['l_' + name]
        sub = mx.LegendreKernel(l, omega, beta=beta)
        assert np.array_equal(np.asarray(sub.K), full[l]), name
        assert np.array_equal(sub.data_variable, l)
    assert list(kk['l_even']) == list(range(0, 30, 2)) and sorted(kk['l_shuffled']) == list(range(10))


def test_argument_refusals():
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=20)
    with pytest.raises(ValueError, match='beta'):
        mx.LegendreKernel(np.arange(5), omega)
    with pytest.raises(ValueError, match='beta'):
        mx.LegendreKernel(np.arange(5), omega, beta=0.0)
    for bad in ([0, 1.5, 2], [0, -1, 2], [0, 1, 1], [[0, 1], [2, 3]], [], [0, np.nan], [0, 5000]):
        with pytest.raises(ValueError, match=r'\bl\b'):
            mx.LegendreKernel(bad, omega, beta=10.0)
    K = mx.LegendreKernel([0.0, 2.0, 1.0], omega, beta=10.0)            # integer-valued floats are integers
    assert K.l.dtype == np.int64 and list(K.l) == [0, 2, 1]
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    with pytest.raises(ValueError, match='beta'):
        tm.set_G_l_data(np.ones(4), None)
    with pytest.raises(AssertionError, match='real'):
        tm.set_G_l_data(np.ones(4) + 0j, 10.0)
    with pytest.raises(AssertionError, match='dimension'):
        tm.set_G_l_data(np.ones(4), 10.0, l=[0, 1, 2])
    with pytest.raises(ValueError, match=r'\bl\b'):
        tm.set_G_l_data(np.ones(3), 10.0, l=[0, 1, 1])
    assert isinstance(tm.K, mx.TauKernel)                               # refused data leave the object as it was


def test_cache_returns_the_same_frozen_arrays_for_equal_grids():
    w = np.linspace(-5, 5, 31)
    a = mx.LegendreKernel(np.arange(12), mx.DataOmegaMesh(w), beta=7.0)
    b = mx.LegendreKernel(list(range(12)), mx.DataOmegaMesh(w.copy()), beta=7.0)
    assert a.K is b.K and a.K_delta is b.K_delta and not a.K.flags.writeable
    with pytest.raises(ValueError):
        a.K[0, 0] = 1.0
    c = mx.LegendreKernel(np.arange(12), mx.DataOmegaMesh(w), beta=8.0)
    assert c.K is not a.K
    # a key of its own kind: a tau grid of the same values is another kernel
    t = mx.TauKernel(np.arange(12.0), mx.DataOmegaMesh(w), beta=7.0)
    assert t.K is not a.K and not np.array_equal(t.K, a.K)
    # rotation, fold and unfold as the other kernels
    T = np.linalg.qr(np.random.RandomState(0).randn(12, 12))[0]
    a.transform(T)
    np.testing.assert_allclose(a.K, T @ np.asarray(b.K), atol=1e-13)
    assert a.rotation is T and a.fold(w) is w and a.unfold(w) is w
    a.transform(None)
    np.testing.assert_allclose(a.K, b.K, atol=1e-13)


def test_the_facade_switches_between_the_kernels_and_refills_only_on_change():
    g = load('legendre')
    beta = 10.0
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.DataOmegaMesh(g['omega'])
    G_l = mx.get_G_l_from_A_w(g['A_true'], g['omega'], np.arange(30), beta)
    tm.set_G_l_data(G_l, beta)
    K = tm.K
    assert type(K) is mx.LegendreKernel and np.array_equal(tm.tau, np.arange(30)) and K.beta == beta
    assert np.array_equal(tm.G, G_l) and tm.K.K.shape == (30, 200)
    filled = K.K
    tm.set_G_l_data(2 * G_l, beta)                                      # same l, same beta: the same kernel and matrix
    assert tm.K is K and K.K is filled
    tm.set_G_l_data(G_l[::2], beta, l=np.arange(0, 30, 2))              # another l: refilled
    assert tm.K is K and K.K.shape == (15, 200) and np.array_equal(K.K, np.asarray(filled)[::2])
    tm.set_G_l_data(G_l[::2], 2 * beta, l=np.arange(0, 30, 2))          # another beta: refilled
    assert K.beta == 2 * beta and not np.array_equal(K.K, np.asarray(filled)[::2])
    # inside a PreblurKernel
    tm.K = mx.PreblurKernel(K=mx.LegendreKernel(np.arange(30), tm.omega, beta=beta), b=0.1)
    tm.set_G_l_data(G_l, beta)
    assert type(tm.K) is mx.PreblurKernel and type(tm.K.kernel) is mx.LegendreKernel
    # and back to G(tau)
    tau = np.linspace(0, beta, 21)
    tm.K = tm.K.kernel
    tm.set_G_tau_data(tau, mx.get_G_tau_from_A_w(g['A_true'], g['omega'], beta, 21).data[:, 0, 0])
    assert type(tm.K) is mx.TauKernel and np.array_equal(tm.tau, tau) and tm.K.K.shape == (21, 200)
    assert kernels.LegendreKernel is mx.LegendreKernel


def test_elementwise_setters_take_the_shapes_of_the_tau_setters():
    g = load('legendre_elementwise')
    ew = mx.ElementwiseMaxEnt()
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.DataOmegaMesh(g['omega'])
    ew.set_G_l_data(g['G_l'], float(g['beta']))
    assert tuple(ew.shape) == (2, 2) and np.array_equal(ew.tau, g['l'])
    assert type(ew.maxent_diagonal.K) is mx.LegendreKernel and type(ew.maxent_offdiagonal.K) is mx.LegendreKernel
    with pytest.raises(AssertionError):
        ew.set_G_l_data(g['G_l'][0, 0], float(g['beta']))
    with pytest.raises(AssertionError, match='use_complex'):
        ew.set_G_l_bins(np.ones((4, 2, 2, 30)) + 1j * np.random.RandomState(0).randn(4, 2, 2, 30), 40.0)


def test_G_tau_from_G_l_from_A_w_is_G_tau_from_A_w():
    g = load('legendre')
    beta, l = 10.0, np.arange(120)
    G_l = mx.get_G_l_from_A_w(g['A_true'], g['omega'], l, beta)
    assert G_l.shape == (120,)
    want = mx.get_G_tau_from_A_w(g['A_true'], g['omega'], beta, 41)
    got = mx.get_G_tau_from_G_l(G_l, l, want.mesh, beta)
    assert got.shape == (41,) and np.abs(got - want.data[:, 0, 0]).max() <= 1e-10
    # a leading axis and a subset of the orders
    both = mx.get_G_tau_from_G_l(np.stack([G_l, 2 * G_l]), l, want.mesh, beta)
    assert both.shape == (2, 41) and np.array_equal(both[0], got) and np.array_equal(both[1], 2 * got)
    ev = mx.get_G_tau_from_G_l(G_l[::2], l[::2], want.mesh, beta)
    np.testing.assert_allclose(ev, 0.5 * (got + got[::-1]), atol=1e-13)     # the even orders: the part even in x


def _truncated_eigenbasis(bins):
    """sigma, T (rows) and the mean of (n_bins, n) bins with n_bins <= n: the covariance of the mean has n_bins - 1
    directions, T has fewer rows than columns"""
    x = np.asarray(bins, dtype=np.longdouble)
    nb = x.shape[0]
    X = (x - x.mean(axis=0)) / np.sqrt(np.longdouble(nb) * (nb - 1))
    var, vec = np.linalg.eigh(np.asarray(X.T @ X, dtype=float))
    keep = var >= 1e-20
    assert keep.sum() == nb - 1
    return np.sqrt(var[keep]), vec[:, keep].T.copy(), np.asarray(x.mean(axis=0), dtype=float)


@pytest.mark.parametrize('kind', ['legendre', 'preblur', 'data', 'tau'])
def test_a_second_truncated_eigenbasis_rotates_the_kernel_itself(kind):
    """what the element-wise drivers do with bins (legendre_bins.npz: 12 bins of 12 coefficients, 11 directions): one
    worker takes the eigenbasis of one matrix element after the other.  T_old^H T_old is a projection, so a hop from
    the old rotation would hand the second element T_new applied to a projected kernel; it gets T_new K"""
    b = load('legendre_bins')
    beta, l, omega = float(b['beta']), b['e_l'], mx.DataOmegaMesh(b['omega'])
    tm = mx.TauMaxEnt(cost_function='plusminus')
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = omega
    K0 = np.array(mx.LegendreKernel(l, omega, beta=beta).K)
    if kind == 'preblur':
        tm.K = mx.PreblurKernel(K=mx.LegendreKernel(l, omega, beta=beta), b=0.1)
        K0 = np.array(mx.PreblurKernel(K=mx.LegendreKernel(l, omega, beta=beta), b=0.1).K)
    elif kind == 'data':
        tm.K = mx.DataKernel(l, omega, K0.copy())
    elif kind == 'tau':
        tau = np.linspace(0, beta, len(l))
        K0 = np.array(mx.TauKernel(tau, omega, beta=beta).K)
    nrm = np.linalg.norm(K0, 2)
    for i, j in ((0, 1), (1, 0), (0, 1)):
        sigma, T, mean = _truncated_eigenbasis(b['e_bins'][:, i, j, :])
        assert T.shape == (11, 12)
        if kind == 'tau':
            tm.set_G_tau_data(tau, mean)
        elif kind == 'data':
            tm.G = mean
            tm._adopt_data()
        else:
            tm.set_G_l_data(mean, beta, l)
        tm._set_eigenbasis(sigma, T)
        assert tm.K.rotation is T and np.array_equal(tm.err, sigma)
        assert np.abs(np.asarray(tm.K.K) - T @ K0).max() <= 8 * EPS * nrm, (i, j)
        assert np.abs((tm.K.U * tm.K.S) @ tm.K.V.T - T @ K0).max() <= 64 * EPS * nrm, (i, j)
        np.testing.assert_allclose(np.asarray(tm.G), T @ mean, rtol=0, atol=8 * EPS * np.abs(mean).max())
    # a square rotation is left by the hop, as ever: the kernel object keeps its decomposition
    var, vec = np.linalg.eigh(np.cov(b['e_bins'][:, 0, 0, :4].T))
    t4 = mx.TauMaxEnt()
    t4.set_verbosity(mx.VerbosityFlags.Quiet)
    t4.omega = omega
    t4.set_G_l_data(b['e_bins'][0, 0, 0, :4], beta)
    V = t4.K.V
    t4._set_eigenbasis(np.sqrt(var), vec.T.copy())
    t4._set_eigenbasis(np.sqrt(var), vec.T[::-1].copy())
    assert t4.K.V is V


def test_a_data_kernel_keeps_the_matrix_it_was_given_through_hops():
    """set_cov (truncated), set_error, set_cov on a DataKernel: transform(T1) -> transform(None) -> transform(T2) leaves
    a projected matrix, as in the reference; refill_unrotated goes back to the matrix that was given, not to the
    projection the second hop started from"""
    b = load('legendre_bins')
    omega = mx.DataOmegaMesh(b['omega'])
    K0 = np.array(mx.LegendreKernel(b['e_l'], omega, beta=float(b['beta'])).K)
    _, T1, _ = _truncated_eigenbasis(b['e_bins'][:, 0, 1, :])
    _, T2, _ = _truncated_eigenbasis(b['e_bins'][:, 1, 0, :])
    K = mx.DataKernel(b['e_l'], omega, K0.copy())
    K.transform(T1)
    K.transform(None)
    assert K._projected and np.abs(np.asarray(K.K) - K0).max() > 1e-3        # (T1^H T1 K0: the reference's hop)
    K.transform(T2)
    K.refill_unrotated()
    assert K.rotation is None and not K._projected and np.array_equal(K.K, K0)
    K.transform(T2)
    assert np.array_equal(K.K, T2 @ K0)
    np.testing.assert_allclose((K.U * K.S) @ K.V.T, T2 @ K0, rtol=0, atol=64 * EPS * np.linalg.norm(K0, 2))


def test_the_facade_refuses_a_bad_beta_before_it_changes_anything():
    g = load('legendre')
    tm = mx.TauMaxEnt()
    tm.omega = mx.DataOmegaMesh(g['omega'])
    tm.set_G_l_data(g['data'], 40.0)
    filled = tm.K.K
    for beta in (-1.0, 0.0, np.inf, None):
        with pytest.raises(ValueError, match='beta'):
            tm.set_G_l_data(g['data'], beta)
        assert tm.K.beta == 40.0 and tm.K.K is filled
    # the work of a column grows like beta |omega| / 2: the cap of the device entry holds on the host too
    with pytest.raises(ValueError, match='omega'):
        mx.LegendreKernel(np.arange(3), mx.DataOmegaMesh(np.array([-1.0, 0.0, 1.0])), beta=2.1e6)
