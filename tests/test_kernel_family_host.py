"""What the shared code of the kernel family owns, kind by kind: the fill cache and its read-only contract, fold / unfold
and the row counts, the rotation of a filled matrix, which kinds ``PreblurKernel.scan`` takes -- and the rule of
``TauMaxEnt._use_kernel`` (keep, refill once, or replace), through the public setters.
"""
import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device, kernels

BETA = 6.0
FULL = np.linspace(-4.0, 4.0, 9)
HALF = np.linspace(0.0, 4.0, 9)
TAU = np.linspace(0.0, BETA, 5)
NU_F = (2 * np.arange(5) + 1) * np.pi / BETA
NU_B = 2 * np.arange(5) * np.pi / BETA
L = np.array([4, 0, 2])


def _data_matrix(w):
    return np.random.RandomState(3).randn(4, len(w))


#: name -> (constructor on an omega mesh, its omega values, rows of K for n grid points, n, scannable)
KINDS = {
    'tau': (lambda om: mx.TauKernel(TAU, om, beta=BETA), FULL, 5, 5, True),
    'iomega': (lambda om: mx.IOmegaKernel(NU_F, om), FULL, 10, 5, False),
    'boson_tau': (lambda om: mx.BosonicTauKernel(TAU, om, beta=BETA), FULL, 5, 5, True),
    'boson_tau_symmetric': (lambda om: mx.BosonicTauKernel(TAU, om, beta=BETA, symmetric=True), HALF, 5, 5, True),
    'boson_iomega': (lambda om: mx.BosonicIOmegaKernel(NU_B, om), FULL, 10, 5, False),
    'boson_iomega_symmetric': (lambda om: mx.BosonicIOmegaKernel(NU_B, om, symmetric=True), HALF, 5, 5, False),
    'legendre': (lambda om: mx.LegendreKernel(L, om, beta=BETA), FULL, 3, 3, True),
    'data': (lambda om: mx.DataKernel(np.arange(4.0), om, _data_matrix(np.asarray(om))), FULL, 4, 4, False),
}


@pytest.fixture
def fresh_cache(monkeypatch):
    monkeypatch.setattr(kernels, '_recent_fill', kernels._Recent())


@pytest.mark.parametrize('name', sorted(KINDS))
def test_what_the_shared_code_owns(name, fresh_cache):
    make, w, n_rows, n, scannable = KINDS[name]
    K1, K2 = make(mx.DataOmegaMesh(w)), make(mx.DataOmegaMesh(w.copy()))
    filled = name != 'data'
    assert K1.K.shape == (n_rows, len(w)) and (K1.kind is not None) == filled
    assert np.array_equal(K1.K_delta, K1.K * K1.omega.delta[None, :])

    # ---- the fill cache hands the second object the first one's matrix, frozen
    if filled:
        assert K2.K is K1.K and K2.K_delta is K1.K_delta
        for a in (K1.K, K1.K_delta):
            with pytest.raises(ValueError, match='read-only'):
                a[0, 0] = 1.0
    K0 = np.array(K1.K)

    # ---- fold / unfold and the documented row counts: 2 n stacked, n otherwise
    rng = np.random.RandomState(5)
    if K1.stacked:
        assert n_rows == 2 * n and K1.n_iw == n
        z = rng.randn(2, n) + 1j * rng.randn(2, n)
        x = K1.unfold(z)
        assert x.dtype == float and x.shape == (2, 2 * n) and np.array_equal(x, kernels.stack_complex(z))
        assert np.array_equal(K1.fold(x), z)
        assert np.array_equal(K1.K_complex, K0[:n] + 1j * K0[n:])
        with pytest.raises(ValueError):
            K1.fold(x[:, :-1])
    else:
        assert n_rows == n
        z = x = rng.randn(2, n)
        assert K1.unfold(x) is x and K1.fold(x) is x
        if name == 'boson_iomega_symmetric':
            assert np.array_equal(K1.unfold(x + 1j), x) and np.array_equal(K1.K_complex, K0 + 0j)
    Kb = mx.PreblurKernel(K1, 0.3)
    assert np.array_equal(Kb.unfold(z), x) and np.array_equal(Kb.fold(x), z)     # (a PreblurKernel folds as its kernel)

    # ---- a filled matrix under a rotation: T K_unrotated, also after a refill; refill_unrotated gives the bits back
    T, _ = np.linalg.qr(rng.randn(n_rows, n_rows))
    K2.transform(T)
    assert K2.rotation is T and np.array_equal(K2.K, np.dot(T, K0))
    if filled:
        assert K1.K is not K2.K and np.array_equal(K1.K, K0)          # (the shared matrix is not the rotated one)
        K2.parameter_change()
        assert K2.rotation is T and np.array_equal(K2.K, np.dot(T, K0))
        assert np.array_equal(K2._K_unrotated, K0)
    else:
        with pytest.raises(NotImplementedError):
            K2.parameter_change()
    K2.refill_unrotated()
    assert K2.rotation is None and np.array_equal(K2.K, K0)
    if filled:
        assert K2.K is K1.K

    # ---- PreblurKernel.scan: unrotated TauKernel, BosonicTauKernel, LegendreKernel; everything else is refused
    assert K1.scannable == scannable and K1.has_device_entry
    if not scannable:
        with pytest.raises(NotImplementedError, match='unrotated TauKernel, BosonicTauKernel or LegendreKernel'):
            mx.PreblurKernel.scan(K1, [0.1, 0.2])
    elif device.device_count() < 1:
        with pytest.raises(device.MaxEntDeviceError, match='no HIP device'):
            mx.PreblurKernel.scan(K1, [0.1, 0.2])
    else:
        assert len(mx.PreblurKernel.scan(K1, [0.1, 0.2])) == 2
    if scannable:
        K2.transform(T)
        with pytest.raises(NotImplementedError, match='unrotated'):
            mx.PreblurKernel.scan(K2, [0.1])
    with pytest.raises(NotImplementedError, match='unrotated'):
        mx.PreblurKernel.scan(Kb, [0.1])


def test_equal_grid_values_of_different_kinds_do_not_collide(fresh_cache):
    grid = np.arange(1.0, 5.0)                             # tau, i omega_n, i nu_n and l alike
    made = []
    for _ in range(2):                                     # (more kinds than the cache holds: found there or filled again)
        om = mx.DataOmegaMesh(HALF)
        made.append([mx.TauKernel(grid, om, beta=BETA), mx.IOmegaKernel(grid, om, beta=BETA),
                     mx.BosonicTauKernel(grid, om, beta=BETA), mx.BosonicTauKernel(grid, om, beta=BETA, symmetric=True),
                     mx.BosonicIOmegaKernel(grid, om, beta=BETA), mx.BosonicIOmegaKernel(grid, om, beta=BETA, symmetric=True),
                     mx.LegendreKernel(grid, om, beta=BETA)])
    first, second = made
    for i, a in enumerate(first):
        assert np.array_equal(a.K, second[i].K)
        for b in first[i + 1:]:
            assert a.K is not b.K
            assert a.K.shape != b.K.shape or not np.array_equal(a.K, b.K)
    # two kinds alone, so that both fills are certainly in the cache when they are asked for again
    om = mx.DataOmegaMesh(FULL)
    Kt, Ki = mx.TauKernel(grid, om, beta=BETA), mx.IOmegaKernel(grid, om, beta=BETA)
    assert mx.TauKernel(grid, om, beta=BETA).K is Kt.K and mx.IOmegaKernel(grid, om, beta=BETA).K is Ki.K
    assert Kt.K.shape == (4, 9) and Ki.K.shape == (8, 9)


# ---- TauMaxEnt._use_kernel through the public setters -------------------------------------------------------------------

class Fills(object):
    """counts the calls of ``_compute`` per class (a refill from the cache would not count: every test starts with an
    empty cache and asks for matrices it has not asked for before)"""

    def __init__(self, monkeypatch):
        self.n = {}
        for cls in (mx.TauKernel, mx.IOmegaKernel, mx.BosonicTauKernel, mx.BosonicIOmegaKernel, mx.LegendreKernel):
            monkeypatch.setattr(cls, '_compute', self._wrap(cls, cls._compute))

    def _wrap(self, cls, compute):
        def counted(kernel, *args):
            self.n[cls] = self.n.get(cls, 0) + 1
            return compute(kernel, *args)
        return counted

    def take(self):
        n, self.n = self.n, {}
        return n


def _tm(preblur, first):
    """a TauMaxEnt after ``first(tm)``, its kernel then wrapped in a PreblurKernel if ``preblur``"""
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.DataOmegaMesh(HALF)
    first(tm)
    if preblur:
        tm.K = mx.PreblurKernel(tm.K, 0.2)
    return tm


def _check_blur(tm, preblur):
    """the PreblurKernel is still there and holds the blur of what its kernel holds now"""
    if preblur:
        assert isinstance(tm.K, mx.PreblurKernel)
        B = mx.get_preblur(tm.omega, 0.2)
        assert np.array_equal(tm.K.K, np.dot(tm.K.kernel.K, B * tm.omega.delta[:, None]))
    return tm._inner_kernel()


SETTERS = {
    'iomega': lambda tm, **kw: tm.set_G_iw_data(NU_F, np.ones(5) + 0.5j, **kw),
    'boson_tau': lambda tm, **kw: tm.set_chi_tau_data(TAU, np.ones(5), **kw),
    'boson_iomega': lambda tm, **kw: tm.set_chi_iw_data(NU_B, np.ones(5) + 0.5j, **kw),
    'legendre': lambda tm, **kw: tm.set_G_l_data(np.ones(3), kw.pop('beta', BETA), L, **kw),
}


@pytest.mark.parametrize('preblur', [False, True])
@pytest.mark.parametrize('other', sorted(SETTERS))
def test_a_tau_setter_replaces_the_other_filled_kinds(other, preblur, fresh_cache, monkeypatch):
    """rule a, first half: Matsubara, bosonic or Legendre data were there"""
    tm = _tm(preblur, SETTERS[other])
    assert tm._inner_kernel().kind == other
    fills = Fills(monkeypatch)
    tm.set_G_tau_data(TAU, -np.ones(5))
    assert type(tm.K) is mx.TauKernel and np.array_equal(tm.tau, TAU) and tm.K.omega is tm.omega
    assert fills.take() == {mx.TauKernel: 1}
    assert tm._stacked_kernel() is None


@pytest.mark.parametrize('preblur', [False, True])
def test_a_tau_setter_keeps_a_tau_kernel_and_a_data_kernel(preblur, fresh_cache, monkeypatch):
    """rule a, second half"""
    tm = _tm(preblur, lambda tm: tm.set_G_tau_data(TAU, -np.ones(5)))
    inner = tm._inner_kernel()
    fills = Fills(monkeypatch)
    tm.set_G_tau_data(TAU, -2.0 * np.ones(5))
    assert tm._inner_kernel() is inner and fills.take() == {}
    tm.set_G_tau_data(0.5 * TAU, -np.ones(5))                         # a new grid: the same object, filled once
    assert _check_blur(tm, preblur) is inner and np.array_equal(inner.tau, 0.5 * TAU)
    assert fills.take() == {mx.TauKernel: 1}

    tm = _tm(preblur, lambda tm: setattr(tm, 'K', mx.DataKernel(TAU, tm.omega, np.random.RandomState(4).randn(5, 9))))
    inner = tm._inner_kernel()
    tm.set_G_tau_data(TAU, -np.ones(5))
    assert _check_blur(tm, preblur) is inner and type(inner) is mx.DataKernel and fills.take() == {}
    tm.set_chi_tau_data(TAU, np.ones(5), beta=BETA)                   # any other kind replaces it
    assert type(tm.K) is mx.BosonicTauKernel


@pytest.mark.parametrize('preblur', [False, True])
@pytest.mark.parametrize('kind', ['iomega', 'boson_iomega'])
def test_a_matsubara_kernel_that_stays_takes_beta_without_a_refill(kind, preblur, fresh_cache, monkeypatch):
    """rule b"""
    tm = _tm(preblur, SETTERS[kind])
    inner = tm._inner_kernel()
    assert inner.beta == pytest.approx(BETA, rel=1e-14)               # from the spacing of the grid
    fills = Fills(monkeypatch)
    SETTERS[kind](tm, beta=7.5)
    assert _check_blur(tm, preblur) is inner and inner.beta == 7.5 and fills.take() == {}
    SETTERS[kind](tm)
    assert tm._inner_kernel() is inner and inner.beta == pytest.approx(BETA, rel=1e-14) and fills.take() == {}
    assert (tm._stacked_kernel() is inner) and tm.G.shape == (10,)


@pytest.mark.parametrize('preblur', [False, True])
def test_beta_in_the_matrix_refills_exactly_once(preblur, fresh_cache, monkeypatch):
    """rule c: BosonicTauKernel and LegendreKernel, beta alone and beta together with the grid"""
    tm = _tm(preblur, lambda tm: tm.set_chi_tau_data(TAU, np.ones(5), beta=BETA))
    inner = tm._inner_kernel()
    fills = Fills(monkeypatch)
    tm.set_chi_tau_data(TAU, 2.0 * np.ones(5), beta=BETA)
    assert tm._inner_kernel() is inner and fills.take() == {}
    tm.set_chi_tau_data(TAU, np.ones(5), beta=BETA + 1.0)
    assert _check_blur(tm, preblur) is inner and inner.beta == BETA + 1.0 and fills.take() == {mx.BosonicTauKernel: 1}
    tm.set_chi_tau_data(0.5 * TAU, np.ones(5), beta=BETA + 2.0)
    assert _check_blur(tm, preblur) is inner and inner.beta == BETA + 2.0 and np.array_equal(inner.tau, 0.5 * TAU)
    assert fills.take() == {mx.BosonicTauKernel: 1}
    assert np.array_equal(inner.K, mx.BosonicTauKernel(0.5 * TAU, tm.omega, beta=BETA + 2.0).K)
    tm.set_chi_tau_data(0.5 * TAU, np.ones(5), beta=BETA + 2.0, symmetric=True)     # another kernel, not a refill
    assert tm._inner_kernel() is not inner and tm.K.symmetric and fills.take() == {mx.BosonicTauKernel: 1}

    tm = _tm(preblur, lambda tm: tm.set_G_l_data(np.ones(3), BETA, L))
    inner = tm._inner_kernel()
    fills.take()
    tm.set_G_l_data(np.ones(3), BETA, L)
    assert tm._inner_kernel() is inner and fills.take() == {}
    tm.set_G_l_data(np.ones(3), BETA + 1.0, L)
    assert _check_blur(tm, preblur) is inner and inner.beta == BETA + 1.0 and fills.take() == {mx.LegendreKernel: 1}
    tm.set_G_l_data(np.ones(3), BETA + 2.0, [1, 5, 3])
    assert _check_blur(tm, preblur) is inner and inner.beta == BETA + 2.0 and np.array_equal(inner.l, [1, 5, 3])
    assert fills.take() == {mx.LegendreKernel: 1}
    assert np.array_equal(inner.K, mx.LegendreKernel([1, 5, 3], tm.omega, beta=BETA + 2.0).K)


@pytest.mark.parametrize('preblur', [False, True])
@pytest.mark.parametrize('start', ['legendre', 'boson_tau'])
def test_legendre_arguments_are_validated_before_anything_changes(start, preblur, fresh_cache, monkeypatch):
    """rule e: on a LegendreKernel that would stay and on a kernel that would be replaced"""
    tm = _tm(preblur, SETTERS[start])
    K, inner = tm.K, tm._inner_kernel()
    G, grid, beta, K_before = np.array(tm.G), np.array(tm.tau), inner.beta, inner.K
    fills = Fills(monkeypatch)
    for bad in (dict(beta=-1.0), dict(beta=np.inf), dict(beta=None), dict(l=[0, 2, 2]), dict(l=[0, -1, 2]),
                dict(l=[0.5, 1, 2])):
        with pytest.raises(ValueError, match='LegendreKernel'):
            tm.set_G_l_data(2.0 * np.ones(3), bad.get('beta', BETA + 1.0), bad.get('l', [1, 5, 3]))
        assert tm.K is K and tm._inner_kernel() is inner and inner.beta == beta and inner.K is K_before
        assert np.array_equal(tm.tau, grid) and np.array_equal(tm.G, G)
    assert fills.take() == {}
