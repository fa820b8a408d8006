"""Self-energy continuation on the host (no GPU): ArrayGf, the Sigma -> G_aux constructions of
InversionSigmaContinuator / DirectSigmaContinuator and their inverses S_w, the input checks that come before any
device call, get_G_tau_from_A_w, and persistence.  (The reference's sigma_continuator.py and maxent_util.py need TRIQS;
the closed-form semicircle stands in for its Gfs.)"""
import pickle

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device
from maxent_amd.sigma_continuator import fit_tail

BETA = 50.0
IOMEGA = (2 * np.arange(1025) + 1) * np.pi / BETA


def semicircle_iw(iomega, D=1.0, eps=0.0):
    """G(i w_n) of a semicircle of half-width D centred at eps: 2 (z - sqrt(z^2 - D^2)) / D^2, z = i w_n - eps,
    in the form without cancellation at large w_n"""
    z = 1j * iomega - eps
    r = np.sqrt(z * z - D * D)
    r = np.where((r / z).real < 0, -r, r)              # the branch with G ~ 1/z
    return 2.0 / (z + r)


def semicircle_w(w, D=1.0, eta=0.05):
    z = w + 1j * eta
    r = np.sqrt(z * z - D * D)
    r = np.where((r / z).real < 0, -r, r)
    return 2.0 / (z + r)


def rotation(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def test_array_gf_layout_copy_and_pickle():
    w = np.linspace(-3, 3, 11)
    g = mx.ArrayGf(w, 1.0 / (w + 0.5j))
    assert g.data.shape == (11, 1, 1) and g.data.dtype == complex and g.target_shape == (1, 1)
    assert [x.real for x in g.mesh] == list(w)
    np.testing.assert_array_equal(g.data[:, 0, 0], 1.0 / (w + 0.5j))
    c = g.copy()
    c.data[0, 0, 0] = 7.0
    assert g.data[0, 0, 0] != 7.0
    back = pickle.loads(pickle.dumps(g))
    assert np.array_equal(back.mesh, g.mesh) and np.array_equal(back.data, g.data)
    with pytest.raises(ValueError):
        mx.ArrayGf(w, np.zeros((11, 2, 3)))
    with pytest.raises(ValueError):
        mx.ArrayGf(w, np.zeros(10))


def test_inversion_on_a_semicircle():
    G = semicircle_iw(IOMEGA)
    S = 1j * IOMEGA + 2.4 - 1.0 / G
    for S_iw in (mx.ArrayGf(IOMEGA, S), (IOMEGA, S)):
        sc = mx.InversionSigmaContinuator(S_iw, 2.4)
        assert isinstance(sc.Gaux_iw, mx.ArrayGf) and sc.Gaux_iw.data.shape == (len(IOMEGA), 1, 1)
        assert np.array_equal(sc.Gaux_iw.mesh, IOMEGA)
        assert np.max(np.abs(sc.Gaux_iw.data[:, 0, 0] - G)) < 1e-12
        assert sc._constant_shift == {'0': 2.4}


def test_inversion_blocks():
    G1, G2 = semicircle_iw(IOMEGA), semicircle_iw(IOMEGA, D=2.0, eps=0.3)
    S = {'b1': mx.ArrayGf(IOMEGA, 1j * IOMEGA + 2.4 - 1 / G1), 'b2': (IOMEGA, 1j * IOMEGA + 3.3 - 1 / G2)}
    sc = mx.InversionSigmaContinuator(S, {'b1': 2.4, 'b2': 3.3})
    assert set(sc.Gaux_iw) == {'b1', 'b2'}
    assert np.max(np.abs(sc.Gaux_iw['b1'].data[:, 0, 0] - G1)) < 1e-12
    assert np.max(np.abs(sc.Gaux_iw['b2'].data[:, 0, 0] - G2)) < 1e-12
    # a scalar shift goes to every block
    sc = mx.InversionSigmaContinuator({'a': (IOMEGA, 1j * IOMEGA + 1.0 - 1 / G1),
                                       'b': (IOMEGA, 1j * IOMEGA + 1.0 - 1 / G2)}, 1.0)
    assert sc._constant_shift == {'a': 1.0, 'b': 1.0}
    assert np.max(np.abs(sc.Gaux_iw['b'].data[:, 0, 0] - G2)) < 1e-12


def test_inversion_of_a_matrix_sigma():
    Gd = np.zeros((len(IOMEGA), 2, 2), dtype=complex)
    Gd[:, 0, 0] = semicircle_iw(IOMEGA, D=1.0, eps=-0.4)
    Gd[:, 1, 1] = semicircle_iw(IOMEGA, D=1.5, eps=0.7)
    U = rotation(0.3)
    G = U @ Gd @ U.T
    C = 0.8
    S = (1j * IOMEGA + C)[:, None, None] * np.eye(2) - np.linalg.inv(G)
    sc = mx.InversionSigmaContinuator(mx.ArrayGf(IOMEGA, S), C)
    assert sc.Gaux_iw.target_shape == (2, 2)
    assert np.max(np.abs(sc.Gaux_iw.data - G)) < 1e-12
    # and back on the real axis: S_w = (w + C) 1 - G_w^-1
    w = np.linspace(-4, 4, 301)
    Gw = np.zeros((len(w), 2, 2), dtype=complex)
    Gw[:, 0, 0], Gw[:, 1, 1] = semicircle_w(w + 0.4), semicircle_w(w - 0.7, D=1.5)
    Gw = U @ Gw @ U.T
    sc.set_Gaux_w(mx.ArrayGf(w, Gw))
    want = (w + C)[:, None, None] * np.eye(2) - np.linalg.inv(Gw)
    np.testing.assert_allclose(sc.S_w.data, want, rtol=1e-13, atol=1e-13)


def test_tail_fit_of_a_semicircle():
    G = semicircle_iw(IOMEGA)
    c = fit_tail(IOMEGA, G - 1.3)
    assert abs(c[0] + 1.3) < 3e-8 and abs(c[1] - 1.0) < 3e-8
    assert np.isrealobj(c) and len(c) == 5


def test_direct_on_a_semicircle():
    G = semicircle_iw(IOMEGA)
    sc = mx.DirectSigmaContinuator(mx.ArrayGf(IOMEGA, G - 1.3))
    assert abs(sc._constant_shift['0'] + 1.3) < 1e-6
    assert abs(sc._norm['0'] - 1.0) < 1e-6
    assert np.max(np.abs(sc.Gaux_iw.data[:, 0, 0] - G)) < 1e-6
    # given values skip the fit
    sc2 = mx.DirectSigmaContinuator((IOMEGA, 2 * G + 0.5), constant_shift=0.5, norm=2.0)
    assert sc2._constant_shift == {'0': 0.5} and sc2._norm == {'0': 2.0}
    assert np.array_equal(sc2.Gaux_iw.data[:, 0, 0], (2 * G + 0.5 - 0.5) / 2.0)
    # blocks: a fit per block
    sc3 = mx.DirectSigmaContinuator({'up': (IOMEGA, G - 1.3), 'dn': (IOMEGA, 2 * G + 0.7)}, tail_fraction=0.3)
    assert abs(sc3._constant_shift['up'] + 1.3) < 1e-6 and abs(sc3._norm['dn'] - 2.0) < 1e-6
    assert abs(sc3._constant_shift['dn'] - 0.7) < 1e-6
    assert np.max(np.abs(sc3.Gaux_iw['dn'].data[:, 0, 0] - G)) < 1e-6


def test_direct_rejects_a_matrix_sigma():
    S = np.zeros((len(IOMEGA), 2, 2), dtype=complex)
    S[:, 0, 0] = S[:, 1, 1] = semicircle_iw(IOMEGA)
    with pytest.raises(NotImplementedError):
        mx.DirectSigmaContinuator(mx.ArrayGf(IOMEGA, S))


def test_set_gaux_w_gives_s_w():
    w = np.linspace(-5, 5, 401)
    Gw = semicircle_w(w)
    G = semicircle_iw(IOMEGA)
    inv = mx.InversionSigmaContinuator((IOMEGA, 1j * IOMEGA + 2.4 - 1 / G), 2.4)
    inv.set_Gaux_w(mx.ArrayGf(w, Gw))
    assert isinstance(inv.S_w, mx.ArrayGf) and np.array_equal(inv.S_w.mesh, w)
    np.testing.assert_allclose(inv.S_w.data[:, 0, 0], w + 2.4 - 1 / Gw, rtol=1e-15, atol=1e-14)
    assert inv.Gaux_w.data.shape == (len(w), 1, 1)
    d = mx.DirectSigmaContinuator((IOMEGA, G - 1.3))
    d.set_Gaux_w((w, Gw))
    c0, c1 = d._constant_shift['0'], d._norm['0']
    np.testing.assert_allclose(d.S_w.data[:, 0, 0], Gw * c1 + c0, rtol=1e-15, atol=1e-15)
    # blocks
    b = mx.InversionSigmaContinuator({'x': (IOMEGA, 1j * IOMEGA - 1 / G), 'y': (IOMEGA, 1j * IOMEGA + 1 - 1 / G)},
                                     {'x': 0.0, 'y': 1.0})
    b.set_Gaux_w({'x': mx.ArrayGf(w, Gw), 'y': mx.ArrayGf(w, 2 * Gw)})
    np.testing.assert_allclose(b.S_w['y'].data[:, 0, 0], w + 1.0 - 1 / (2 * Gw), rtol=1e-15, atol=1e-14)


def test_rejected_input_before_any_device_call():
    G = semicircle_iw(IOMEGA)
    w = np.linspace(-5, 5, 50)
    b = mx.InversionSigmaContinuator({'x': (IOMEGA, 1j * IOMEGA - 1 / G), 'y': (IOMEGA, 1j * IOMEGA - 1 / G)})
    with pytest.raises(Exception, match='not the same'):
        b.set_Gaux_w_from_Aaux_w({'x': np.ones(50), 'z': np.ones(50)}, w)
    with pytest.raises(Exception, match='not the same'):
        b.set_Gaux_w_from_Aaux_w(np.ones(50), w)
    with pytest.raises(IOError):
        b.set_Gaux_w({'x': mx.ArrayGf(w, np.ones(50))})
    s = mx.InversionSigmaContinuator((IOMEGA, 1j * IOMEGA - 1 / G))
    with pytest.raises(Exception, match='numpy ndarray'):
        s.set_Gaux_w_from_Aaux_w(list(np.ones(50)), w)
    with pytest.raises(NotImplementedError):
        s.set_Gaux_w(np.ones(50))
    with pytest.raises(Exception, match='wrong shape') as e:
        mx.get_G_w_from_A_w(np.ones((2, 3, 50)), w)
    assert not isinstance(e.value, mx.MaxEntDeviceError)
    with pytest.raises(Exception, match='wrong shape') as e:
        mx.get_G_w_from_A_w(np.ones((2, 50)), w)
    with pytest.raises(Exception, match='w_min') as e:
        mx.get_G_w_from_A_w(np.ones(50), w, w_min=3, w_max=2)
    assert not isinstance(e.value, mx.MaxEntDeviceError)
    with pytest.raises(NotImplementedError):
        mx.InversionSigmaContinuator(np.ones(10))


def test_get_G_tau_from_A_w():
    w = np.linspace(-5, 5, 201)
    A = np.exp(-w ** 2) / np.sqrt(np.pi)
    g = mx.get_G_tau_from_A_w(A, w, 10.0, 51)
    K = mx.TauKernel(np.linspace(0, 10.0, 51), mx.DataOmegaMesh(w), beta=10.0)
    assert g.data.shape == (51, 1, 1) and np.array_equal(g.mesh, np.linspace(0, 10.0, 51))
    np.testing.assert_array_equal(g.data[:, 0, 0].real, np.asarray(K.K_delta) @ A)
    assert np.all(g.data.imag == 0)
    g2 = mx.get_G_tau_from_A_w(A, mx.DataOmegaMesh(w), 10.0, 51)     # a mesh is taken as it is
    assert np.array_equal(g2.data, g.data)
    # G(tau = 0) + G(tau = beta) = -1 for a normalised A
    assert abs(g.data[0, 0, 0].real + g.data[-1, 0, 0].real + 1) < 1e-3


@pytest.mark.parametrize('kind', ['inversion', 'direct', 'blocks'])
def test_round_trips(kind):
    G = semicircle_iw(IOMEGA)
    w = np.linspace(-5, 5, 101)
    if kind == 'inversion':
        sc = mx.InversionSigmaContinuator((IOMEGA, 1j * IOMEGA + 2.4 - 1 / G), 2.4)
        sc.set_Gaux_w(mx.ArrayGf(w, semicircle_w(w)))
    elif kind == 'direct':
        sc = mx.DirectSigmaContinuator((IOMEGA, G - 1.3))
        sc.set_Gaux_w(mx.ArrayGf(w, semicircle_w(w)))
    else:
        sc = mx.InversionSigmaContinuator({'a': (IOMEGA, 1j * IOMEGA - 1 / G), 'b': (IOMEGA, 1j * IOMEGA + 1 - 1 / G)},
                                          {'a': 0.0, 'b': 1.0})
        sc.set_Gaux_w({'a': (w, semicircle_w(w)), 'b': (w, semicircle_w(w, D=2))})
    for back in (pickle.loads(pickle.dumps(sc)),
                 type(sc).__factory_from_dict__(type(sc).__name__, sc.__reduce_to_dict__())):
        assert type(back) is type(sc)
        assert back._constant_shift == sc._constant_shift
        if kind == 'direct':
            assert back._norm == sc._norm
        for attr in ('S_iw', 'Gaux_iw', 'Gaux_w', 'S_w'):
            a, b = getattr(sc, attr), getattr(back, attr)
            pairs = [(a[k], b[k]) for k in a] if isinstance(a, dict) else [(a, b)]
            assert not isinstance(a, dict) or set(a) == set(b)
            for x, y in pairs:
                assert np.array_equal(x.mesh, y.mesh) and np.array_equal(x.data, y.data)
