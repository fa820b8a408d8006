"""The host fills every ordinary run goes through -- TauKernel, IOmegaKernel, get_preblur -- against 40-digit truth
(tests/golden/fermion_kernels.npz from tests/golden/make_golden_fermion_kernels.py), under the bounds the device
kernels are held to in tests/test_gpu_fill_truth.py.  That the plain numpy path meets them shows that the bounds are
conditions a correct binary64 evaluation satisfies, and that the fixture is right.

EPS = 2^-52.  Every entry is checked: where |truth| > 1e-300 ("big") the relative error is gated, elsewhere
|got| < 1e-290.

  tau fill       (8 + x) EPS, x = tau |w| for w >= 0, (beta - tau) |w| for w < 0: the rounded product in the exponent
                 costs x/2 ulp, the rounding of beta - tau on the negative half-axis as much again; exp, the sum and the
                 quotient a few ulp (the form of the bosonic gate, tests/test_boson_host.py)
  Matsubara fill 8 EPS
  blur matrix    (17 + n_omega/16 + 4 y) EPS, y = (w_l - w_i)^2 / (2 b^2): about 3 roundings in the exponent's
                 argument, each worth y; two sums of n_omega positive terms; a few quotients

Each test prints its worst ratio to the bound (pytest -s).
"""
import os
from fractions import Fraction

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd.preblur import get_preblur

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 2.0 ** -52
BIG = 1e-300
SMALL = 1e-290

TAU_GRIDS = ['tau', 'tau_one']
OMEGA_GRIDS = ['hyp67', 'wide41', 'zero']
PB_MESHES = ['lin2', 'lin3', 'hyp3', 'lin255', 'hyp255', 'lin257', 'hyp257', 'lin513', 'hyp513']


def load():
    with np.load(os.path.join(GOLD, 'fermion_kernels.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def fk():
    return load()


def check_entries(got, truth, bound, what):
    """every entry of ``got``: relative error <= ``bound`` (an array of truth's shape) where |truth| > 1e-300,
    |got| < 1e-290 elsewhere, nothing infinite or NaN.  Prints and returns the worst error in units of the bound."""
    got, truth = np.asarray(got), np.asarray(truth)
    bound = np.broadcast_to(bound, truth.shape)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert np.all(np.isfinite(got)), what
    big = np.abs(truth) > BIG
    L = np.longdouble
    rel = np.asarray(np.abs(got[big].astype(L) - truth[big].astype(L)) / np.abs(truth[big].astype(L)), dtype=float)
    ratio = rel / bound[big]
    worst = float(ratio.max()) if big.any() else 0.0
    tiny = float(np.abs(got[~big]).max()) if (~big).any() else 0.0
    print('%s: worst ratio to the bound %.3f (max rel %.2e), %d big entries, %d below 1e-300 (largest |got| there %.1e)'
          % (what, worst, rel.max() if big.any() else 0.0, big.sum(), (~big).sum(), tiny))
    assert np.all(ratio <= 1.0), (what, worst)
    assert tiny < SMALL, (what, tiny)
    return worst


def tau_bound(tau, w, beta):
    """(8 + x) EPS of the module docstring"""
    t, w = np.asarray(tau)[:, None], np.asarray(w)[None, :]
    x = np.where(w >= 0, t * np.abs(w), (beta - t) * np.abs(w))
    return (8 + x) * EPS


def blur_bound(w, rows, b):
    """(17 + n_omega/16 + 4 y) EPS for the rows ``rows`` of the blur matrix on ``w``"""
    y = (w[None, :] - w[rows][:, None]) ** 2 / (2 * b * b)
    return (17 + len(w) / 16.0 + 4 * y) * EPS


def blur_truth(fk, name, ib):
    """the stored rows of the blur matrix on mesh ``name`` for width number ``ib``: binary64 value plus remainder"""
    return fk['pb_B_' + name][ib].astype(np.longdouble) + fk['pb_Blo_' + name][ib].astype(np.longdouble)


def blur_longdouble(w, delta, b):
    """get_preblur's steps in np.longdouble, for the truth of a blur PRODUCT (which needs all of B, not the stored rows).
    The exponent y = (w_j - w_i)^2 / (2 b^2) is formed exactly, in fractions, and split into its binary64 value and
    the remainder, exp(-y) = exp(-y_hi) (1 - y_lo): y rounded to longdouble is off by y 2^-64, which is 4e-17 of the
    entry at y = 690, where the entries are still above 1e-300.  Pairs with y > 800 keep the binary64 estimate: their
    entries are below the smallest longdouble that matters here (e^-800 = 1e-348)."""
    L = np.longdouble
    n = len(w)
    fw = [Fraction(float(x)) for x in w]
    den = 2 * Fraction(float(b)) ** 2
    hi = (w[None, :] - w[:, None]) ** 2 / (2 * b * b)
    lo = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            if hi[i, j] <= 800.0:
                y = (fw[j] - fw[i]) ** 2 / den
                h = float(y)
                hi[i, j] = hi[j, i] = h
                lo[i, j] = lo[j, i] = float(y - Fraction(h))
    G = np.exp(-hi.astype(L)) * (1 - lo.astype(L)) / np.sqrt(2 * L(np.pi) * L(b) ** 2)
    dl = np.asarray(delta).astype(L)
    c = (G * dl[None, :]).sum(axis=1)                  # (G is symmetric: sum_k delta_k G[k][i] = sum_k G[i][k] delta_k)
    B1 = G / c[:, None]
    s = (B1 * dl[None, :]).sum(axis=1)
    return B1 / s[None, :]


def check_blur_longdouble(fk, name, ib, B):
    """the longdouble restatement against the stored rows of the fixture: 1e-17 relative where the truth is above 1e-300"""
    rows = fk['pb_rows_%d' % B.shape[0]]
    truth = blur_truth(fk, name, ib)
    big = np.abs(truth) > BIG
    rel = float((np.abs(B[rows][big] - truth[big]) / np.abs(truth[big])).max())
    print('longdouble blur matrix %s b=%g against the fixture: max rel %.2e' % (name, fk['pb_b'][ib], rel))
    assert rel <= 1e-17, (name, ib, rel)
    assert np.all(np.abs(B[rows][~big]) < SMALL)


def test_the_fixture_holds_what_the_tests_need(fk):
    beta = float(fk['beta'])
    assert beta == 40.0 and fk['tau'].shape == (36,) and fk['tau_one'].shape == (1,)
    assert {0.0, 1e-7, beta - 1e-7, beta / 3, beta} <= set(fk['tau']) and fk['tau_one'][0] == beta / 3
    assert np.all(np.diff(fk['tau']) > 0)
    assert fk['w_hyp67'].shape == (67,) and fk['w_wide41'].shape == (41,)
    assert np.array_equal(fk['w_zero'], [-1e-3, 0.0, 1e-300, 3.0])
    assert np.array_equal(fk['w_hyp67'], np.asarray(mx.HyperbolicOmegaMesh(-10, 10, 67)))
    assert np.array_equal(fk['w_wide41'], np.linspace(-60, 60, 41))
    assert np.array_equal(fk['iw'], (2 * np.arange(16) + 1) * np.pi / beta)
    # many entries of the wide grid are below the smallest binary64 number, and many are not
    Kw = fk['K_tau_wide41']
    assert (Kw == 0).sum() > 100 and (np.abs(Kw) > BIG).sum() > 100
    assert np.array_equal(fk['pb_b'], [1e-3, 0.05, 0.3, 50.0]) and np.array_equal(fk['pb_n'], [2, 3, 255, 257, 513])
    for name in PB_MESHES:
        n = int(name[3:])
        mesh = mx.DataOmegaMesh(np.linspace(-5, 5, n)) if name.startswith('lin') else mx.HyperbolicOmegaMesh(-5, 5, n)
        assert np.array_equal(fk['pb_w_' + name], np.asarray(mesh)) and np.array_equal(fk['pb_delta_' + name], mesh.delta)
        assert np.array_equal(fk['pb_rows_%d' % n], sorted({0, 1, n // 2, n - 2, n - 1}))
        assert fk['pb_B_' + name].shape == fk['pb_Blo_' + name].shape == (4, len(fk['pb_rows_%d' % n]), n)
        assert np.all(np.abs(fk['pb_Blo_' + name]) <= 0.5 * np.spacing(np.abs(fk['pb_B_' + name])))
    # the hyperbolic mesh is where the blur matrix is not symmetric: B[0][n-1] against B[n-1][0] differ on neither
    # mesh (both are mirror images), B[0][1] against B[1][0] differ on the hyperbolic one
    B = fk['pb_B_hyp257'][2]                          # b = 0.3, rows 0, 1, 128, 255, 256
    assert abs(B[0, 1] - B[1, 0]) > 1e-3 * abs(B[0, 1])


@pytest.mark.parametrize('tname', TAU_GRIDS)
@pytest.mark.parametrize('wname', OMEGA_GRIDS)
def test_host_tau_fill_against_the_truth(fk, wname, tname):
    tau, w, beta = fk[tname], fk['w_' + wname], float(fk['beta'])
    K = np.asarray(mx.TauKernel(tau, mx.DataOmegaMesh(w), beta=beta).K)
    truth = fk['K_%s_%s' % ('tau' if tname == 'tau' else 'tau_one', wname)]
    check_entries(K, truth, tau_bound(tau, w, beta), 'host tau fill %s x %s' % (tname, wname))
    if wname == 'zero':
        assert np.all(K[:, 1] == -0.5)


@pytest.mark.parametrize('wname', ['hyp67', 'zero'])
def test_host_matsubara_fill_against_the_truth(fk, wname):
    iw, w = fk['iw'], fk['w_' + wname]
    K = np.asarray(mx.IOmegaKernel(iw, mx.DataOmegaMesh(w)).K)
    check_entries(K, fk['K_iw_' + wname], 8 * EPS, 'host Matsubara fill ' + wname)
    assert np.all(K[fk['K_iw_' + wname] == 0.0] == 0.0)


@pytest.mark.parametrize('name', PB_MESHES)
def test_host_get_preblur_against_the_truth(fk, name):
    w, rows = fk['pb_w_' + name], fk['pb_rows_%d' % len(fk['pb_w_' + name])]
    mesh = mx.DataOmegaMesh(w)
    assert np.array_equal(mesh.delta, fk['pb_delta_' + name])
    for ib, b in enumerate(fk['pb_b']):
        B = get_preblur(mesh, float(b))
        check_entries(B[rows], blur_truth(fk, name, ib), blur_bound(w, rows, float(b)), 'host get_preblur %s b=%g' % (name, b))


@pytest.mark.parametrize('name', ['hyp3', 'hyp255', 'hyp257'])
def test_longdouble_restatement_of_the_blur_matrix_against_the_truth(fk, name):
    """the truth tests/test_gpu_fill_truth.py forms for the blur product, on the meshes and widths it runs"""
    w, delta = fk['pb_w_' + name], fk['pb_delta_' + name]
    for ib in (1, 2):                                 # b = 0.05, 0.3
        check_blur_longdouble(fk, name, ib, blur_longdouble(w, delta, float(fk['pb_b'][ib])))
