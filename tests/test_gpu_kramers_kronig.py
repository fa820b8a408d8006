"""The Kramers-Kronig transform on the GPU (mxe_kramers_kronig): get_G_w_from_A_w, kramers_kronig and the
self-energy workflow of SigmaContinuator.set_Gaux_w_from_Aaux_w.

The reference's transform needs TRIQS, so no fixture of it exists; the formula of maxent_util.py:91-130 is restated
here in numpy (``kk_np``) and pinned by the reference's own closed-form case (test/python/G_w_from_A_w.py).
Gate: max |G_dev - G_np| <= 1e-12 * max_o sum_j |A_j c_oj|, relative to the sum of absolute terms.

The sizes on both sides of every tile of kk_partial and of every decision of mxe_kramers_kronig are held to a
np.longdouble restatement instead, within (KK_SLICE + n_slice + 8) 2^-52 of the same scale: the fixed summation order
csrc/mxe_kk.hip.h documents, turned into a bound.
"""
import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device, synthetic

pytestmark = pytest.mark.gpu

REL = 1e-12


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def kk_np(A, w, w_out, bf=1.0):
    """the restatement: G = sum_j A_j D_j / (w_out - w_j + i bf D_j), D_j = (w[j+1] - w[j-1]) / 2 (one-sided at the
    ends); returns G (..., n_out) and the scale max_o sum_j |A_j c_oj| of every spectrum"""
    w = np.asarray(w, dtype=float)
    n = len(w)
    j = np.arange(n)
    D = (w[np.minimum(j + 1, n - 1)] - w[np.maximum(j - 1, 0)]) * 0.5
    C = D[None, :] / (np.asarray(w_out)[:, None] - w[None, :] + 1j * bf * D[None, :])     # (n_out, n_w)
    A = np.asarray(A)
    G = A @ C.T
    scale = (np.abs(A) @ np.abs(C).T).max(axis=-1)
    return G, scale


def check(G, A, w, w_out, bf=1.0):
    G_np, scale = kk_np(A, w, w_out, bf)
    err = np.abs(G - G_np).max(axis=-1)
    assert np.all(np.isfinite(G))
    assert np.all(err <= REL * scale + 1e-300), (err.max(), scale.min())


def grid(kind, n):
    if kind == 'linear':
        return np.linspace(-5.0, 5.0, n)
    if n == 1:
        return np.array([0.37])                # (a one-point hyperbolic mesh has no defined point)
    return np.asarray(mx.HyperbolicOmegaMesh(-5.0, 5.0, n))


@pytest.mark.parametrize('kind', ['linear', 'hyperbolic'])
@pytest.mark.parametrize('n_w', [1, 2, 3, 97, 1000])
def test_device_matches_the_restatement(kind, n_w):
    w = grid(kind, n_w)
    rng = np.random.RandomState(n_w)
    for n_out in (1, 5, 2001):
        w_out = np.linspace(-6.1, 5.3, n_out)           # (never on a point of w: n_w = 1 has Delta = 0)
        for bf in (1.0, 0.3):
            for n_spec in (1, 7, 300):
                A = rng.rand(n_spec, n_w) - 0.3
                G = mx.kramers_kronig(A, w, w_out, broadening_factor=bf)
                assert G.shape == (n_spec, n_out) and G.dtype == complex
                check(G, A, w, w_out, bf)
                Ac = A + 1j * (rng.rand(n_spec, n_w) - 0.5)
                Gc = mx.kramers_kronig(Ac, w, w_out, broadening_factor=bf)
                check(Gc, Ac, w, w_out, bf)
    if n_w == 1:
        assert np.all(G == 0)


# ---- the tile edges of kk_partial and the decisions of mxe_kramers_kronig ---------------------------------------------
EPS = 2.0 ** -52
KK_T, KK_SLICE, KK_CHUNK = 256, 256, 64          # csrc/mxe_kk.hip.h: output points of a tile, j values of a slice, of a chunk
# mxe_kramers_kronig: TS = 2 spectra per workgroup up to n_spec = 2, 8 up to 8, 16 beyond (17: a second tile of one
# spectrum); one workgroup per j slice ("split") where n_slice > 1 and the unsplit grid ceil(n_spec / TS) *
# ceil(n_out / KK_T) has fewer than KK_SPLIT_BELOW workgroups, else every workgroup adds the slices itself ("combine")
KK_TS_EDGES = (2, 8, 16)
KK_SPLIT_BELOW = 1024
KK_POOL = 17                                     # distinct spectra of a large batch (coprime to every TS)


def kk_edge_spectra(n_w, n_out):
    """seeded grids, weights and a pool of signed spectra for one (n_w, n_out), with the longdouble restatement
    G = sum_j A_j weight_j / (w_out - w_j + i eta_j) of the pool and its scale max_o sum_j |A_j c_oj|"""
    Lf = np.longdouble
    rng = np.random.RandomState(1000 * n_w + n_out)
    w = np.asarray(mx.HyperbolicOmegaMesh(-5.0, 5.0, n_w))
    weight, eta = 0.01 + 0.05 * rng.rand(n_w), 0.02 + 0.2 * rng.rand(n_w)
    w_out = np.linspace(-6.1, 5.3, n_out)
    pool = rng.rand(KK_POOL, n_w) - 0.3
    x = w_out.astype(Lf)[:, None] - w.astype(Lf)[None, :]
    den = x * x + (eta.astype(Lf) ** 2)[None, :]
    c_re = weight.astype(Lf)[None, :] * x / den
    c_im = -(weight.astype(Lf) * eta.astype(Lf))[None, :] / den
    G_re, G_im = pool.astype(Lf) @ c_re.T, pool.astype(Lf) @ c_im.T
    scale = (np.abs(pool) @ np.asarray(np.sqrt(c_re ** 2 + c_im ** 2), dtype=float).T).max(axis=-1)
    return w, weight, eta, w_out, pool, G_re, G_im, scale


def kk_edge_check(n_w, n_out, n_spec, case):
    """``n_spec`` spectra (row r is pool row r mod KK_POOL: the bits of a spectrum do not depend on its place) through
    device.kramers_kronig; every value within (KK_SLICE + n_slice + 8) EPS scale of the restatement: at most KK_SLICE
    fma in a row, n_slice partial sums added in order (the header's fixed summation order), 8 for c_oj itself"""
    w, weight, eta, w_out, pool, G_re, G_im, scale = case
    idx = np.arange(n_spec) % KK_POOL
    G = device.kramers_kronig(w, weight, eta, w_out, pool[idx])
    assert G.shape == (n_spec, n_out) and np.all(np.isfinite(G))
    n_slice = -(-n_w // KK_SLICE)
    gate = (KK_SLICE + n_slice + 8) * EPS * scale[idx]
    err = np.asarray(np.sqrt((G.real - G_re[idx]) ** 2 + (G.imag - G_im[idx]) ** 2), dtype=float).max(axis=-1)
    assert np.all(err <= gate), (n_w, n_out, n_spec, (err / gate).max())
    return float((err / gate).max())


@pytest.mark.parametrize('n_w', [KK_CHUNK - 1, KK_CHUNK, KK_CHUNK + 1, KK_SLICE - 1, KK_SLICE, KK_SLICE + 1,
                                 2 * KK_SLICE + 1])
def test_tile_edges_against_the_longdouble_restatement(n_w):
    """n_w on both sides of a chunk, of a slice (one slice / two: the split decision) and two slices plus one value;
    n_out on both sides of an output tile; n_spec on both sides of every tile size"""
    worst = 0.0
    for n_out in (KK_T - 1, KK_T, KK_T + 1):
        case = kk_edge_spectra(n_w, n_out)
        for n_spec in sorted({1} | {e + d for e in KK_TS_EDGES for d in (0, 1)}):
            worst = max(worst, kk_edge_check(n_w, n_out, n_spec, case))
    print('kramers_kronig tile edges n_w=%d: worst ratio to the bound %.3f' % (n_w, worst))


@pytest.mark.parametrize('n_out', [KK_T, KK_T + 1])
def test_split_and_combine_against_the_longdouble_restatement(n_out):
    """the largest batch that is still split over the j slices and the smallest that is not, with one output tile and
    with two, at the smallest n_w that has two slices.  (The other clause of that decision, a gigabyte of partial sums,
    is out of a quick test's reach.)"""
    n_w = KK_SLICE + 1
    tiles_out = -(-n_out // KK_T)
    n_last_split = ((KK_SPLIT_BELOW - 1) // tiles_out) * KK_TS_EDGES[-1]      # 16368 with one output tile, 8176 with two
    case = kk_edge_spectra(n_w, n_out)
    for n_spec in (n_last_split, n_last_split + 1):
        worst = kk_edge_check(n_w, n_out, n_spec, case)
        print('kramers_kronig n_w=%d n_out=%d n_spec=%d (%s): worst ratio to the bound %.3f'
              % (n_w, n_out, n_spec, 'split' if n_spec == n_last_split else 'combine', worst))


def test_leading_shapes_and_the_device_binding():
    w = np.asarray(mx.HyperbolicOmegaMesh(-8.0, 8.0, 200))
    w_out = np.linspace(-9, 9, 301)
    A = np.random.RandomState(5).rand(3, 4, 2, 200)
    G = mx.kramers_kronig(A, w, w_out)
    assert G.shape == (3, 4, 2, 301)
    check(G.reshape(-1, 301), A.reshape(-1, 200), w, w_out)
    # device.kramers_kronig takes weight and eta as given
    t = {}
    weight, eta = np.full(200, 0.05), np.full(200, 0.2)
    G2 = device.kramers_kronig(w, weight, eta, w_out, A[0, 0], timing=t)
    want = A[0, 0] @ (weight[None, :] / (w_out[:, None] - w[None, :] + 1j * eta[None, :])).T
    assert np.abs(G2 - want).max() < 1e-12 * np.abs(want).max()
    assert t['launches'] == 1 and t['ms'] > 0
    with pytest.raises(ValueError):
        device.kramers_kronig(w, weight, eta, w_out, np.ones((2, 199)))


def test_the_references_analytic_case():
    """test/python/G_w_from_A_w.py: G = 1/((w + 4i)(w + 3i)) on linspace(-20, 20, 700), A = -Im G / pi; G back within 1e-2"""
    n, wmin, wmax = 700, -20.0, 20.0
    w = np.linspace(wmin, wmax, n)
    g = 1.0 / ((w + 4j) * (w + 3j))
    A = -g.imag / np.pi
    rec = mx.get_G_w_from_A_w(A, w, np_omega=n, w_min=wmin, w_max=wmax)
    assert isinstance(rec, mx.ArrayGf) and rec.data.shape == (n, 1, 1) and np.array_equal(rec.mesh, w)
    assert np.abs(rec.data[:, 0, 0].real - g.real).max() < 1e-2
    assert np.abs(rec.data[:, 0, 0].imag - g.imag).max() < 1e-2
    check(rec.data[:, 0, 0], A, w, w)
    # the rotated 2 x 2 matrix case
    gd = np.zeros((n, 2, 2), dtype=complex)
    gd[:, 0, 0] = g
    gd[:, 1, 1] = 1.0 / ((w + 2j) * (w + 3j))
    th = np.pi / 3
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    g_rot = R @ gd @ R.conj().T
    A_rot = np.transpose((-1.0 / (2 * np.pi * 1j)) * (g_rot - np.conj(np.transpose(g_rot, (0, 2, 1)))), (1, 2, 0))
    rec = mx.get_G_w_from_A_w(A_rot, w, np_omega=n, w_min=wmin, w_max=wmax)
    assert rec.data.shape == (n, 2, 2) and rec.target_shape == (2, 2)
    assert np.abs(rec.data.real - g_rot.real).max() < 1e-2
    assert np.abs(rec.data.imag - g_rot.imag).max() < 1e-2
    # with interpolation onto 1.2 times the points (np.interp, as the reference)
    rec = mx.get_G_w_from_A_w(A_rot, w, np_interp_A=int(n * 1.2), np_omega=n, w_min=wmin, w_max=wmax)
    w_i = np.linspace(wmin, wmax, int(n * 1.2))
    A_i = np.stack([[np.interp(w_i, w, A_rot[i, j]) for j in range(2)] for i in range(2)])
    check(np.transpose(rec.data, (1, 2, 0)).reshape(4, n), A_i.reshape(4, -1), w_i, w)
    assert np.abs(rec.data - g_rot).max() < 1e-2


def test_bits_do_not_depend_on_batching():
    w = np.asarray(mx.HyperbolicOmegaMesh(-10.0, 10.0, 1000))
    w_out = np.linspace(-10, 10, 2001)
    A = np.random.RandomState(11).rand(300, 1000)
    G = mx.kramers_kronig(A, w, w_out)
    for k in (0, 1, 7, 150, 299):
        assert np.array_equal(mx.kramers_kronig(A[k], w, w_out), G[k]), k
    assert np.array_equal(mx.kramers_kronig(A[::-1], w, w_out)[::-1], G)
    wt = (w[np.minimum(np.arange(1000) + 1, 999)] - w[np.maximum(np.arange(1000) - 1, 0)]) * 0.5
    et = wt.copy()
    t = {}
    chunked = device.kramers_kronig(w, wt, et, w_out, A, max_spectra=7, timing=t)
    assert t['launches'] == 43
    assert np.array_equal(chunked, G)
    assert np.array_equal(mx.kramers_kronig(A, w, w_out), G)          # launch after launch
    # a small batch (one workgroup per j slice) and a large one (each workgroup adds the slices itself)
    big = np.random.RandomState(12).rand(4000, 1000)
    big[123] = A[5]
    assert np.array_equal(mx.kramers_kronig(big, w, w_out)[123], G[5])


def _semicircle_iw(iomega, D=1.0):
    z = 1j * iomega
    r = np.sqrt(z * z - D * D)
    r = np.where((r / z).real < 0, -r, r)
    return 2.0 / (z + r)


def test_blocks_in_one_launch_equal_per_block_calls(monkeypatch):
    iom = (2 * np.arange(64) + 1) * np.pi / 20.0
    G = _semicircle_iw(iom)
    S = {'up': (iom, 1j * iom + 0.5 - 1 / G), 'dn': (iom, 1j * iom + 0.5 - 1 / G), 'm': (iom, 1j * iom - 1 / G)}
    sc = mx.InversionSigmaContinuator(S, {'up': 0.5, 'dn': 0.5, 'm': 0.0})
    w = np.asarray(mx.HyperbolicOmegaMesh(-6.0, 6.0, 301))
    rng = np.random.RandomState(3)
    A = {'up': rng.rand(301), 'dn': rng.rand(301), 'm': rng.rand(301) + 0.1j * rng.rand(301)}
    kw = dict(np_interp_A=800, np_omega=1001, w_min=-3, w_max=3)
    calls = []
    real_kk = device.kramers_kronig
    monkeypatch.setattr(device, 'kramers_kronig', lambda *a, **k: calls.append(a[4].shape) or real_kk(*a, **k))
    sc.set_Gaux_w_from_Aaux_w(A, w, **kw)
    assert calls == [(4, 800)]                  # one launch: up, dn, and both rows of the complex block
    monkeypatch.undo()
    for name in A:
        one = mx.get_G_w_from_A_w(A[name], w, **kw)
        assert np.array_equal(sc.Gaux_w[name].data, one.data), name
        assert np.array_equal(sc.Gaux_w[name].mesh, np.linspace(-3, 3, 1001))
        want = (one.mesh + sc._constant_shift[name]) - 1.0 / one.data[:, 0, 0]
        np.testing.assert_allclose(sc.S_w[name].data[:, 0, 0], want, rtol=1e-14, atol=0)


def test_sigma_continuation_end_to_end():
    """Sigma(i w_n) from a two-Gaussian A_aux through the inversion form, with seeded noise; then the guide's steps:
    InversionSigmaContinuator -> TauMaxEnt.set_G_iw_data -> run() -> set_Gaux_w_from_Aaux_w(LineFit A_out)"""
    beta, n_iw, C = 40.0, 40, 1.7
    iom = (2 * np.arange(n_iw) + 1) * np.pi / beta
    omega = mx.HyperbolicOmegaMesh(-10.0, 10.0, 200)
    A_true = synthetic.two_gaussian_spectrum(omega)
    K = mx.IOmegaKernel(iom, omega)
    Gaux = (K.K_complex * omega.delta[None, :]) @ A_true
    rng = np.random.RandomState(77)
    Gaux_noisy = Gaux + 1e-4 * (rng.randn(n_iw) + 1j * rng.randn(n_iw))
    S_iw = mx.ArrayGf(iom, 1j * iom + C - 1.0 / Gaux_noisy)

    isc = mx.InversionSigmaContinuator(S_iw, C)
    assert np.abs(isc.Gaux_iw.data[:, 0, 0] - Gaux_noisy).max() < 1e-12
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = omega
    tm.set_G_iw_data(isc.Gaux_iw.mesh, isc.Gaux_iw.data[:, 0, 0])
    tm.set_error(1e-4)
    tm.alpha_mesh = mx.LogAlphaMesh(1e-2, 1e4, 30)
    res = tm.run()
    assert np.all(res.converged)
    assert tm.last_launch['audit_max'] < 1e-6, tm.last_launch['audit_max']
    A_out = np.asarray(res.analyzer_results['LineFitAnalyzer']['A_out'])
    assert np.mean((A_out - A_true) ** 2) < 1e-2

    w = np.asarray(omega)
    kw = dict(np_interp_A=4000, np_omega=2000, w_min=-5.0, w_max=5.0)
    isc.set_Gaux_w_from_Aaux_w(A_out, w, **kw)
    assert isinstance(isc.Gaux_w, mx.ArrayGf) and isc.Gaux_w.data.shape == (2000, 1, 1)
    assert np.all(np.isfinite(isc.S_w.data))
    w_i = np.linspace(w.min(), w.max(), 4000)
    check(isc.Gaux_w.data[:, 0, 0], np.interp(w_i, w, A_out), w_i, np.linspace(-5.0, 5.0, 2000))
    # Sigma(w) is causal where the spectrum lives, and S_w inverts G_aux(w)
    want = (isc.Gaux_w.mesh + C) - 1.0 / isc.Gaux_w.data[:, 0, 0]
    np.testing.assert_allclose(isc.S_w.data[:, 0, 0], want, rtol=1e-14, atol=0)
    assert np.all(isc.S_w.data[:, 0, 0].imag < 1e-8)
