"""Matsubara-axis continuation on the GPU: TauMaxEnt / ElementwiseMaxEnt on G(i omega_n), the device fill and
decomposition of the stacked IOmegaKernel (mxe_kernel_svd_iw), and mxe_kernel_svd unchanged by the shared code.

Gate as everywhere (test_gpu_api.py): 1e-6 relative L2 against the extended-precision fixed point (oracle/hp_truth.py)
of the reference's own iterates (tests/golden/make_golden_iw.py).
"""
import hashlib
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device, synthetic
from oracle import ref_numpy as R, hp_truth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GATE = 1e-6


@pytest.fixture(autouse=True, scope='module')
def _audit_every_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv('MAXENT_AMD_AUDIT', '1')
    yield
    mp.undo()


def load(name):
    with np.load(os.path.join(GOLD, name + '.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def g():
    return load('iw_single')


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def iw_tm(g, svd_backend='host'):
    tm = mx.TauMaxEnt(svd_backend=svd_backend)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.DataOmegaMesh(g['omega'])
    tm.set_G_iw_data(g['iomega'], g['G_iw'])
    tm.set_error(float(g['err'][0]))
    tm.alpha_mesh = mx.DataAlphaMesh(g['alpha'] / len(g['err']))
    return tm


def truth_of(g):
    """chi2, S and Q of the fixture's extended-precision H"""
    K = mx.IOmegaKernel(g['iomega'], mx.DataOmegaMesh(g['omega']))
    G_r = np.concatenate([g['G_iw'].real, g['G_iw'].imag])
    p = R.Problem(np.array(K.K), None, None, None, G_r, g['err'], g['D'])
    chi2 = np.array([R.chi2_f(p, H) for H in g['H_truth']])
    S = np.array([R.S_f(p, H) for H in g['H_truth']])
    return chi2, S, 0.5 * chi2 - g['alpha'] * S


def test_single_scan_matches_the_reference_fixed_point(g):
    tm = iw_tm(g)
    res = tm.run()
    n = len(g['iomega'])
    assert isinstance(tm.K, mx.IOmegaKernel) and len(tm.K.S) == len(g['S'])
    assert np.all(res.converged)
    np.testing.assert_allclose(np.asarray(res.alpha), g['alpha'], rtol=1e-14)      # Ndata = 2 n_iw
    assert rel_l2(np.asarray(res.A), g['A_truth']).max() < GATE
    assert rel_l2(np.asarray(res.H), g['H_truth']).max() < GATE
    chi2, S, Q = truth_of(g)
    for got, want in ((res.chi2, chi2), (res.S, S), (res.Q, Q)):
        assert np.max(np.abs(np.asarray(got) - want) / np.abs(want)) < GATE
    assert tm.last_launch['audit_max'] < GATE, tm.last_launch['audit_max']
    # the data-space fields, complex of n_iw values
    assert np.array_equal(res.data_variable, g['iomega'])
    assert res.G.dtype == complex and res.G.shape == (n,) and np.array_equal(res.G, g['G_iw'])
    assert res.G_orig.dtype == complex and np.array_equal(res.G_orig, g['G_iw'])
    G_rec = np.asarray(res.G_rec)
    assert G_rec.dtype == complex and G_rec.shape == (len(g['alpha']), n)
    Kd = tm.K.K_complex * g['delta'][None, :]
    np.testing.assert_allclose(G_rec, np.asarray(res.A) @ Kd.T, rtol=0, atol=1e-13)
    # the analyzers as for tau data; the reference's LineFit picks the same alpha
    assert res.analyzer_results['LineFitAnalyzer']['alpha_index'] == int(g['linefit_alpha_index'])
    # pickle and the plain-data form keep the complex dtypes
    import pickle
    back = pickle.loads(pickle.dumps(res.data))
    assert np.asarray(back.G).dtype == complex and np.array_equal(back.G, res.G)
    assert np.asarray(back.G_rec).dtype == complex and np.array_equal(back.G_rec, G_rec)
    d = mx.MaxEntResultData.__factory_from_dict__('MaxEntResultData', res.data.__reduce_to_dict__())
    assert np.asarray(d.G_orig).dtype == complex and np.array_equal(d.G_orig, g['G_iw'])


def test_maxent_loop_with_a_user_built_kernel_equals_the_facade(g):
    """the reference's own composition style: MaxEntLoop + IOmegaKernel + the stacked data"""
    omega = mx.DataOmegaMesh(g['omega'])
    loop = mx.MaxEntLoop(alpha_mesh=mx.DataAlphaMesh(g['alpha'] / len(g['err'])))
    loop.set_verbosity(mx.VerbosityFlags.Quiet)
    K = mx.IOmegaKernel(g['iomega'], omega)
    loop.K = K
    loop.D = mx.FlatDefaultModel(omega)
    loop.G = K.unfold(g['G_iw'])
    loop.err = g['err']
    res = loop.run()
    ref = iw_tm(g).run()
    assert np.array_equal(np.asarray(res.H), np.asarray(ref.H))
    assert res.G.dtype == complex and np.array_equal(res.G, g['G_iw'])


def test_iomega_and_tau_continuations_of_one_spectrum_agree(g):
    """exact G(tau) on 2 n_iw points and exact G(i omega_n) of one A: LineFit A_out within 1e-2 mean square
    (the reference's own tolerance, test/python/complex_A.py)"""
    omega = mx.DataOmegaMesh(g['omega'])
    beta, n = float(g['beta']), len(g['iomega'])
    A = g['A_true']
    tau = np.linspace(0, beta, 2 * n)
    outs = []
    for kind in ('tau', 'iw'):
        tm = mx.TauMaxEnt()
        tm.set_verbosity(mx.VerbosityFlags.Quiet)
        tm.omega = omega
        if kind == 'tau':
            K = mx.TauKernel(tau, omega, beta=beta)
            tm.set_G_tau_data(tau, np.array(K.K_delta) @ A)
        else:
            K = mx.IOmegaKernel(g['iomega'], omega)
            tm.set_G_iw_data(g['iomega'], (K.K_complex * g['delta'][None, :]) @ A)
        tm.set_error(1e-4)
        tm.alpha_mesh = mx.LogAlphaMesh(1e-2, 1e4, 30)
        res = tm.run()
        assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE
        outs.append(np.asarray(res.analyzer_results['LineFitAnalyzer']['A_out']))
    assert np.mean((outs[0] - outs[1]) ** 2) < 1e-2
    assert np.mean((outs[1] - A) ** 2) < 1e-2


def _matrix_iw(n_orb=4, n_iw=30, n_omega=100, beta=40.0):
    """a rotated matrix spectrum built like synthetic.matrix_G, exact G_ij(i omega_n)"""
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=n_omega)
    w = np.asarray(omega)
    mu, s = np.linspace(-1.5, 1.5, n_orb), np.linspace(0.4, 0.7, n_orb)
    A_diag = np.exp(-(w[None, :] - mu[:, None]) ** 2 / (2 * s[:, None] ** 2))
    A_diag /= np.trapezoid(A_diag, w, axis=1)[:, None]
    Rm, _ = np.linalg.qr(np.random.RandomState(2024).randn(n_orb, n_orb))
    A_mat = np.einsum('ik,kw,jk->ijw', Rm, A_diag, Rm)
    iomega = (2 * np.arange(n_iw) + 1) * np.pi / beta
    K = mx.IOmegaKernel(iomega, omega)
    G_iw = np.einsum('nw,ijw->ijn', K.K_complex * omega.delta[None, :], A_mat)
    return iomega, omega, K, G_iw


def _ew(iomega, omega, G_iw, herm):
    ew = mx.ElementwiseMaxEnt(use_hermiticity=herm)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = omega
    ew.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e3, n_points=8)
    ew.set_G_iw_data(iomega, G_iw)
    ew.set_error(1e-4)
    return ew


def test_elementwise_matches_the_oracle_and_run_many_returns_the_same_bits():
    iomega, omega, K, G_iw = _matrix_iw()
    n_orb = G_iw.shape[0]
    K.reduce_singular_space(1e-14)
    Kr, U, S, V = np.array(K.K), K.U, K.S, K.V
    D = mx.FlatDefaultModel(omega).D
    err = 1e-4 * np.ones(2 * len(iomega))
    alphas = np.array(mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e3, n_points=8))
    truth = {}
    for i in range(n_orb):
        for j in range(i, n_orb):
            G_r = K.unfold(0.5 * (G_iw[i, j] + G_iw[j, i]))
            ent = 'normal' if i == j else 'plusminus'
            p = R.Problem(Kr, U, S, V, G_r, err, D, entropy=ent)
            out = R.alpha_loop(p, omega.delta, alphas)
            Ht = np.empty_like(out['H'])
            for ia in range(len(alphas)):
                info = {}
                _, Ht[ia] = hp_truth.polish(Kr, G_r, err, D, V, S, out['alpha'][ia], out['v'][ia], ent, iters=6, info=info)
                assert info['converged'], (i, j, ia)
            truth[i, j] = truth[j, i] = Ht
    for herm in (True, False):
        ew = _ew(iomega, omega, G_iw, herm)
        res = ew.run()
        assert isinstance(ew.maxent_diagonal.K, mx.IOmegaKernel) and isinstance(ew.maxent_offdiagonal.K, mx.IOmegaKernel)
        assert np.array_equal(ew.maxent_diagonal.K.V, ew.maxent_offdiagonal.K.V)      # one decomposition for all elements
        assert all(info['audit_max'] < GATE for info in ew.last_launches) and ew.last_launches
        H = np.asarray(res.H)
        assert H.shape == (n_orb, n_orb, len(alphas), len(omega))
        for (i, j), Ht in truth.items():
            e = rel_l2(H[i, j], Ht)
            assert np.all(np.isfinite(e)) and e.max() < GATE, (herm, i, j, e.max())
        G = np.asarray(res.G)
        assert G.dtype == complex and G.shape == (n_orb, n_orb, len(iomega))
        np.testing.assert_allclose(G[0, 1], 0.5 * (G_iw[0, 1] + G_iw[1, 0]), rtol=0, atol=1e-16)
        # two objects in flight together: every field what run() returns, bit for bit
        jobs = [_ew(iomega, omega, G_iw, herm), _ew(iomega, omega, 0.5 * G_iw, herm)]
        seq = [np.asarray(job.run().H).copy() for job in jobs]
        many = mx.run_many(jobs)
        for s, r in zip(seq, many):
            assert np.array_equal(np.asarray(r.H), s, equal_nan=True)
        assert np.array_equal(seq[0], H, equal_nan=True)


def test_device_fill_and_svd_of_the_stacked_kernel(g):
    omega = mx.DataOmegaMesh(g['omega'])
    K = mx.IOmegaKernel(g['iomega'], omega)
    bs = [0.0, 0.1]
    res = device.kernel_svd_iw(g['iomega'], g['omega'], omega.delta, bs, want_K=True)
    for b, r in zip(bs, res):
        Kh = np.array(K.K) if b <= 0 else np.array(mx.PreblurKernel(K=K, b=b).K)
        nrm = np.linalg.norm(Kh, 2)
        # (the fill: the host's arithmetic, to the last ulp)
        assert np.abs(r['K'] - Kh).max() <= (4e-16 * np.abs(Kh).max() if b <= 0 else 1e-14 * nrm)
        Sl = np.linalg.svd(Kh, compute_uv=False)
        U, S, V = r['U'], r['S'], r['V']
        # (LAPACK's own singular values are good to ~eps S_0 absolute: the small ones are compared on that scale, the
        #  leading ones value by value)
        k = int((Sl >= 1e-12 * Sl[0]).sum())
        lead = int((Sl >= 1e-4 * Sl[0]).sum())
        d_abs = np.max(np.abs(S[:k] - Sl[:k])) / Sl[0]
        d_rel = np.max(np.abs(S[:lead] - Sl[:lead]) / Sl[:lead])
        print('mxe_kernel_svd_iw b=%g: n_s=%d (LAPACK %d) qr_rank=%d sweeps=%d %.3f ms; |dS|/S_0 %.1e, leading %d '
              'values relative %.1e' % (b, len(S), int((Sl >= 1e-14).sum()), r['qr_rank'], r['sweeps'], r['ms'],
                                        d_abs, lead, d_rel))
        assert r['sweeps'] < 20
        assert len(S) >= k and d_abs < 1e-12 and d_rel < 1e-12
        assert np.abs((U * S) @ V.T - Kh).max() < 1e-13 * nrm
        assert np.abs(U.T @ U - np.eye(len(S))).max() < 1e-12
        assert np.abs(V.T @ V - np.eye(len(S))).max() < 1e-12
    # the facade with the device decomposition meets the gate
    tm = iw_tm(g, svd_backend='device')
    out = tm.run()
    assert tm.K.svd_backend == 'device' and np.all(out.converged)
    assert rel_l2(np.asarray(out.A), g['A_truth']).max() < GATE
    # more rows than the decomposition's LDS holds: a clear error (the host backend takes them)
    n_big = device.SVD_MAX_ROWS // 2 + 1
    with pytest.raises(device.MaxEntDeviceError, match='host'):
        device.kernel_svd_iw(np.arange(n_big) + 0.5, g['omega'], omega.delta)


def test_tau_device_svd_is_bitwise_what_it_was():
    """mxe_kernel_svd after its body became the code it shares with mxe_kernel_svd_iw: U, S, V on the cfg2 grid, bit for
    bit the ones the library before that change computed (their sha256, tests/golden/kernel_svd_bits.npz)"""
    bits = load('kernel_svd_bits')
    tau, omega = synthetic.grids(200, 500)
    bs = list(bits['preblur_b'])
    res = device.kernel_svd(tau, np.asarray(omega), omega.delta, synthetic.BETA, bs)
    for ib, r in enumerate(res):
        for name in ('U', 'S', 'V'):
            h = hashlib.sha256(np.ascontiguousarray(r[name]).tobytes()).hexdigest()
            assert h == str(bits[name][ib]), (bs[ib], name)
        assert r['sweeps'] == int(bits['sweeps'][ib])


def test_many_directions():
    """beta = 100, 1000 Matsubara frequencies: n_s above 64 (directions_to_keep / the one-chain kernel), audited"""
    beta, n_iw = 100.0, 1000
    omega = mx.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=500)
    iomega = (2 * np.arange(n_iw) + 1) * np.pi / beta
    A = synthetic.two_gaussian_spectrum(omega)
    K = mx.IOmegaKernel(iomega, omega)
    tm = mx.TauMaxEnt()
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = omega
    tm.set_G_iw_data(iomega, (K.K_complex * omega.delta[None, :]) @ A)
    tm.set_error(1e-4)
    tm.alpha_mesh = mx.LogAlphaMesh(alpha_min=1e-1, alpha_max=1e3, n_points=6)
    res = tm.run()
    assert len(tm.K.S) > 64
    assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE, tm.last_launch['audit_max']
    assert np.mean((np.asarray(res.analyzer_results['LineFitAnalyzer']['A_out']) - A) ** 2) < 1e-2
