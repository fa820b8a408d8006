"""Bosonic continuation on the GPU: TauMaxEnt / ElementwiseMaxEnt on chi(tau) and chi(i nu_n), the device fills against
40-digit truth, the device decomposition of the new kernels and of a caller's matrix (mxe_kernel_svd_boson,
mxe_kernel_svd_boson_iw, mxe_kernel_svd_data), and chi(omega) from A(omega) (get_chi_w_from_A_w).

Gate as everywhere (test_gpu_api.py, test_gpu_iw.py): 1e-6 relative L2 against the extended-precision fixed point
(oracle/hp_truth.py) of the reference's own iterates (tests/golden/make_golden_boson.py).
"""
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GATE = 1e-6
EPS = 2.0 ** -52
SVD_MAX_SWEEPS = 40


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
def kk():
    return load('boson_kernels')


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


# the four single-scan problems that have a fixture: (file, suffix of its keys, kernel of boson_kernels.npz)
CASES = {'tau': ('boson_tau', '', 'K_tau_w200'), 'tau_sym': ('boson_tau', '_sym', 'K_tau_whalf'),
         'iw': ('boson_iw', '', 'K_nu_w200'), 'iw_sym': ('boson_iw', '_sym', 'K_nu_whalf')}


def case(name, kk):
    f, suf, kkey = CASES[name]
    g = load(f)
    if suf:
        c = {k[:-len(suf)]: v for k, v in g.items() if k.endswith(suf)}
        c.update(grid=g['grid'], beta=g['beta'])
    else:
        c = {k: v for k, v in g.items() if not k.endswith('_sym')}
    c['K'] = kk[kkey]
    c['name'] = name
    return c


def facade(c, svd_backend='host'):
    tm = mx.TauMaxEnt(svd_backend=svd_backend)
    tm.set_verbosity(mx.VerbosityFlags.Quiet)
    tm.omega = mx.DataOmegaMesh(c['omega'])
    sym = c['name'].endswith('_sym')
    if c['name'].startswith('tau'):
        tm.set_chi_tau_data(c['grid'], c['data'], beta=float(c['beta']), symmetric=sym)
    elif sym:
        tm.set_chi_iw_data(c['grid'], c['data'], symmetric=True)
    else:
        n = len(c['grid'])
        tm.set_chi_iw_data(c['grid'], c['data'][:n] + 1j * c['data'][n:])
    tm.set_error(float(c['err'][0]))
    tm.alpha_mesh = mx.DataAlphaMesh(c['alpha'] / len(c['err']))
    return tm


def truth_of(c):
    """chi2, S and Q of the fixture's extended-precision H, with the fixture's (40-digit) kernel"""
    p = R.Problem(c['K'], None, None, None, c['data'], c['err'], c['D'])
    chi2 = np.array([R.chi2_f(p, H) for H in c['H_truth']])
    S = np.array([R.S_f(p, H) for H in c['H_truth']])
    return chi2, S, 0.5 * chi2 - c['alpha'] * S


@pytest.mark.parametrize('name', sorted(CASES))
def test_single_scan_matches_the_reference_fixed_point(kk, name):
    c = case(name, kk)
    assert np.all(c['converged_ref']) and len(c['converged_ref']) == len(c['alpha']) == 30
    tm = facade(c)
    res = tm.run()
    # (the count of singular values above the absolute 1e-14: the reference decomposed the 40-digit matrix, this is the
    #  binary64 fill, and a value may lie within rounding of the cut -- the tau kernel's 50th is 1.02e-14)
    assert abs(len(tm.K.S) - len(c['S'])) <= 1
    assert np.all(res.converged)
    np.testing.assert_allclose(np.asarray(res.alpha), c['alpha'], rtol=1e-14)          # Ndata: 2 n for the stacked form
    eA, eH = rel_l2(np.asarray(res.A), c['A_truth']).max(), rel_l2(np.asarray(res.H), c['H_truth']).max()
    chi2, S, Q = truth_of(c)
    es = [np.max(np.abs(np.asarray(got) - want) / np.abs(want)) for got, want in ((res.chi2, chi2), (res.S, S), (res.Q, Q))]
    print('%s: A %.2e H %.2e chi2 %.2e S %.2e Q %.2e audit %.2e' % ((name, eA, eH) + tuple(es) + (tm.last_launch['audit_max'],)))
    assert eA < GATE and eH < GATE
    assert all(e < GATE for e in es)
    assert tm.last_launch['audit_max'] < GATE, tm.last_launch['audit_max']
    # the data-space fields in the form the data came in
    n = len(c['grid'])
    assert np.array_equal(res.data_variable, c['grid'])
    G_rec = np.asarray(res.G_rec)
    if name == 'iw':
        chi = c['data'][:n] + 1j * c['data'][n:]
        assert res.G.dtype == complex and np.array_equal(res.G, chi) and np.array_equal(res.G_orig, chi)
        assert G_rec.dtype == complex and G_rec.shape == (30, n)
        np.testing.assert_allclose(G_rec, np.asarray(res.A) @ (tm.K.K_complex * c['delta'][None, :]).T, rtol=0, atol=1e-13)
    else:
        assert np.asarray(res.G).dtype == float and np.array_equal(res.G, c['data']) and G_rec.dtype == float
        assert G_rec.shape == (30, n)
    assert res.analyzer_results['LineFitAnalyzer']['alpha_index'] == int(c['linefit_alpha_index'])
    import pickle
    back = pickle.loads(pickle.dumps(res.data))
    assert np.asarray(back.G).dtype == np.asarray(res.G).dtype and np.array_equal(back.G_rec, G_rec)


@pytest.mark.parametrize('name', sorted(CASES))
def test_maxent_loop_with_a_data_kernel_of_the_truth_equals_the_facade(kk, name):
    """the way a user had to do it before: MaxEntLoop + DataKernel of the (40-digit) matrix; the new classes change
    nothing but the fill"""
    c = case(name, kk)
    omega = mx.DataOmegaMesh(c['omega'])
    loop = mx.MaxEntLoop(alpha_mesh=mx.DataAlphaMesh(c['alpha'] / len(c['err'])))
    loop.set_verbosity(mx.VerbosityFlags.Quiet)
    grid = np.concatenate([c['grid'], c['grid']]) if name == 'iw' else c['grid']
    loop.K = mx.DataKernel(grid, omega, c['K'])
    loop.D = mx.FlatDefaultModel(omega)
    loop.G = c['data']
    loop.err = c['err']
    res = loop.run()
    ref = facade(c).run()
    assert np.all(res.converged) and np.all(ref.converged)
    e = rel_l2(np.asarray(res.H), np.asarray(ref.H)).max()
    print('%s: hand-built vs facade %.2e' % (name, e))
    assert e < GATE
    assert rel_l2(np.asarray(res.H), c['H_truth']).max() < GATE


def test_tau_and_matsubara_continuations_of_one_spectrum_agree(kk):
    """exact chi(tau) on 2 n points and exact chi(i nu_n) of one A: LineFit A_out within 1e-2 mean square of each
    other and of the input (the tolerance of test_iomega_and_tau_continuations_of_one_spectrum_agree)"""
    g = load('boson_iw')
    omega = mx.DataOmegaMesh(g['omega'])
    beta, nu = float(g['beta']), g['grid']
    A = g['A_true']
    tau = np.linspace(0, beta, 2 * len(nu))
    outs = []
    for kind in ('tau', 'iw'):
        tm = mx.TauMaxEnt()
        tm.set_verbosity(mx.VerbosityFlags.Quiet)
        tm.omega = omega
        if kind == 'tau':
            K = mx.BosonicTauKernel(tau, omega, beta=beta)
            tm.set_chi_tau_data(tau, np.array(K.K_delta) @ A, beta=beta)
        else:
            K = mx.BosonicIOmegaKernel(nu, omega)
            tm.set_chi_iw_data(nu, (K.K_complex * g['delta'][None, :]) @ A)
        tm.set_error(1e-4)
        tm.alpha_mesh = mx.LogAlphaMesh(1e-2, 1e4, 30)
        res = tm.run()
        assert np.all(res.converged) and tm.last_launch['audit_max'] < GATE
        outs.append(np.asarray(res.analyzer_results['LineFitAnalyzer']['A_out']))
    print('tau vs iw %.2e, iw vs input %.2e' % (np.mean((outs[0] - outs[1]) ** 2), np.mean((outs[1] - A) ** 2)))
    assert np.mean((outs[0] - outs[1]) ** 2) < 1e-2
    assert np.mean((outs[1] - A) ** 2) < 1e-2


def _ew(g, chi, herm=True):
    ew = mx.ElementwiseMaxEnt(use_hermiticity=herm)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.omega = mx.DataOmegaMesh(g['omega'])
    ew.alpha_mesh = mx.DataAlphaMesh(g['alpha_mesh'])
    ew.set_chi_tau_data(g['tau'], chi, beta=float(g['beta']))
    ew.set_error(float(g['err']))
    return ew


def test_elementwise_fixture_and_run_many_returns_the_same_bits():
    g = load('boson_elementwise')
    for herm in (True, False):
        ew = _ew(g, g['chi'], herm)
        res = ew.run()
        assert type(ew.maxent_diagonal.K) is mx.BosonicTauKernel and type(ew.maxent_offdiagonal.K) is mx.BosonicTauKernel
        assert np.array_equal(ew.maxent_diagonal.K.V, ew.maxent_offdiagonal.K.V)      # one decomposition for all elements
        assert all(info['audit_max'] < GATE for info in ew.last_launches) and ew.last_launches
        H = np.asarray(res.H)
        assert H.shape == g['H_truth'].shape
        for i in range(2):
            for j in range(2):
                e = rel_l2(H[i, j], g['H_truth'][i, j])
                print('element-wise herm=%s (%d, %d): %.2e' % (herm, i, j, e.max()))
                assert np.all(np.isfinite(e)) and e.max() < GATE, (herm, i, j, e.max())
        jobs = [_ew(g, g['chi'], herm), _ew(g, 0.5 * g['chi'], herm)]
        seq = [np.asarray(job.run().H).copy() for job in jobs]
        many = mx.run_many(jobs)
        for s, r in zip(seq, many):
            assert np.array_equal(np.asarray(r.H), s, equal_nan=True)
        assert np.array_equal(seq[0], H, equal_nan=True)


# ---- chi(omega) -----------------------------------------------------------------------------------------------
REL = 1e-12            # (the gate of test_gpu_kramers_kronig.py: relative to the sum of absolute terms)


def chi_np(A, w, w_out, bf=1.0):
    """chi = sum_j A_j (-w_j D_j) / (w_out - w_j + i bf D_j), D_j as in get_G_w_from_A_w; and the scale
    max_o sum_j |A_j c_oj|"""
    w = np.asarray(w, dtype=float)
    n = len(w)
    j = np.arange(n)
    D = (w[np.minimum(j + 1, n - 1)] - w[np.maximum(j - 1, 0)]) * 0.5
    C = (-w * D)[None, :] / (np.asarray(w_out)[:, None] - w[None, :] + 1j * bf * D[None, :])
    return np.asarray(A) @ C.T, (np.abs(A) @ np.abs(C).T).max(axis=-1), D


def test_get_chi_w_from_A_w_against_the_numpy_sum():
    g = load('boson_iw')
    w, A = g['omega'], g['A_true']
    chi = mx.get_chi_w_from_A_w(A, w, np_omega=801, w_min=-8, w_max=8)
    assert isinstance(chi, mx.ArrayGf) and chi.data.shape == (801, 1, 1)
    want, scale, _ = chi_np(A, w, chi.mesh)
    assert np.abs(chi.data[:, 0, 0] - want).max() <= REL * scale
    # Im chi(w) = pi w A(w) (to the broadening), odd; Re chi even
    assert np.abs(chi.data[:, 0, 0].imag + chi.data[::-1, 0, 0].imag).max() < 1e-3
    # a matrix-valued spectrum and the interpolation
    Am = np.stack([np.stack([A, 0.3 * A]), np.stack([0.3 * A, 2 * A])])
    chim = mx.get_chi_w_from_A_w(Am, w, np_interp_A=1500, np_omega=300, w_min=-5, w_max=5)
    wi = np.linspace(w.min(), w.max(), 1500)
    want, scale, _ = chi_np(np.stack([np.interp(wi, w, a) for a in Am.reshape(4, -1)]), wi, chim.mesh)
    assert np.all(np.abs(chim.data.transpose(1, 2, 0).reshape(4, -1) - want).max(axis=-1) <= REL * scale)
    # symmetric: the half-axis spectrum mirrored first; Re chi(0) = sum_j A_j D_j
    wh = g['omega_sym'][1:]                          # (no point at 0: the term w_j / (w_j - i eta) of it would be 0, not 1)
    Ah = g['A_true_sym'][1:]
    chis = mx.get_chi_w_from_A_w(Ah, wh, np_omega=3, w_min=-4, w_max=4, broadening_factor=1e-9, symmetric=True)
    wfull, Afull = np.concatenate([-wh[::-1], wh]), np.concatenate([Ah[::-1], Ah])
    want, scale, D = chi_np(Afull, wfull, chis.mesh, bf=1e-9)
    assert chis.mesh[1] == 0.0
    assert np.abs(chis.data[:, 0, 0] - want).max() <= REL * scale
    assert abs(chis.data[1, 0, 0].real - np.sum(Afull * D)) <= REL * scale
    assert abs(chis.data[1, 0, 0].imag) <= REL * scale


# ---- the device fills and decompositions ----------------------------------------------------------------------
def check_fill(got, truth, tau_abs_omega, what):
    """the bound of tests/test_boson_host.py: relative error <= (8 + tau |omega|) 2^-52 where the truth is above 1e-300,
    exact 0 where it is 0"""
    assert got.shape == truth.shape and np.all(np.isfinite(got))
    big = np.abs(truth) > 1e-300
    rel = np.abs(got[big] - truth[big]) / np.abs(truth[big])
    bound = ((8 + tau_abs_omega) * EPS * np.ones(truth.shape))[big]
    print('device fill %s: max rel %.2e (%.2f of the bound)' % (what, rel.max(), (rel / bound).max()))
    assert np.all(rel <= bound)
    assert np.all(got[truth == 0.0] == 0.0)


def _delta(w):
    return mx.DataOmegaMesh(w).delta


@pytest.mark.parametrize('name', ['w200', 'w201z', 'wmid', 'wwide', 'whalf'])
def test_device_tau_fill_against_the_truth(kk, name):
    w, tau = kk[name], kk['tau']
    r = device.kernel_svd_boson(tau, w, _delta(w), float(kk['beta']), symmetric=(name == 'whalf'), want_K=True)[0]
    check_fill(r['K'], kk['K_tau_' + name], tau[:, None] * np.abs(w)[None, :], 'tau ' + name)


@pytest.mark.parametrize('name', ['w200', 'w201z', 'wmid', 'whalf'])
def test_device_matsubara_fill_is_the_host_fill_bit_for_bit(kk, name):
    w, nu = kk[name], kk['nu']
    sym = name == 'whalf'
    r = device.kernel_svd_boson_iw(nu, w, _delta(w), symmetric=sym, want_K=True)[0]
    assert np.array_equal(r['K'], np.asarray(mx.BosonicIOmegaKernel(nu, mx.DataOmegaMesh(w), symmetric=sym).K))
    check_fill(r['K'], kk['K_nu_' + name], 0.0, 'nu ' + name)


def check_svd(r, Kh, what):
    """the assertions and constants of test_device_fill_and_svd_of_the_stacked_kernel, except the sweep count: the
    decomposition reports convergence (below SVD_MAX_SWEEPS)"""
    nrm = np.linalg.norm(Kh, 2)
    Sl = np.linalg.svd(Kh, compute_uv=False)
    U, S, V = r['U'], r['S'], r['V']
    k = int((Sl >= 1e-12 * Sl[0]).sum())
    lead = int((Sl >= 1e-4 * Sl[0]).sum())
    d_abs = np.max(np.abs(S[:k] - Sl[:k])) / Sl[0]
    d_rel = np.max(np.abs(S[:lead] - Sl[:lead]) / Sl[:lead])
    print('%s: n_s=%d (LAPACK %d above 1e-14) qr_rank=%d sweeps=%d %.3f ms; |dS|/S_0 %.1e, leading %d values relative %.1e'
          % (what, len(S), int((Sl >= 1e-14).sum()), r['qr_rank'], r['sweeps'], r['ms'], d_abs, lead, d_rel))
    assert 0 < r['sweeps'] < SVD_MAX_SWEEPS             # (info == 0: a call that ran out of sweeps raises MaxEntDeviceError)
    assert len(S) >= k and d_abs < 1e-12 and d_rel < 1e-12
    assert np.abs((U * S) @ V.T - Kh).max() < 1e-13 * nrm
    assert np.abs(U.T @ U - np.eye(len(S))).max() < 1e-12
    assert np.abs(V.T @ V - np.eye(len(S))).max() < 1e-12


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_svd_of_the_new_kernels_and_of_a_callers_matrix(kk, name):
    sym = name.endswith('_sym')
    w = kk['whalf'] if sym else kk['w200']
    omega = mx.DataOmegaMesh(w)
    bs = [0.0, 0.1]
    if name.startswith('tau'):
        K = mx.BosonicTauKernel(kk['tau'], omega, beta=float(kk['beta']), symmetric=sym)
        res = device.kernel_svd_boson(kk['tau'], w, omega.delta, float(kk['beta']), sym, bs, want_K=True)
        Kt = kk['K_tau_whalf' if sym else 'K_tau_w200']
    else:
        K = mx.BosonicIOmegaKernel(kk['nu'], omega, symmetric=sym)
        res = device.kernel_svd_boson_iw(kk['nu'], w, omega.delta, sym, bs, want_K=True)
        Kt = kk['K_nu_whalf' if sym else 'K_nu_w200']
    res_d = device.kernel_svd_data(Kt, w, omega.delta, bs, want_K=True)
    assert np.array_equal(res_d[0]['K'], Kt)                     # the transposition on the device moves bits
    for b, r, rd in zip(bs, res, res_d):
        Kh = np.array(K.K) if b <= 0 else np.array(mx.PreblurKernel(K=K, b=b).K)
        assert np.abs(r['K'] - Kh).max() <= (16 * EPS * np.abs(Kh).max() if b <= 0 else 1e-14 * np.linalg.norm(Kh, 2))
        check_svd(r, Kh, 'fill + SVD %s b=%g' % (name, b))
        Kd = Kt if b <= 0 else np.array(mx.PreblurKernel(K=mx.DataKernel(None, omega, Kt), b=b).K)
        assert np.abs(rd['K'] - Kd).max() <= 1e-14 * np.linalg.norm(Kd, 2)
        check_svd(rd, Kd, 'mxe_kernel_svd_data %s b=%g' % (name, b))


def test_the_data_entry_returns_the_bits_of_the_matsubara_entry():
    """mxe_kernel_svd_data fed the host-filled stacked matrix of the fermionic IOmegaKernel (that fill equals the device
    fill bit for bit): both entries decompose the same matrix with the same code"""
    g = load('iw_single')
    omega = mx.DataOmegaMesh(g['omega'])
    K = mx.IOmegaKernel(g['iomega'], omega)
    bs = [0.0, 0.1]
    a = device.kernel_svd_iw(g['iomega'], g['omega'], omega.delta, bs, want_K=True)
    b = device.kernel_svd_data(np.asarray(K.K), g['omega'], omega.delta, bs, want_K=True)
    for ra, rb in zip(a, b):
        for key in ('K', 'U', 'S', 'V'):
            assert np.array_equal(ra[key], rb[key]), key
        assert ra['sweeps'] == rb['sweeps'] and ra['qr_rank'] == rb['qr_rank']


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_backend_end_to_end(kk, name):
    c = case(name, kk)
    tm = facade(c, svd_backend='device')
    out = tm.run()
    assert tm.K.svd_backend == 'device' and np.all(out.converged)
    e = rel_l2(np.asarray(out.A), c['A_truth']).max()
    print('%s device backend: %.2e' % (name, e))
    assert e < GATE
    # the same through a DataKernel on the device, plain and inside a PreblurKernel
    omega = mx.DataOmegaMesh(c['omega'])
    Kd = mx.DataKernel(c['grid'], omega, c['K'], svd_backend='device')
    U, S, V = Kd.U, Kd.S, Kd.V
    assert np.abs((U * S) @ V.T - c['K']).max() < 1e-13 * np.linalg.norm(c['K'], 2)
    Kb = mx.PreblurKernel(K=Kd, b=0.1)
    assert Kb.svd_backend == 'device'
    assert np.abs((Kb.U * Kb.S) @ Kb.V.T - Kb.K).max() < 1e-13 * np.linalg.norm(Kb.K, 2)


def test_preblur_scan_of_the_bosonic_tau_kernel(kk):
    omega = mx.DataOmegaMesh(kk['w200'])
    K = mx.BosonicTauKernel(kk['tau'], omega, beta=float(kk['beta']), svd_backend='device')
    scan = mx.PreblurKernel.scan(K, [0.05, 0.1, 0.2])
    for Kb, b in zip(scan, [0.05, 0.1, 0.2]):
        assert Kb.b == b and Kb.S.min() >= 1e-14
        Kh = np.array(mx.PreblurKernel(K=mx.BosonicTauKernel(kk['tau'], omega, beta=float(kk['beta'])), b=b).K)
        assert np.abs((Kb.U * Kb.S) @ Kb.V.T - Kh).max() < 1e-12 * np.linalg.norm(Kh, 2)


def test_too_many_rows_point_to_the_host_backend(kk):
    w = kk['whalf']
    n_big = device.SVD_MAX_ROWS + 1
    with pytest.raises(device.MaxEntDeviceError, match='host'):
        device.kernel_svd_data(np.ones((n_big, len(w))), w, _delta(w))
    with pytest.raises(device.MaxEntDeviceError, match='host'):
        device.kernel_svd_boson_iw(2 * np.pi * np.arange(n_big // 2 + 1) / 40.0, w, _delta(w))
    with pytest.raises(device.MaxEntDeviceError):               # a symmetric kernel on a two-sided mesh: MXE_ERR_ARG
        device.kernel_svd_boson(kk['tau'], kk['w200'], _delta(kk['w200']), 40.0, symmetric=True)
