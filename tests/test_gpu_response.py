"""The linear response on the device (mxe_response) against the extended-precision truth of ``response_ref``.

Gate of every comparison: max|X - X_t| <= 1e-6 max|X_t| per column (right-hand side).  Every test prints its worst figure."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from response_ref import GATE, LD, truth_response, weights, rhs_rows, worst_rel               # noqa: E402
from test_response_host import big_data_kernel, dlogD_directions, FD_STEP_MODEL, FD_MODEL_ERROR     # noqa: E402
import maxent_amd as mx                                                                         # noqa: E402
from maxent_amd import device, synthetic, posterior, hostprep, response                        # noqa: E402
from maxent_amd.minimizers import NewtonStepConvergenceMethod                                  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ('normal', 'plusminus')


def quiet(obj):
    obj.set_verbosity(mx.VerbosityFlags.Quiet)
    return obj


def check(label, X, Xt, gate=GATE):
    assert np.all(np.isfinite(X)), label
    worst = worst_rel(X, Xt)
    print('%s: %s values, worst max|X - X_t| / max|X_t| of a column %.2e' % (label, np.shape(X), worst))
    assert worst <= gate, (label, worst)
    return worst


class Small(object):
    """40 x 64, an error bar per tau point (n_s = 35: a ragged tile), two elements on one data set -- normal and plus-minus
    entropy --, 10 alphas solved on the device; the truth per (entropy, alpha) is computed once"""

    def __init__(self):
        self.tau, self.omega, K, self.G = synthetic.single_G(40, 64)
        K.reduce_singular_space(1e-14)
        self.K, self.Kk = K, np.array(K.K)
        self.n_s = len(K.S)
        self.D = synthetic.flat_D(self.omega)
        self.err = synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(40))
        self.alphas = np.array(synthetic.alpha_mesh(10)) * 40
        self.ctx = device.DeviceContext(K.U, K.S, K.V)
        ds = self.ctx.add_dataset(self.err)
        kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
        self.ctx.set_elements([ds] * 2, [self.G, self.G], np.tile(self.D, (2, 1)), kinds)
        v0 = np.stack([hostprep.initial_v(K.V, self.D, self.omega.delta, k) for k in kinds])
        sol = self.ctx.solve_chains(np.arange(2), self.alphas, v0)
        assert sol['converged'].all()
        self.H = np.array(sol['H'])                              # (2, 10, 64)
        self.F = rhs_rows(64, self.omega)
        self._truth = {}

    def w(self, e, ia):
        return weights(self.H[e, ia], self.D, KINDS[e])

    def truth(self, e, ia, eta=1.0):
        key = (e, ia, eta)
        if key not in self._truth:
            self._truth[key] = truth_response(self.Kk, self.err, self.w(e, ia), self.alphas[ia], eta=eta)
        return self._truth[key]


@pytest.fixture(scope='module')
def small():
    s = Small()
    yield s
    s.ctx.close()


def test_model_space_ragged_tile_and_a_short_block(small):
    s = small
    assert 32 < s.n_s < 48 and s.n_s % 16 != 0 and len(s.F) == 20
    for e in (0, 1):
        el = np.full(10, e)
        t = {}
        Xw = s.ctx.response(el, s.alphas, s.F, H=s.H[e], weighted=True, timing=t)
        Xu = s.ctx.response(el, s.alphas, s.F, H=s.H[e], weighted=False)
        assert Xw.shape == (10, 20, 64) and t['launches'] == 1 and t['ms'] > 0
        Xt = np.stack([np.dot(s.truth(e, ia)[0], s.F.T.astype(LD)).T for ia in range(10)])
        wt = np.stack([s.w(e, ia) for ia in range(10)]).astype(LD)
        check('model space, R f (%s)' % KINDS[e], Xw, Xt)
        check('model space, S f (%s)' % KINDS[e], Xu, Xt / wt[:, None, :])


def test_data_space_and_its_agreement_with_model_space(small):
    s = small
    units = np.eye(40)[[0, 1, 7, 15, 16, 22, 38, 39]]
    through = (s.Kk @ s.F[8:].T).T / s.err[None, :]             # Sigma^-1/2 K f of the 12 smooth and oscillating rows
    Fd = np.concatenate([units, through])
    for e in (0, 1):
        el = np.full(10, e)
        Xd = s.ctx.response(el, s.alphas, Fd, H=s.H[e], space='data')
        Xt = np.stack([np.dot(s.truth(e, ia)[1], Fd.T.astype(LD)).T for ia in range(10)])
        check('data space (%s)' % KINDS[e], Xd, Xt)
        Xm = s.ctx.response(el, s.alphas, s.F[8:], H=s.H[e])
        both = worst_rel(Xd[:, 8:], Xm)
        print('data space through K f against model space (%s): %.2e' % (KINDS[e], both))
        assert both <= 2 * GATE, both


def test_cross_checks_with_fit_diagnostics_and_posterior_var(small):
    s = small
    units = np.eye(64)
    for e in (0, 1):
        el = np.full(10, e)
        R = s.ctx.response(el, s.alphas, units, H=s.H[e])       # row j of X: column j of R
        Rjj = R[:, np.arange(64), np.arange(64)]
        diag = s.ctx.fit_diagnostics(el, s.alphas, H=s.H[e])
        var = s.ctx.posterior_var(el, s.alphas, H=s.H[e], want_diag=True)
        ng = diag['n_good']
        tr = Rjj.sum(axis=1)
        print('tr R against N_g (%s): worst %.2e relative' % (KINDS[e], float(np.max(np.abs(tr - ng) / ng))))
        assert np.all(np.abs(tr - ng) <= 1e-6 * ng + 1e-12)
        w = np.stack([s.w(e, ia) for ia in range(10)])
        share = 1.0 - s.alphas[:, None] * var['diag'] / w
        print('R_jj against 1 - alpha Gamma_jj / w_j (%s): worst %.2e' % (KINDS[e], float(np.max(np.abs(Rjj - share)))))
        assert np.all(np.abs(Rjj - share) <= 1e-6 * np.abs(share) + 1e-12)
        assert np.all(Rjj >= -1e-12) and np.all(Rjj <= 1 + 1e-12)


def test_plus_minus_entropy_with_covariances_of_differing_rank():
    """2 x 2 element-wise with a covariance per element (given as bins): the off-diagonal elements -- plus-minus entropy,
    w = sqrt(H^2 + 4 D^2) -- have 57 and 55 rows, in ONE call with ld = 60: entries behind a set's rows are ignored"""
    n_tau = 60
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, n_tau, 100)
    ew = quiet(mx.ElementwiseMaxEnt(use_hermiticity=False))
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    rng = np.random.RandomState(4)
    drop = {(0, 0): 0, (0, 1): 3, (1, 0): 5, (1, 1): 2}
    n_bins = 80
    bins = np.empty((n_bins, 2, 2, n_tau))
    for key, d in drop.items():
        Qm = np.linalg.qr(rng.randn(n_tau, n_tau))[0]
        sd = synthetic.SIGMA * np.sqrt(n_bins) * np.sqrt(1.0 + rng.rand(n_tau))
        sd[n_tau - d:] = 0.0
        bins[(slice(None),) + key] = Gmat[key][None, :] + (rng.randn(n_bins, n_tau) * sd) @ Qm.T
    ew.set_G_tau_bins(tau, bins)
    worker = ew.maxent_offdiagonal
    specs, Kks, errs = [], [], []
    for key in ((0, 1), (1, 0)):
        ew._load_element(worker, key, True)
        specs.append(worker.maxent_loop.make_spec())
        Kks.append(np.array(worker.K.K))
        errs.append(np.array(worker.err, dtype=float))
    assert [len(sp['G']) for sp in specs] == [57, 55] and all(sp['T'] is not None for sp in specs)
    w_mesh = np.asarray(omega)
    D = np.asarray(specs[0]['D'])
    H = np.stack([D * np.sin(1.3 * w_mesh), -0.5 * D * np.cos(0.7 * w_mesh) * np.exp(-w_mesh ** 2 / 20.0)])   # (signs: plus-minus)
    alphas = np.array([300.0, 3.0])
    F = rhs_rows(100, omega)[[1, 4, 8, 9, 12, 15, 19]]
    Fd = np.full((2, 9, 60), 1.0e3)                               # (junk behind the rows of each set)
    for n in range(2):
        rows = len(specs[n]['G'])
        Fd[n, :2, :rows] = np.eye(rows)[[0, rows - 1]]
        Fd[n, 2:, :rows] = (Kks[n] @ F.T).T / errs[n][None, :]
    ctx = posterior._stage(worker.K, specs, 0)
    try:
        Xm = ctx.response([0, 1], alphas, F, H=H)
        Xd = ctx.response([0, 1], alphas, Fd, H=H, space='data')
    finally:
        ctx.close()
    for n in range(2):
        rows = len(specs[n]['G'])
        R, Dm = truth_response(Kks[n], errs[n], weights(H[n], D, 'plusminus'), alphas[n])
        check('plus-minus, rotated set of %d rows, model space' % rows, Xm[n], np.dot(R, F.T.astype(LD)).T)
        check('plus-minus, rotated set of %d rows, data space, ld 60' % rows, Xd[n], np.dot(Dm, Fd[n, :, :rows].T.astype(LD)).T)


def test_128_row_build_with_17_right_hand_sides():
    label, K, err, H, _, w_mesh = big_data_kernel()
    assert len(K.S) > 64
    Kk = np.array(K.K)
    D = synthetic.flat_D(K.omega)
    ctx = device.DeviceContext(K.U, K.S, K.V)
    try:
        ds = ctx.add_dataset(err)
        ctx.set_elements([ds], [Kk @ H], D[np.newaxis, :], [device.ENTROPY_NORMAL])
        alphas = np.array([50.0, 0.5])
        F = rhs_rows(96, w_mesh)[:17]
        Fd = np.concatenate([np.eye(80)[[0, 41, 79]], (Kk @ F[3:].T).T / err[None, :]])
        assert len(F) == 17 and len(Fd) == 17
        Hs = np.tile(H, (2, 1))
        Xm = ctx.response([0, 0], alphas, F, H=Hs)
        Xu = ctx.response([0, 0], alphas, F, H=Hs, weighted=False)
        Xd = ctx.response([0, 0], alphas, Fd, H=Hs, space='data')
    finally:
        ctx.close()
    for ia in range(2):
        R, Dm = truth_response(Kk, err, H, alphas[ia])
        Xt = np.dot(R, F.T.astype(LD)).T
        check('%s, n_s = %d, alpha %g, R f' % (label, len(K.S), alphas[ia]), Xm[ia], Xt)
        check('%s, alpha %g, S f' % (label, alphas[ia]), Xu[ia], Xt / np.asarray(H, dtype=LD)[None, :])
        check('%s, alpha %g, data space' % (label, alphas[ia]), Xd[ia], np.dot(Dm, Fd.T.astype(LD)).T)


def test_chi2_factor(small):
    """Q = eta chi2 / 2 - alpha S with eta = 2.5: exactly the response of the problem at alpha / eta"""
    s = small
    pick = [2, 7]
    scaled = s.ctx.response([0, 0], s.alphas[pick], s.F, H=s.H[0][pick], chi2_factor=2.5)
    plain = s.ctx.response([0, 0], s.alphas[pick] / 2.5, s.F, H=s.H[0][pick])
    assert np.array_equal(scaled, plain)
    Xt = np.stack([np.dot(s.truth(0, ia, eta=2.5)[0], s.F.T.astype(LD)).T for ia in pick])
    check('chi2_factor 2.5', scaled, Xt)
    Fd = np.eye(40)[[3, 30]]
    Xd = s.ctx.response([0, 0], s.alphas[pick], Fd, H=s.H[0][pick], chi2_factor=2.5, space='data')
    check('chi2_factor 2.5, data space', Xd, np.stack([np.dot(s.truth(0, ia, eta=2.5)[1], Fd.T.astype(LD)).T for ia in pick]))


def test_bits_do_not_depend_on_batch_block_or_place(small):
    s = small
    for space, F in (('model', s.F), ('data', (s.Kk @ s.F.T).T / s.err[None, :])):
        el = np.array([0] * 10 + [1] * 10)
        al = np.concatenate([s.alphas, s.alphas])
        Hs = s.H.reshape(20, 64)
        batch = s.ctx.response(el, al, F, H=Hs, space=space)
        alone = s.ctx.response([1], al[13:14], F, H=Hs[13:14], space=space)
        assert np.array_equal(alone[0], batch[13]), space
        # in calls of a few problems each (the split over P)
        split = s.ctx.response(el, al, F, H=Hs, space=space, max_values=3 * 20 * 64, timing=(t := {}))
        assert t['launches'] == 7 and np.array_equal(split, batch), space
        # a column alone, and at another place among the 20 (another lane, another block of 16)
        one = s.ctx.response([0], s.alphas[4:5], F[[13]], H=s.H[0][4:5], space=space)
        assert np.array_equal(one[0, 0], batch[4, 13]), space
        perm = np.roll(np.arange(20), 7)
        moved = s.ctx.response([0], s.alphas[4:5], F[perm], H=s.H[0][4:5], space=space)
        assert np.array_equal(moved[0], batch[4][perm]), space


def test_nan_policy_and_argument_errors(small):
    s = small
    el = np.zeros(4, dtype=np.int32)
    al = np.ascontiguousarray(s.alphas[:4])
    H = np.ascontiguousarray(s.H[0][:4])
    good = s.ctx.response(el, al, s.F, H=H)
    Hn = H.copy()
    Hn[2, 17] = np.nan
    mixed = s.ctx.response(el, al, s.F, H=Hn)                     # (returns: MXE_OK)
    assert np.all(np.isnan(mixed[2])) and np.array_equal(mixed[[0, 1, 3]], good[[0, 1, 3]])
    mixed_d = s.ctx.response(el, al, np.eye(40)[:3], H=Hn, space='data')
    assert np.all(np.isnan(mixed_d[2])) and np.all(np.isfinite(mixed_d[[0, 1, 3]]))
    # the raw call on a context of its own, before any launch
    ctx = device.DeviceContext(s.K.U, s.K.S, s.K.V)
    try:
        ds = ctx.add_dataset(s.err)
        ctx.set_elements([ds], [s.G], s.D[np.newaxis, :], [device.ENTROPY_NORMAL])
        out = np.empty((4, 20, 64))

        def raw(P=4, Hrows=H, space=0, n_rhs=20, ld=64, F=None):
            F = np.ascontiguousarray(np.tile(s.F, (4, 1, 1))) if F is None else F
            return ctx._lib.mxe_response(ctx._h, P, device._p(el), device._p(al), None if Hrows is None else device._p(Hrows),
                                         None, 1.0, space, 1, n_rhs, ld, device._p(F), device._p(out), None)
        assert raw() == 0
        assert np.array_equal(out, good)
        assert raw(Hrows=None) == -4                               # MXE_ERR_STATE: nothing was launched
        assert raw(n_rhs=0) == -1 and raw(space=2) == -1 and raw(space=-1) == -1 and raw(P=0) == -1
        assert raw(ld=63) == -1                                    # model space: ld below n_omega
        Fd = np.zeros((4, 20, 64))
        assert raw(space=1, F=Fd, ld=64) == 0 and raw(space=1, F=Fd, ld=40) == 0
        assert raw(space=1, F=Fd, ld=39) == -1                     # data space: ld below the rows of the data set
        Fn = np.ascontiguousarray(np.tile(s.F, (4, 1, 1)))
        Fn[3, 19, 63] = np.inf
        assert raw(F=Fn) == -1
        assert raw(n_rhs=2 ** 23, ld=64) == -1                     # P n_rhs max(ld, n_omega) = 2^31 > 2^31 - 1 (checked before F is read)
        with pytest.raises(ValueError):
            ctx.response(el, al, Fn, H=H)
        with pytest.raises(ValueError):
            ctx.response(el, al, s.F[:, :63], H=H)
        with pytest.raises(ValueError):
            ctx.response(el, al, s.F, H=H, space='both')
        with pytest.raises(device.MaxEntDeviceError):
            ctx.response(el, al, s.F)
    finally:
        ctx.close()


def small_job(n_alpha=10, **kw):
    tau, omega, K, G = synthetic.single_G(40, 64)
    tm = quiet(mx.TauMaxEnt(**kw))
    tm.omega = omega
    tm.set_G_tau_data(tau, G)
    tm.set_error(synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(40)))
    tm.alpha_mesh = synthetic.alpha_mesh(n_alpha)
    return tm, tau, omega


def solved(tm):
    res = tm.run()
    assert np.all(res.converged)
    return res


def close_summaries(label, got, psf_t, w_mesh, delta, x0):
    """the summaries of the device's point-spread functions against those of the truth's columns.  The columns agree to
    1e-6 of their largest entry; the summaries are ratios of sums over the column whose denominators (the weight, sum p^2
    delta) are of the size of the numerators at the points taken, so 1e-4 (of the mesh's width for positions) bounds them
    100 x over"""
    ref = response.psf_summaries(w_mesh, delta, np.asarray(psf_t, dtype=float), x0)
    width = w_mesh.max() - w_mesh.min()
    for name in ('weight', 'spread', 'height'):
        np.testing.assert_allclose(got[name], ref[name], rtol=1e-4, err_msg='%s %s' % (label, name))
    for name in ('centroid', 'shift', 'fwhm'):
        np.testing.assert_allclose(got[name], ref[name], rtol=0, atol=1e-4 * width, equal_nan=True, err_msg='%s %s' % (label, name))
    assert np.array_equal(got['peak'], ref['peak']), label


def test_resolution_of_a_tau_maxent():
    tm, tau, omega = small_job()
    res = solved(tm)
    w_mesh, delta = np.asarray(omega), np.asarray(omega.delta)
    Kk, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H), np.asarray(res.alpha)
    test = np.stack([np.exp(-(w_mesh - 1.0) ** 2 / 0.02), np.where(np.abs(w_mesh + 1.5) < 0.5, 1.0, 0.0)])
    t = {}
    out = tm.resolution(res, omega0=[-1.52, 0.03, 1.0], alpha='all', test=test, timing=t)
    assert t['reused_contexts'] == 1 and t['ms'] > 0, t          # (the solver's context still holds this element staged)
    idx = out['index']
    assert idx.shape == (3,) and np.array_equal(out['omega0'], w_mesh[idx])
    assert np.array_equal(idx, [np.argmin(np.abs(w_mesh - x)) for x in (-1.52, 0.03, 1.0)])
    for name, shape in (('psf', (10, 3, 64)), ('averaging_kernel', (10, 3, 64)), ('image', (10, 2, 64)), ('weight', (10, 3)),
                        ('centroid', (10, 3)), ('shift', (10, 3)), ('spread', (10, 3)), ('peak', (10, 3)), ('fwhm', (10, 3)),
                        ('data_share', (10, 3)), ('alpha', (10,)), ('alpha_index', (10,))):
        assert np.shape(out[name]) == shape, (name, np.shape(out[name]))
    Rs = [truth_response(Kk, err, H[ia], alpha[ia])[0] for ia in range(10)]
    psf_t = np.stack([(R[:, idx] / delta[:, None].astype(LD)).T for R in Rs])
    avk_t = np.stack([R[idx, :] / delta[idx, None].astype(LD) for R in Rs])
    img_t = np.stack([(np.dot(R, (test * delta).T.astype(LD)) / delta[:, None].astype(LD)).T for R in Rs])
    check('resolution: psf', out['psf'], psf_t)
    check('resolution: averaging kernel', out['averaging_kernel'], avk_t)
    check('resolution: image', out['image'], img_t)
    share_t = np.stack([np.diag(R)[idx].astype(float) for R in Rs])
    assert np.all(np.abs(out['data_share'] - share_t) <= 1e-6 * share_t + 1e-12)
    close_summaries('resolution', out, psf_t, w_mesh, delta, w_mesh[idx])
    assert out['info']['nan_rows'] == []
    # alpha='all' equals the per-alpha calls, and the analyzer's alpha by default
    for ia in (0, 6):
        one = tm.resolution(res, omega0=[-1.52, 0.03, 1.0], alpha=ia, test=test)
        assert one['psf'].shape == (3, 64) and int(one['alpha_index']) == ia
        for name in ('psf', 'averaging_kernel', 'image', 'weight', 'spread', 'fwhm', 'data_share'):
            assert np.array_equal(one[name], out[name][ia], equal_nan=True), (name, ia)
    default = tm.resolution(res, omega0=1.0)
    ia = int(res.analyzer_results[res.default_analyzer_name]['alpha_index'])
    assert int(default['alpha_index']) == ia and np.array_equal(default['psf'][0], out['psf'][ia, 2])
    # every mesh point: tr R = N_g
    every = tm.resolution(res, alpha=3)
    assert every['psf'].shape == (64, 64)
    ng = tm.fit_diagnostics(res, alpha=3)['n_good']
    assert abs(every['data_share'].sum() - ng) <= 1e-6 * ng
    # the mesh points in chunks of 20 (four chunks, the last one short): one visit of the device, the same bits
    mp = pytest.MonkeyPatch()
    mp.setattr(response, 'CHUNK_VALUES', 20 * 64)
    try:
        t = {}
        chunked = tm.resolution(res, alpha=3, test=test, timing=t)
    finally:
        mp.undo()
    assert t['launches'] == 9 and t['reused_contexts'] == 1, t
    for name in ('psf', 'averaging_kernel', 'data_share', 'spread'):
        assert np.array_equal(chunked[name], every[name]), name
    with pytest.raises(ValueError, match='bryan'):
        tm.resolution(res, alpha='bryan')
    with pytest.raises(ValueError, match='finite'):
        tm.resolution(res, test=np.full((1, 64), np.nan))


def test_resolution_with_a_preblur_goes_through_the_data():
    tm, tau, omega = small_job(n_alpha=6)
    b = 0.1
    tm.A_of_H = mx.PreblurA_of_H(b=b, omega=tm.omega)
    tm.K = mx.PreblurKernel(K=tm.K, b=b)
    res = solved(tm)
    w_mesh, delta = np.asarray(omega), np.asarray(omega.delta)
    B = np.asarray(tm.A_of_H.matrix(), dtype=float)
    Kb, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H), np.asarray(res.alpha)
    notes = []
    tm.logtaker.error_message = lambda msg, *a, **k: notes.append(msg)
    test = np.exp(-(w_mesh - 1.0) ** 2 / 0.02)[None, :]
    out = tm.resolution(res, omega0=[-1.5, 1.0], alpha=[1, 4], test=test)
    assert out['averaging_kernel'] is None and len(notes) == 1 and 'averaging_kernel' in notes[0]
    assert out['psf'].shape == (2, 2, 64) and out['image'].shape == (2, 1, 64)
    idx = out['index']
    Kd = np.asarray(tm.K.K_delta, dtype=float)
    for n, ia in enumerate((1, 4)):
        _, Dm = truth_response(Kb, err, H[ia], alpha[ia])
        lift = np.dot(B.astype(LD), Dm)                          # dA = B Gamma eta K'^T Sigma^-1/2 dG~
        dG = (Kd[:, idx] / delta[idx][None, :]) / err[:, None]   # unit weight at omega_j: dA_t = e_j / delta_j
        check('preblur psf, alpha index %d' % ia, out['psf'][n], np.dot(lift, dG.astype(LD)).T)
        check('preblur image, alpha index %d' % ia, out['image'][n], np.dot(lift, ((Kd @ test.T) / err[:, None]).astype(LD)).T)
    assert np.all(np.isfinite(out['weight'])) and np.all(np.isfinite(out['spread']))


def test_elementwise_resolution_with_hermiticity():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 40, 64)
    ew = quiet(mx.ElementwiseMaxEnt(use_hermiticity=True))
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.set_error(synthetic.SIGMA)
    ew.alpha_mesh = synthetic.alpha_mesh(6)
    res = ew.run()
    assert np.all(res.converged)
    w_mesh, delta = np.asarray(omega), np.asarray(omega.delta)
    t = {}
    out = ew.resolution(res, omega0=[-1.5, 0.5], alpha=[1, 4], timing=t)
    print('element-wise resolution: timing', t)
    # two phases, each a weighted and an unweighted call.  run() of a plain ElementwiseMaxEnt puts both phases into ONE
    # launch (run_async), so the solver's context holds the three elements together; a phase asks for a context that
    # holds exactly its own (BatchSolver.staged_context_for: old['n'] != n), finds none and stages one: 0.  A
    # DiagonalMaxEnt has one phase and one launch: the context is taken (below).
    assert t['reused_contexts'] == 0 and t['launches'] == 4 and t['ms'] > 0, t
    assert out['psf'].shape == (2, 2, 2, 2, 64) and out['averaging_kernel'].shape == (2, 2, 2, 2, 64)
    assert out['fwhm'].shape == (2, 2, 2, 2) and out['index'].shape == (2,)
    for name in ('psf', 'averaging_kernel', 'weight', 'spread', 'data_share'):
        assert np.all(np.isfinite(out[name])), name
        assert np.array_equal(out[name][1, 0], out[name][0, 1]), name       # (the hermitian partner, unchanged)
    idx = out['index']
    for (i, j) in ((0, 0), (0, 1), (1, 1)):
        worker = ew.maxent_diagonal if i == j else ew.maxent_offdiagonal
        kind = 'normal' if i == j else 'plusminus'
        for n, ia in enumerate((1, 4)):
            Hn = np.asarray(res.H[i][j][ia])
            R, _ = truth_response(np.array(worker.K.K), synthetic.SIGMA, weights(Hn, worker.D.D, kind), float(res.alpha[ia]))
            check('element-wise psf (%d, %d), alpha index %d' % (i, j, ia), out['psf'][i, j, n], (R[:, idx] / delta[:, None].astype(LD)).T)
    d = dlogD_directions(w_mesh)
    dm = ew.default_model_response(res, d, alpha=[1, 4])
    assert dm['dA'].shape == (2, 2, 2, 2, 64) and np.array_equal(dm['dA'][1, 0], dm['dA'][0, 1])
    # one phase, one launch: the solver's context holds exactly the two diagonal elements and is taken; the same bits
    dg = quiet(mx.DiagonalMaxEnt())
    dg.set_G_tau_data(tau, Gmat)
    dg.omega = omega
    dg.set_error(synthetic.SIGMA)
    dg.alpha_mesh = synthetic.alpha_mesh(6)
    res_d = dg.run()
    t = {}
    out_d = dg.resolution(res_d, omega0=[-1.5, 0.5], alpha=[1, 4], timing=t)
    assert t['reused_contexts'] == 1 and t['launches'] == 2, t
    assert np.all(np.isnan(out_d['psf'][0, 1])) and np.all(np.isnan(out_d['psf'][1, 0]))
    for i in (0, 1):
        assert np.array_equal(np.asarray(res_d.H[i][i]), np.asarray(res.H[i][i]))
        assert np.array_equal(out_d['psf'][i, i], out['psf'][i, i]) and np.array_equal(out_d['fwhm'][i, i], out['fwhm'][i, i], equal_nan=True)


def test_elements_under_the_threshold_hold_nan():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 40, 64)
    Gmat = Gmat.copy()
    Gmat[0, 1] = Gmat[1, 0] = 0.0                                 # (below G_threshold: not computed)
    ew = quiet(mx.ElementwiseMaxEnt(use_hermiticity=True))
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.set_error(synthetic.SIGMA)
    ew.alpha_mesh = synthetic.alpha_mesh(4)
    res = ew.run()
    assert (0, 1) in [tuple(z)[:2] for z in res.zero_elements]
    out = ew.resolution(res, omega0=[0.5], alpha=2)
    dm = ew.default_model_response(res, dlogD_directions(np.asarray(omega)), alpha=2)
    assert out['psf'].shape == (2, 2, 1, 64) and dm['dA'].shape == (2, 2, 2, 64)
    for key in ((0, 1), (1, 0)):
        assert np.all(np.isnan(out['psf'][key])) and np.all(np.isnan(out['data_share'][key])) and np.all(np.isnan(dm['dA'][key]))
        assert out['alpha_index'][key] == -1
    for key in ((0, 0), (1, 1)):
        assert np.all(np.isfinite(out['psf'][key])) and np.all(np.isfinite(dm['dA'][key])) and out['alpha_index'][key] == 2


def dA_truth(Kk, err, H, D, kind, alpha, d, delta):
    R, _ = truth_response(Kk, err, weights(H, D, kind), alpha)
    f = (H[None, :] * d).astype(LD)
    return (f - np.dot(R, f.T).T) / delta[None, :].astype(LD)


@pytest.mark.parametrize('kind', KINDS)
def test_default_model_response_against_the_truth(kind):
    tm, tau, omega = small_job(cost_function=kind) if kind == 'plusminus' else small_job()
    res = solved(tm)
    w_mesh, delta = np.asarray(omega), np.asarray(omega.delta)
    d = dlogD_directions(w_mesh)
    out = tm.default_model_response(res, d, alpha='all')
    assert out['dA'].shape == (10, 2, 64) and out['dH'].shape == (10, 2, 64)
    Kk, err, H, alpha = np.array(tm.K.K), np.asarray(tm.err), np.asarray(res.H), np.asarray(res.alpha)
    Xt = np.stack([dA_truth(Kk, err, H[ia], np.asarray(tm.D.D), kind, alpha[ia], d, delta) for ia in range(10)])
    check('default-model response (%s)' % kind, out['dA'], Xt)
    one = tm.default_model_response(res, d)
    ia = int(res.analyzer_results[res.default_analyzer_name]['alpha_index'])
    assert one['dA'].shape == (2, 64) and np.array_equal(one['dA'], out['dA'][ia])
    with pytest.raises(ValueError, match='dlogD'):
        tm.default_model_response(res, d[:, :63])
    with pytest.raises(ValueError, match='bryan'):
        tm.default_model_response(res, d, alpha='bryan')


def test_default_model_response_with_poormans_off_diagonal_models():
    tau, omega, K, Gmat, _ = synthetic.matrix_G(2, 40, 64)
    pm = quiet(mx.PoormanMaxEnt(use_hermiticity=True))
    pm.set_G_tau_data(tau, Gmat)
    pm.omega = omega
    pm.set_error(synthetic.SIGMA)
    pm.alpha_mesh = synthetic.alpha_mesh(6)
    res = pm.run()
    assert np.all(res.converged)
    w_mesh, delta = np.asarray(omega), np.asarray(omega.delta)
    d = dlogD_directions(w_mesh)
    t = {}
    out = pm.default_model_response(res, d, alpha=[1, 4], timing=t)
    print('Poorman: timing', t)
    # (run_diagonal and run_offdiagonal are launches of their own, each on its worker's solver: both contexts are taken)
    assert t['reused_contexts'] == 2 and t['launches'] == 2, t
    assert out['dA'].shape == (2, 2, 2, 2, 64) and np.array_equal(out['dA'][1, 0], out['dA'][0, 1])
    D01 = np.asarray(pm._posterior_models(pm._offdiag_jobs(), res)[0].D, dtype=float)
    assert not np.allclose(D01, synthetic.flat_D(omega))
    Kk = np.array(pm.maxent_offdiagonal.K.K)
    for n, ia in enumerate((1, 4)):
        Hn = np.asarray(res.H[0][1][ia])
        check('Poorman (0, 1), alpha index %d' % ia, out['dA'][0, 1, n],
              dA_truth(Kk, synthetic.SIGMA, Hn, D01, 'plusminus', float(res.alpha[ia]), d, delta))


def test_default_model_response_against_two_runs_of_the_device():
    """dA against (A[D e^{+eps d}] - A[D e^{-eps d}]) / (2 eps) of two run() calls (Newton step below 1e-13, normal
    entropy) on the problem, the two alphas (alpha~ = 100 and 1) and at the step FD_STEP_MODEL = 1e-3 of the CPU test.
    Gate: 10 x the error the difference quotient of the truth showed there (FD_MODEL_ERROR['normal'] = 1.22e-9, so 1.22e-8
    of the largest entry): the device solve adds tol_h / eps = 1e-10 of noise on top of the truncation error."""
    eps = FD_STEP_MODEL

    def job(factor):
        tm, tau, omega = small_job()
        tm.scale_alpha = 1.0
        tm.alpha_mesh = mx.DataAlphaMesh([100.0, 1.0])           # (those of test_response_host: the gate was measured there)
        tm.minimizer = mx.LevenbergMinimizer(convergence=NewtonStepConvergenceMethod(1e-13, estimate=False))
        if factor is not None:
            tm.D = mx.DataDefaultModel(np.asarray(tm.D.D) / np.asarray(omega.delta) * factor, omega)
        return tm, omega
    tm, omega = job(None)
    res = solved(tm)
    assert sorted(np.asarray(res.alpha)) == [1.0, 100.0]
    d = dlogD_directions(np.asarray(omega))
    out = tm.default_model_response(res, d, alpha='all')
    worst = 0.0
    for n in range(2):
        Ap = np.asarray(solved(job(np.exp(eps * d[n]))[0]).A)
        Am = np.asarray(solved(job(np.exp(-eps * d[n]))[0]).A)
        fd = (Ap - Am) / (2.0 * eps)
        for ia in range(2):
            rel = worst_rel(out['dA'][ia, n][None, :], fd[ia][None, :])
            print('direction %d, alpha %g: %.2e' % (n, res.alpha[ia], rel))
            worst = max(worst, rel)
    print('default-model response against two device runs (step %.0e): worst %.2e of the largest entry (gate %.1e)'
          % (eps, worst, 10 * FD_MODEL_ERROR['normal']))
    assert worst <= 10 * FD_MODEL_ERROR['normal'], worst
