#!/usr/bin/env python3
"""Generate the bosonic fixtures boson_kernels.npz, boson_tau.npz, boson_iw.npz and boson_elementwise.npz.

Like make_golden_iw.py (and make_golden.py, whose ``import_reference`` it uses) it runs only where the reference
is.  Conventions: A(w) = Im chi(w) / (pi w); K(tau, w) = w e^{-tau w} / (1 - e^{-beta w}), 1/beta at
w = 0; K(i nu_n, w) = w / (w - i nu_n), 1 at w = nu_n = 0, stacked [Re K ; Im K]; symmetric forms K(., w) + K(., -w)
on w >= 0 (the Matsubara one real, n rows).

  1. boson_kernels.npz -- all four kernels evaluated with mpmath at 40 digits from the binary64 grid values and
     rounded to binary64, for beta = 40, tau = linspace(0, beta, 100), nu_n = 2 pi n / beta (n = 0..49) on
       w200   HyperbolicOmegaMesh(-10, 10, 200)
       w201z  HyperbolicOmegaMesh(-10, 10, 201) with its middle point (-1.8e-15) set to exactly 0
       wmid   that middle point itself, and its mirror image (two columns)
       whalf  the points w >= 0 of w201z (the symmetric forms)
       wwide  -20, -19.5, ..., 20: beta w up to +-800, where e^{-beta |w|} is below the smallest binary64 number
     (tau only: the Matsubara kernel has no exponentials).
  2. boson_tau.npz, boson_iw.npz -- the REFERENCE's MaxEntLoop on DataKernel(grid, omega, K_truth) with
     MaxEntCostFunction, LevenbergMinimizer(MaxDerivativeConvergenceMethod(1e-7), maxiter=5000),
     LogAlphaMesh(1e-2, 1e4, 30), flat default model, data K_truth delta A + seeded noise 1e-4, A = two Gaussians at
     +-1.5 (width 0.5) plus one at 0 (width 0.3), normalised.  Keys without suffix: the two-sided problem on w200;
     keys ending in ``_sym``: the symmetric form on whalf, with the first noise seed of ``SYM_SEEDS`` at which the
     reference converged at every alpha (``seed_sym``); boson_tau.npz has them only if such a seed exists.  Then, as in make_golden_iw.py, the run is reproduced by
     oracle/ref_numpy.py (iteration counts; H, A, chi2, S, Q to 1e-12) and every alpha's H is polished in extended
     precision (oracle/hp_truth.py).  The kernels are the entries of boson_kernels.npz and are not stored again.
  3. boson_elementwise.npz -- a 2 x 2 chi(tau) matrix (diagonal spectra rotated by a fixed orthogonal matrix as in
     maxent_amd.synthetic.matrix_G, symmetrised noise 1e-4), 8 alphas, normal entropy on the diagonal and plus-minus
     off it.  Through the PINNED PORT (oracle/ref_numpy.py, the port steps 2 check against the reference), not the
     reference's element-wise class: that class drives TauMaxEnt workers whose setters assign ``tau`` to the kernel,
     which the reference's DataKernel does not take.

The generator asserts that the reference (or the port) converged at EVERY alpha and that every polish converged.

Usage:  python tests/golden/make_golden_boson.py [--reuse-kernels]
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, record_v        # noqa: E402  (also puts the repository root on sys.path)
from oracle import ref_numpy as R, hp_truth                # noqa: E402

BETA, N_TAU, N_NU, N_ALPHA, SIGMA = 40.0, 100, 50, 30, 1.e-4
# noise seeds tried in turn for the symmetric problems: the first at which the reference converges at every alpha is the
# fixture (on the half-axis mesh its Levenberg iteration runs into maxiter = 5000 at one or two alphas for some noise
# realisations -- seeds 4322 (tau) and 8766 (Matsubara) among them; which seed is taken depends on the reference alone)
SYM_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


# ---- 1. the kernels in 40 digits ------------------------------------------------------------------------------
def k_tau(t, w, b, mp):
    if w == 0:
        return 1 / b
    return w * mp.exp(-t * w) / (1 - mp.exp(-b * w))


def k_nu(nu, w, mp):
    if w == 0 and nu == 0:
        return mp.mpc(1)
    return w / mp.mpc(w, -nu)


def truth_tau(tau, w, symmetric=False):
    import mpmath as mp
    mp.mp.dps = 40
    b = mp.mpf(BETA)
    out = np.empty((len(tau), len(w)))
    for i, t in enumerate(tau):
        t = mp.mpf(float(t))
        for j, x in enumerate(w):
            x = mp.mpf(float(x))
            out[i, j] = float(k_tau(t, x, b, mp) + (k_tau(t, -x, b, mp) if symmetric else 0))
    return out


def truth_nu(nu, w, symmetric=False):
    """stacked [Re K ; Im K] (2 n rows), or the real symmetric form (n rows)"""
    import mpmath as mp
    mp.mp.dps = 40
    re, im = np.empty((len(nu), len(w))), np.empty((len(nu), len(w)))
    for i, n_ in enumerate(nu):
        n_ = mp.mpf(float(n_))
        for j, x in enumerate(w):
            x = mp.mpf(float(x))
            z = k_nu(n_, x, mp) + (k_nu(n_, -x, mp) if symmetric else 0)
            re[i, j], im[i, j] = float(z.real), float(z.imag)
    if symmetric:
        assert not im.any()
        return re
    return np.concatenate([re, im])


def kernels_case(ref):
    tau = np.linspace(0, BETA, N_TAU)
    nu = 2 * np.pi * np.arange(N_NU) / BETA
    w200 = np.array(ref.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=200))
    w201 = np.array(ref.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=201))
    mid = w201[100]
    assert 0 < abs(mid) < 1e-14
    w201z = w201.copy()
    w201z[100] = 0.0
    wmid = np.array([-abs(mid), abs(mid)])
    whalf = w201z[100:].copy()
    wwide = np.arange(-20.0, 20.25, 0.5)
    out = dict(beta=BETA, tau=tau, nu=nu, w200=w200, w201z=w201z, wmid=wmid, whalf=whalf, wwide=wwide)
    for name, w in (('w200', w200), ('w201z', w201z), ('wmid', wmid), ('wwide', wwide)):
        out['K_tau_' + name] = truth_tau(tau, w)
        if name != 'wwide':
            out['K_nu_' + name] = truth_nu(nu, w)
    out['K_tau_whalf'] = truth_tau(tau, whalf, symmetric=True)
    out['K_nu_whalf'] = truth_nu(nu, whalf, symmetric=True)
    np.savez_compressed(os.path.join(HERE, 'boson_kernels.npz'), **out)
    print('boson_kernels: %d bytes' % os.path.getsize(os.path.join(HERE, 'boson_kernels.npz')))
    return out


# ---- 2. the reference on the true kernels ------------------------------------------------------------------------
def spectrum(w):
    """two Gaussians at +-1.5 (width 0.5) plus one at 0 (width 0.3); the integral over the WHOLE axis is 1"""
    w = np.asarray(w)
    A = np.exp(-(w - 1.5) ** 2 / (2 * 0.5 ** 2)) + np.exp(-(w + 1.5) ** 2 / (2 * 0.5 ** 2)) + \
        np.exp(-w ** 2 / (2 * 0.3 ** 2))
    fine = np.linspace(-12, 12, 48001)
    Af = np.exp(-(fine - 1.5) ** 2 / (2 * 0.5 ** 2)) + np.exp(-(fine + 1.5) ** 2 / (2 * 0.5 ** 2)) + \
        np.exp(-fine ** 2 / (2 * 0.3 ** 2))
    return A / np.trapezoid(Af, fine)


def reference_run(ref, grid, w, K, seed):
    """the reference's MaxEntLoop on DataKernel(grid, omega, K); returns the fixture's entries"""
    from triqs_maxent.minimizers.convergence_methods import MaxDerivativeConvergenceMethod
    omega = ref.DataOmegaMesh(w)
    A = spectrum(w)
    rng = np.random.RandomState(seed)
    G = np.dot(K * omega.delta[np.newaxis, :], A) + SIGMA * rng.randn(K.shape[0])
    err = SIGMA * np.ones(K.shape[0])
    loop = ref.MaxEntLoop(cost_function=ref.MaxEntCostFunction(),
                          minimizer=ref.LevenbergMinimizer(MaxDerivativeConvergenceMethod(1e-7), maxiter=5000),
                          alpha_mesh=ref.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e4, n_points=N_ALPHA))
    loop.set_verbosity(ref.VerbosityFlags.Quiet)
    loop.K = ref.DataKernel(grid, omega, K)
    loop.D = ref.FlatDefaultModel(omega)
    loop.G = G
    loop.err = err
    vs, its, conv = record_v(loop)
    res = loop.run()
    if not (all(conv) and len(conv) == N_ALPHA):
        print('   seed %d: the reference did not converge at alpha indices %s' % (seed, [i for i, c in enumerate(conv) if not c]))
        return None

    U, S, V = loop.K.U, loop.K.S, loop.K.V
    p = R.Problem(K, U, S, V, G, err, np.array(loop.D.D))
    opts = R.LevenbergOptions(maxiter=5000, max_derivative=1e-7, rel_function_change=None)
    out = R.alpha_loop(p, omega.delta, np.array(loop.alpha_mesh), opts=opts)
    assert list(out['n_iter']) == list(its), 'oracle port: iteration counts differ'
    for k in ('H', 'A', 'chi2', 'S', 'Q', 'alpha'):
        assert np.allclose(np.asarray(getattr(res, k)), out[k], rtol=1e-12, atol=0), 'oracle port differs in ' + k
    alphas = np.array(res.alpha)
    H_truth = np.empty((N_ALPHA, len(w)))
    for ia in range(N_ALPHA):
        info = {}
        _, H_truth[ia] = hp_truth.polish(K, G, err, p.D, V, S, alphas[ia], vs[ia], 'normal', iters=6, info=info)
        assert info['converged'], ('polish', ia, info)
    e = np.linalg.norm(np.array(res.H) - H_truth, axis=1) / np.linalg.norm(H_truth, axis=1)
    lf = res.analyzer_results['LineFitAnalyzer']
    print('   n_s=%d iters=%d..%d chi2_min=%.1f  ref-vs-truth max %.2e  LineFit A_out vs input %.3f'
          % (len(S), min(its), max(its), np.min(res.chi2), e.max(),
             np.linalg.norm(lf['A_out'] - A) / np.linalg.norm(A)))
    return dict(omega=w, delta=omega.delta, A_true=A, data=G, err=err, D=np.array(loop.D.D), alpha=alphas,
                S=np.array(S), H_ref=np.array(res.H), chi2_ref=np.array(res.chi2), S_ref=np.array(res.S),
                Q_ref=np.array(res.Q), n_iter_ref=np.array(its), converged_ref=np.array(conv),
                H_truth=H_truth, A_truth=H_truth / omega.delta[np.newaxis, :],
                linefit_alpha_index=lf['alpha_index'], A_out_linefit=lf['A_out'])


def single_cases(ref, kk):
    for name, grid_key, plain_key, seed in (('boson_tau', 'tau', 'K_tau_', 4321), ('boson_iw', 'nu', 'K_nu_', 8765)):
        grid = kk[grid_key]
        out = dict(beta=BETA, grid=grid)
        print(name)
        plain = reference_run(ref, grid if name == 'boson_tau' else np.concatenate([grid, grid]), kk['w200'],
                              kk[plain_key + 'w200'], seed)
        assert plain is not None, 'the reference did not converge at every alpha'
        out.update(plain)
        for sym_seed in SYM_SEEDS:
            sym = reference_run(ref, grid, kk['whalf'], kk[plain_key + 'whalf'], sym_seed)
            if sym is not None:
                out.update({k + '_sym': v for k, v in sym.items()})
                out['seed_sym'] = sym_seed
                break
        if name == 'boson_iw':
            assert sym is not None, 'no seed of SYM_SEEDS at which the reference converged at every alpha'
            # the complex form of the stacked data, as a user hands it to set_chi_iw_data
            n = len(grid)
            out['chi_iw'] = out['data'][:n] + 1j * out['data'][n:]
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
        print('   %d bytes' % os.path.getsize(os.path.join(HERE, name + '.npz')))


# ---- 3. the element-wise problem through the pinned port --------------------------------------------------------
def elementwise_case(kk):
    tau, w, K = kk['tau'], kk['w200'], kk['K_tau_w200']
    delta = R.omega_delta(w)
    n_orb, n_alpha = 2, 8
    mu, s = np.array([-1.5, 1.5]), np.array([0.4, 0.7])
    A_diag = np.exp(-(w[None, :] - mu[:, None]) ** 2 / (2 * s[:, None] ** 2))
    A_diag /= np.trapezoid(A_diag, w, axis=1)[:, None]
    Rm, _ = np.linalg.qr(np.random.RandomState(2024).randn(n_orb, n_orb))
    A_mat = np.einsum('ik,kw,jk->ijw', Rm, A_diag, Rm)
    noise = SIGMA * np.random.RandomState(2025).randn(n_orb, n_orb, len(tau))
    chi = np.einsum('tw,ijw->ijt', K * delta[None, :], A_mat) + 0.5 * (noise + noise.transpose(1, 0, 2))
    U, S, V = R.svd_reduce(K, 1e-14)
    D = R.flat_default_model(w)
    err = SIGMA * np.ones(len(tau))
    mesh = R.log_alpha_mesh(1e-1, 1e3, n_alpha)
    H_ref = np.empty((n_orb, n_orb, n_alpha, len(w)))
    H_truth = np.empty_like(H_ref)
    for i in range(n_orb):
        for j in range(n_orb):
            ent = 'normal' if i == j else 'plusminus'
            p = R.Problem(K, U, S, V, chi[i, j], err, D, entropy=ent)
            out = R.alpha_loop(p, delta, mesh)
            assert np.all(out['converged']), ('the port did not converge at every alpha', i, j)
            H_ref[i, j] = out['H']
            for ia in range(n_alpha):
                info = {}
                _, H_truth[i, j, ia] = hp_truth.polish(K, chi[i, j], err, D, V, S, out['alpha'][ia], out['v'][ia],
                                                       ent, iters=6, info=info)
                assert info['converged'], ('polish', i, j, ia, info)
    e = np.linalg.norm(H_ref - H_truth, axis=-1) / np.linalg.norm(H_truth, axis=-1)
    print('boson_elementwise: port-vs-truth max %.2e' % e.max())
    np.savez_compressed(os.path.join(HERE, 'boson_elementwise.npz'), beta=BETA, tau=tau, omega=w, delta=delta,
                        chi=chi, A_mat=A_mat, err=SIGMA, D=D, alpha_mesh=np.array(mesh), H_ref=H_ref, H_truth=H_truth)


def main():
    if 'triqs_maxent' not in sys.modules:
        import_reference()
    import triqs_maxent as ref
    if '--reuse-kernels' in sys.argv:             # (the 40-digit evaluation takes minutes)
        with np.load(os.path.join(HERE, 'boson_kernels.npz')) as d:
            kk = {k: d[k] for k in d.files}
    else:
        kk = kernels_case(ref)
    single_cases(ref, kk)
    elementwise_case(kk)


if __name__ == '__main__':
    main()
