#!/usr/bin/env python3
"""Generate tests/golden/iw_single.npz, the Matsubara-axis fixture, from the REAL reference.

Like make_golden.py (whose ``import_reference`` it uses) it runs only where the reference is.  It
  1. fills the reference's IOmegaKernel (complex K(i w_n, w) = 1 / (i w_n - w)) on beta = 40,
     50 positive fermionic frequencies and HyperbolicOmegaMesh(-10, 10, 200),
  2. makes G(i w_n) of the two-Gaussian spectrum of maxent_amd.synthetic with seeded noise 1e-4 on
     the real and on the imaginary part,
  3. runs the reference's MaxEntLoop on the stacked real problem, DataKernel(iomega stacked, omega,
     [Re K ; Im K]) with G = [Re G ; Im G] (for a real A, chi2 over the complex data is the chi2 of
     that real system), MaxEntCostFunction and LevenbergMinimizer(MaxDerivativeConvergenceMethod(1e-7),
     maxiter=5000) over LogAlphaMesh(1e-2, 1e4, 30),
  4. checks that oracle/ref_numpy.py reproduces that run (iteration counts; H, A, chi2, S, Q to 1e-12),
  5. polishes every alpha's H in extended precision (oracle/hp_truth.py).

Usage:  python tests/golden/make_golden_iw.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, record_v        # noqa: E402  (also puts the repository root on sys.path)
from oracle import ref_numpy as R, hp_truth                # noqa: E402
from maxent_amd import synthetic                           # noqa: E402

BETA, N_IW, N_OMEGA, N_ALPHA, SIGMA = 40.0, 50, 200, 30, 1.e-4


def main():
    if 'triqs_maxent' not in sys.modules:
        import_reference()
    import triqs_maxent as ref
    from triqs_maxent.minimizers.convergence_methods import MaxDerivativeConvergenceMethod

    iomega = (2 * np.arange(N_IW) + 1) * np.pi / BETA
    omega = ref.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=N_OMEGA)
    Kc = np.array(ref.IOmegaKernel(iomega, omega, beta=BETA).K)            # the reference's complex kernel
    A = synthetic.two_gaussian_spectrum(np.array(omega))
    rng = np.random.RandomState(4321)
    G_iw = np.dot(Kc * omega.delta[np.newaxis, :], A) + SIGMA * (rng.randn(N_IW) + 1j * rng.randn(N_IW))

    K_r = np.concatenate([Kc.real, Kc.imag])
    G_r = np.concatenate([G_iw.real, G_iw.imag])
    err = SIGMA * np.ones(2 * N_IW)
    loop = ref.MaxEntLoop(cost_function=ref.MaxEntCostFunction(),
                          minimizer=ref.LevenbergMinimizer(MaxDerivativeConvergenceMethod(1e-7), maxiter=5000),
                          alpha_mesh=ref.LogAlphaMesh(alpha_min=1e-2, alpha_max=1e4, n_points=N_ALPHA))
    loop.set_verbosity(ref.VerbosityFlags.Quiet)
    loop.K = ref.DataKernel(np.concatenate([iomega, iomega]), omega, K_r)
    loop.D = ref.FlatDefaultModel(omega)
    loop.G = G_r
    loop.err = err
    vs, its, conv = record_v(loop)
    res = loop.run()

    U, S, V = loop.K.U, loop.K.S, loop.K.V
    p = R.Problem(K_r, U, S, V, G_r, err, np.array(loop.D.D))
    opts = R.LevenbergOptions(maxiter=5000, max_derivative=1e-7, rel_function_change=None)
    out = R.alpha_loop(p, omega.delta, np.array(loop.alpha_mesh), opts=opts)
    assert list(out['n_iter']) == list(its), 'oracle port: iteration counts differ'
    for k in ('H', 'A', 'chi2', 'S', 'Q', 'alpha'):
        assert np.allclose(np.asarray(getattr(res, k)), out[k], rtol=1e-12, atol=0), 'oracle port differs in ' + k
    alphas = np.array(res.alpha)
    H_truth = np.empty((N_ALPHA, N_OMEGA))
    for ia in range(N_ALPHA):
        info = {}
        _, H_truth[ia] = hp_truth.polish(K_r, G_r, err, p.D, V, S, alphas[ia], vs[ia], 'normal', iters=6, info=info)
        assert info['converged'], ('polish', ia, info)
    e = np.linalg.norm(np.array(res.H) - H_truth, axis=1) / np.linalg.norm(H_truth, axis=1)
    print('iw_single  n_s=%d iters=%d  ref-vs-truth max %.2e' % (len(S), sum(its), e.max()))
    np.savez_compressed(os.path.join(HERE, 'iw_single.npz'),
                        iomega=iomega, beta=BETA, omega=np.array(omega), delta=omega.delta,
                        K_ref=Kc, A_true=A, G_iw=G_iw, err=err, D=np.array(loop.D.D), alpha=alphas,
                        S=np.array(S), H_ref=np.array(res.H), A_ref=np.array(res.A),
                        chi2_ref=np.array(res.chi2), S_ref=np.array(res.S), Q_ref=np.array(res.Q),
                        n_iter_ref=np.array(its), converged_ref=np.array(conv), v_ref=np.array(vs),
                        H_truth=H_truth, A_truth=H_truth / omega.delta[np.newaxis, :],
                        linefit_alpha_index=res.analyzer_results['LineFitAnalyzer']['alpha_index'],
                        A_out_linefit=res.analyzer_results['LineFitAnalyzer']['A_out'])


if __name__ == '__main__':
    main()
