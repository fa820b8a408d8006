#!/usr/bin/env python3
"""Generate the Legendre fixtures legendre_kernels.npz, legendre.npz, legendre_elementwise.npz and legendre_bins.npz.

Like make_golden_boson.py (whose ``reference_run`` and ``spectrum`` it uses) it runs only where the reference is.
Conventions: TRIQS's GfLegendre normalisation, G(tau) = sum_l sqrt(2l+1)/beta P_l(2 tau/beta - 1) G_l,

    K(l, w) = -beta sqrt(2l+1) (-sgn w)^l i_l(beta |w| / 2) / (2 cosh(beta w / 2)),

i_l(a) = sqrt(pi / (2a)) I_{l+1/2}(a) the modified spherical Bessel function of the first kind; at w = 0 the row l = 0 is
-beta/2 and every other row 0.

  1. legendre_kernels.npz -- K evaluated with mpmath at 40 digits from the binary64 grid values and rounded to binary64,
     beta = 40:
       w200      l = 0..29   HyperbolicOmegaMesh(-10, 10, 200)
       w201z     l = 0..29   HyperbolicOmegaMesh(-10, 10, 201) with its middle point (-1.8e-15) set to exactly 0
       wmid      l = 0..29   that middle point itself, and its mirror image (two columns)
       wwide     l = 0..79   -20, -19.5, ..., 20: a = beta |w| / 2 up to 400, so a >> l, a ~ l and a << l all occur
       wsmall    l = 0..79   +-1e-6, +-3e-3
       even      l = 0, 2, ..., 28 (stored in that order) on w200
       shuffled  a fixed permutation of l = 0..9 on w200
       l0        l = [0] alone on w201z
     Keys: ``w_<name>``, ``l_<name>``, ``K_<name>``.
  2. legendre.npz -- the REFERENCE's MaxEntLoop on DataKernel(l, omega, K_w200) with the settings of the bosonic
     fixture (make_golden_boson.reference_run: MaxEntCostFunction, LevenbergMinimizer(MaxDerivativeConvergenceMethod(1e-7),
     maxiter=5000), LogAlphaMesh(1e-2, 1e4, 30), flat default model, its three-Gaussian A, data K delta A + seeded noise
     1e-4), reproduced by oracle/ref_numpy.py and polished by oracle/hp_truth.py there.  The noise seed is the first of
     ``SEEDS`` at which the reference converges at every alpha (``seed``).
  3. legendre_elementwise.npz -- a 2 x 2 matrix of Legendre coefficients (l = 0..29 on w200; diagonal spectra rotated by
     a fixed orthogonal matrix, symmetrised noise 1e-4), 8 alphas, normal entropy on the diagonal and plus-minus off it,
     through the PINNED PORT (oracle/ref_numpy.py), as boson_elementwise.npz.
  4. legendre_bins.npz -- seeded Gaussian noise around K delta A: ``s_bins`` 24 bins x 30 coefficients of the spectrum of
     2. (amplitude 1e-3 per bin), ``e_bins`` 12 bins x 2 x 2 x 12 coefficients (l = 0..11) of the matrix of 3.

The generator asserts that the reference (or the port) converged at EVERY alpha and that every polish converged.

Usage:  python tests/golden/make_golden_legendre.py [--reuse-kernels]
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference                  # noqa: E402,F401  (also puts the repository root on sys.path)
from make_golden_boson import reference_run, spectrum, SIGMA           # noqa: E402
from oracle import ref_numpy as R, hp_truth                # noqa: E402

BETA = 40.0
# noise seeds tried in turn: the first at which the reference converges at every alpha is the fixture.  With 30 data
# values the reference's Levenberg iteration runs into maxiter = 5000 at the smallest alphas (indices 24-29) for most
# noise realisations: 4321 (the bosonic fixture's seed) fails at index 29, and of the seeds 1..38 only 11 and 35
# converge everywhere; which seed is taken depends on the reference alone
SEEDS = (4321, 11, 35)
SHUFFLED = np.array([7, 2, 9, 0, 5, 3, 8, 1, 6, 4])
BIN_SIGMA = 1.e-3


# ---- 1. the kernel in 40 digits --------------------------------------------------------------------------------
def truth(l, w):
    import mpmath as mp
    mp.mp.dps = 40
    b = mp.mpf(BETA)
    half = mp.mpf(1) / 2
    out = np.empty((len(l), len(w)))
    for j, x in enumerate(w):
        x = mp.mpf(float(x))
        a = b * abs(x) / 2
        for i, k in enumerate(l):
            k = int(k)
            if x == 0:
                out[i, j] = float(-b / 2) if k == 0 else 0.0
                continue
            i_k = mp.sqrt(mp.pi / (2 * a)) * mp.besseli(k + half, a)
            sign = (-1) ** k if x > 0 else 1
            out[i, j] = float(-b * mp.sqrt(2 * k + 1) * sign * i_k / (2 * mp.cosh(b * x / 2)))
    return out


def kernels_case(ref):
    w200 = np.array(ref.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=200))
    w201 = np.array(ref.HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=201))
    mid = w201[100]
    assert 0 < abs(mid) < 1e-14
    w201z = w201.copy()
    w201z[100] = 0.0
    grids = (('w200', np.arange(30), w200), ('w201z', np.arange(30), w201z),
             ('wmid', np.arange(30), np.array([-abs(mid), abs(mid)])),
             ('wwide', np.arange(80), np.arange(-20.0, 20.25, 0.5)),
             ('wsmall', np.arange(80), np.array([-3e-3, -1e-6, 1e-6, 3e-3])),
             ('even', np.arange(0, 30, 2), w200), ('shuffled', SHUFFLED.copy(), w200), ('l0', np.array([0]), w201z))
    out = dict(beta=BETA)
    for name, l, w in grids:
        out['w_' + name], out['l_' + name], out['K_' + name] = w, l, truth(l, w)
        print('   %s: %d x %d' % (name, len(l), len(w)))
    # the subsets are rows of the contiguous truth
    assert np.array_equal(out['K_even'], out['K_w200'][::2]) and np.array_equal(out['K_shuffled'], out['K_w200'][SHUFFLED])
    np.savez_compressed(os.path.join(HERE, 'legendre_kernels.npz'), **out)
    print('legendre_kernels: %d bytes' % os.path.getsize(os.path.join(HERE, 'legendre_kernels.npz')))
    return out


# ---- 2. the reference on the true kernel -----------------------------------------------------------------------
def single_case(ref, kk):
    l, w, K = kk['l_w200'], kk['w_w200'], kk['K_w200']
    print('legendre')
    for seed in SEEDS:
        run = reference_run(ref, l.astype(float), w, K, seed)
        if run is not None:
            break
    assert run is not None, 'no seed of SEEDS at which the reference converged at every alpha'
    out = dict(beta=BETA, l=l, seed=seed)
    out.update(run)
    np.savez_compressed(os.path.join(HERE, 'legendre.npz'), **out)
    print('   seed %d, %d bytes' % (seed, os.path.getsize(os.path.join(HERE, 'legendre.npz'))))
    return out


# ---- 3. the element-wise problem through the pinned port -------------------------------------------------------
def matrix_spectrum(w):
    mu, s = np.array([-1.5, 1.5]), np.array([0.4, 0.7])
    A_diag = np.exp(-(w[None, :] - mu[:, None]) ** 2 / (2 * s[:, None] ** 2))
    A_diag /= np.trapezoid(A_diag, w, axis=1)[:, None]
    Rm, _ = np.linalg.qr(np.random.RandomState(2024).randn(2, 2))
    return np.einsum('ik,kw,jk->ijw', Rm, A_diag, Rm)


def elementwise_case(kk):
    l, w, K = kk['l_w200'], kk['w_w200'], kk['K_w200']
    delta = R.omega_delta(w)
    n_orb, n_alpha = 2, 8
    A_mat = matrix_spectrum(w)
    noise = SIGMA * np.random.RandomState(2026).randn(n_orb, n_orb, len(l))
    G_l = np.einsum('lw,ijw->ijl', K * delta[None, :], A_mat) + 0.5 * (noise + noise.transpose(1, 0, 2))
    U, S, V = R.svd_reduce(K, 1e-14)
    D = R.flat_default_model(w)
    err = SIGMA * np.ones(len(l))
    mesh = R.log_alpha_mesh(1e-1, 1e3, n_alpha)
    H_ref = np.empty((n_orb, n_orb, n_alpha, len(w)))
    H_truth = np.empty_like(H_ref)
    for i in range(n_orb):
        for j in range(n_orb):
            ent = 'normal' if i == j else 'plusminus'
            p = R.Problem(K, U, S, V, G_l[i, j], err, D, entropy=ent)
            out = R.alpha_loop(p, delta, mesh)
            assert np.all(out['converged']), ('the port did not converge at every alpha', i, j)
            H_ref[i, j] = out['H']
            for ia in range(n_alpha):
                info = {}
                _, H_truth[i, j, ia] = hp_truth.polish(K, G_l[i, j], err, D, V, S, out['alpha'][ia], out['v'][ia],
                                                       ent, iters=6, info=info)
                assert info['converged'], ('polish', i, j, ia, info)
    e = np.linalg.norm(H_ref - H_truth, axis=-1) / np.linalg.norm(H_truth, axis=-1)
    print('legendre_elementwise: port-vs-truth max %.2e' % e.max())
    # (without delta and D, which follow from omega: the file stays below boson_elementwise.npz)
    np.savez_compressed(os.path.join(HERE, 'legendre_elementwise.npz'), beta=BETA, l=l, omega=w,
                        G_l=G_l, A_mat=A_mat, err=SIGMA, alpha_mesh=np.array(mesh), H_ref=H_ref, H_truth=H_truth)


# ---- 4. bins ---------------------------------------------------------------------------------------------------
def bins_case(kk):
    l, w, K = kk['l_w200'], kk['w_w200'], kk['K_w200']
    delta = R.omega_delta(w)
    A = spectrum(w)
    s_bins = (K * delta[None, :]) @ A + BIN_SIGMA * np.random.RandomState(2027).randn(24, len(l))
    A_mat = matrix_spectrum(w)
    n = 12
    G = np.einsum('lw,ijw->ijl', K[:n] * delta[None, :], A_mat)
    e_bins = G[None] + BIN_SIGMA * np.random.RandomState(2028).randn(12, 2, 2, n)
    np.savez_compressed(os.path.join(HERE, 'legendre_bins.npz'), beta=BETA, omega=w, s_l=l, s_bins=s_bins, s_A_true=A,
                        e_l=l[:n], e_bins=e_bins, e_A_true=A_mat)
    print('legendre_bins: %d bytes' % os.path.getsize(os.path.join(HERE, 'legendre_bins.npz')))


def main():
    if 'triqs_maxent' not in sys.modules:
        import_reference()
    import triqs_maxent as ref
    if '--reuse-kernels' in sys.argv:             # (the 40-digit evaluation takes a while)
        with np.load(os.path.join(HERE, 'legendre_kernels.npz')) as d:
            kk = {k: d[k] for k in d.files}
    else:
        kk = kernels_case(ref)
    single_case(ref, kk)
    elementwise_case(kk)
    bins_case(kk)


if __name__ == '__main__':
    main()
