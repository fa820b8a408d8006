"""Host side of the posterior samples: the counter-based generator's numpy mirror against the published Philox known
answers, a numpy prototype of the four-line recipe of ``mxe_posterior_sample`` against the dense covariance, the
extended-precision truth the GPU tests compare against, and the argument checks of ``maxent_amd.posterior``.

Truth (independent of the Woodbury form the kernel evaluates): with ``sw = sqrt(w)``, ``Y = diag(sw) K^T Sigma^-1/2`` and
``a = alpha~ / eta`` in ``np.longdouble``,

    Gamma = (1 / eta) diag(sw) (a I + Y Y^T)^-1 diag(sw),      delta = diag(sw) (a I + Y Y^T)^-1 (sw o r) / sqrt(eta)

by a Cholesky solve of the n_omega x n_omega matrix, for the right-hand side ``sw o r = sqrt(a) z1 + sw o (V' (c o z2))``.
"""
import os

import numpy as np
import pytest

from maxent_amd import device, posterior
from test_posterior_errors_host import LD, cholesky_ld, forward_ld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- truth and prototype (the GPU tests import these) ------------------------------------------------------------------

def backward_ld(L, Z):
    """L^-T Z, columns at once"""
    X = np.array(Z, dtype=LD)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] /= L[k, k]
        X[:k] -= np.outer(L[k, :k], X[k])
    return X


def whitened_basis(K, err):
    """(V', c) with K^T Sigma^-1 K = V' c^2 V'^T, from numpy's SVD of the whitened kernel (binary64)"""
    C = np.asarray(K, dtype=float) / (np.asarray(err, dtype=float) * np.ones(np.shape(K)[0]))[:, None]
    _, c, Vt = np.linalg.svd(C, full_matrices=False)
    return Vt.T, c


def truth_samples(K, err, w, alpha, Vp, c, z, eta=1.0):
    """(delta (n_samples, n_omega), Gamma (n_omega, n_omega)) in longdouble for the normals z (n_samples, n_omega + n_s) and
    the basis (V', c) the right-hand side is formed with"""
    K = np.asarray(K, dtype=LD)
    err = np.asarray(err, dtype=LD) * np.ones(K.shape[0], dtype=LD)
    w, Vp, c, z = (np.asarray(x, dtype=LD) for x in (w, Vp, c, z))
    n = K.shape[1]
    a = LD(alpha) / LD(eta)
    sw = np.sqrt(w)
    Y = sw[:, None] * (K / err[:, None]).T
    A = np.dot(Y, Y.T)
    A[np.diag_indices_from(A)] += a
    L = cholesky_ld(A)
    rhs = np.sqrt(a) * z[:, :n].T + sw[:, None] * np.dot(Vp, c[:, None] * z[:, n:].T)        # n_omega x n_samples
    delta = sw[:, None] * backward_ld(L, forward_ld(L, rhs)) / np.sqrt(LD(eta))
    Z = forward_ld(L, np.diag(sw))
    return delta.T, np.dot(Z.T, Z) / LD(eta)


def prototype(Vp, c, w, alpha, z, eta=1.0):
    """the four lines of ``mxe_posterior_sample`` in binary64 numpy: z (n_samples, n_omega + n_s) -> delta"""
    n = len(w)
    a = alpha / eta
    W = np.dot(Vp.T * w, Vp)
    L = np.linalg.cholesky(c[:, None] * W * c[None, :] + a * np.eye(len(c)))
    q = np.sqrt(a * w) * z[:, :n] + w * np.dot(z[:, n:] * c, Vp.T)
    y = c * np.dot(q, Vp)
    x = np.linalg.solve(L.T, np.linalg.solve(L, y.T)).T
    return (q - w * np.dot(x * c, Vp.T)) / a / np.sqrt(eta)


def dense_problem(n_tau=12, n_omega=20, seed=5):
    rng = np.random.RandomState(seed)
    tau = np.linspace(0.0, 6.0, n_tau)
    omega = np.linspace(-3.0, 3.0, n_omega)
    K = np.exp(-np.outer(tau, omega) / 3.0) / (1.0 + np.exp(-2.0 * omega))[None, :]
    w = np.exp(-(omega - 0.5) ** 2) * (omega[1] - omega[0]) * (1.0 + 0.1 * rng.rand(n_omega))
    err = 1e-2 * (1.0 + rng.rand(n_tau))
    return omega, K, w, err


# ---- the generator ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('counter, key, words', [
    ([0, 0, 0, 0], [0, 0], '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ([0xffffffff] * 4, [0xffffffff] * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, words):
    got = posterior.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and ' '.join('%08x' % v for v in got) == words


def test_sample_normals_rows_depend_on_seed_stream_and_sample_alone():
    z = posterior.sample_normals(11, 5, 40, 53)
    assert z.shape == (40, 53) and np.all(np.abs(z) < 8.7)
    assert np.array_equal(posterior.sample_normals(11, 5, 7, 53), z[:7])
    # an odd n cuts the last pair, nothing else
    assert np.array_equal(posterior.sample_normals(11, 5, 40, 54)[:, :53], z)
    other_stream, other_seed = posterior.sample_normals(11, 6, 40, 53), posterior.sample_normals(12, 5, 40, 53)
    assert not np.any(other_stream == z) and not np.any(other_seed == z)
    big = posterior.sample_normals(2 ** 63 + 3, 2 ** 40 + 1, 2, 4)              # (all 64 bits of seed and stream count)
    assert not np.any(big == posterior.sample_normals(3, 1, 2, 4))
    # the extreme uniforms: u = 2^-54 gives the largest |z| there is
    assert np.sqrt(-2.0 * np.log(0.5 * 2.0 ** -53)) < 8.7
    with pytest.raises(ValueError):
        posterior.sample_normals(0, 0, 0, 4)


def test_moments_of_65536_normals():
    z = posterior.sample_normals(20261018, 0, 1, 1 << 16)[0]
    n = len(z)
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)


# ---- the recipe ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('alpha, eta', [(0.5, 1.0), (40.0, 2.5)])
def test_numpy_prototype_reproduces_a_factor_of_gamma(alpha, eta):
    omega, K, w, err = dense_problem()
    Vp, c = whitened_basis(K, err)
    n, ns = len(omega), len(c)
    assert ns == 12
    F = prototype(Vp, c, w, alpha, np.eye(n + ns), eta).T                # delta = F z: unit vectors give the columns of F
    _, gamma = truth_samples(K, err, w, alpha, Vp, c, np.zeros((1, n + ns)), eta)
    hess = eta * np.dot(K.T / err ** 2, K) + alpha * np.diag(1.0 / w)      # the dense P of the issue
    np.testing.assert_allclose(np.dot(gamma.astype(float), hess), np.eye(n), atol=1e-9)
    scale = np.sqrt(np.outer(np.diag(gamma), np.diag(gamma))).astype(float)
    assert np.max(np.abs(np.dot(F, F.T) - gamma.astype(float)) / scale) <= 1e-10
    # and the truth's own samples are the prototype's
    z = posterior.sample_normals(1, 2, 5, n + ns)
    d_t, _ = truth_samples(K, err, w, alpha, Vp, c, z, eta)
    assert np.max(np.abs(prototype(Vp, c, w, alpha, z, eta) - d_t.astype(float)) / np.sqrt(np.diag(gamma).astype(float))) <= 1e-10


def test_a_zero_weight_gives_a_zero_row():
    omega, K, w, err = dense_problem()
    w = w.copy()
    w[3] = 0.0
    Vp, c = whitened_basis(K, err)
    d = prototype(Vp, c, w, 2.0, posterior.sample_normals(0, 0, 4, len(w) + len(c)))
    assert np.all(d[:, 3] == 0.0) and np.all(np.isfinite(d))


# ---- host glue -------------------------------------------------------------------------------------------------------

class _Omega(object):
    def __init__(self, n):
        self.delta = np.full(n, 0.1)


class _K(object):
    S = np.ones(3)


def _item(kind=device.ENTROPY_NORMAL, n_alpha=4, n=6):
    return dict(spec=dict(kind=kind, D=np.ones(n), G=np.zeros(2), err=1.0, alpha=np.ones(n_alpha)), H=np.ones((n_alpha, n)),
                alpha=np.ones(n_alpha), analysis={'LineFitAnalyzer': dict(alpha_index=1)}, probability=None, B=None)


def test_argument_errors_are_raised_before_any_device_work():
    om, K = _Omega(6), _K()
    with pytest.raises(ValueError, match='n_samples'):
        posterior.element_samples(K, om, [_item()], n_samples=0)
    with pytest.raises(ValueError, match='transform'):
        posterior.element_samples(K, om, [_item()], transform='sqrt')
    with pytest.raises(ValueError, match='plus-minus'):
        posterior.element_samples(K, om, [_item(device.ENTROPY_PLUSMINUS)], transform='log')
    with pytest.raises(ValueError, match='z: the shape'):
        posterior.element_samples(K, om, [_item()], n_samples=5, z=np.zeros((5, 8)))
    with pytest.raises(ValueError, match='not finite'):
        posterior.element_samples(K, om, [_item()], n_samples=5, z=np.full((5, 9), np.nan))
    with pytest.raises(ValueError, match='Probability not calculated'):
        posterior.element_samples(K, om, [_item()], alpha='bryan')


def test_log_transform_is_positive_and_first_order():
    H = np.array([[1.0, 2.0, 0.0]])
    d = np.array([[[1e-6, -5.0, 0.0], [-1e-6, 1.0, 0.0]]])
    lin, log = posterior.apply_transform(H, d, 'linear'), posterior.apply_transform(H, d, 'log')
    assert lin.shape == (1, 2, 3) and np.array_equal(lin, H[:, None, :] + d)
    assert np.all(log[..., :2] > 0) and np.all(log[..., 2] == 0)
    np.testing.assert_allclose(log[0, :, 0], lin[0, :, 0], rtol=1e-11)


def test_bryan_allotment_is_reproducible_and_complete():
    p = np.array([0.1, 0.6, 0.3])
    a = posterior.bryan_allotment(p, 500, seed=9)
    assert np.array_equal(a, posterior.bryan_allotment(p, 500, seed=9)) and a.shape == (500,)
    counts = np.bincount(a, minlength=3)
    assert counts.sum() == 500 and counts[1] > counts[2] > counts[0] > 0
    assert not np.array_equal(a, posterior.bryan_allotment(p, 500, seed=10))
    assert not np.array_equal(a, posterior.bryan_allotment(p, 500, seed=9, stream_base=1))
    assert posterior.stream_id(5, 1, 30, 7) == (5 * 2 + 1) * 30 + 7


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, 'include', 'maxent_hip.h')) as f:
        header = f.read()
    lib = device.load_library()
    for name in ('mxe_posterior_sample', 'mxe_normals'):
        assert 'int  %s(' % name in header, name
        assert getattr(lib, name) is not None, name                     # (AttributeError: not exported)
    assert 'mxe_posterior_sample (draws of H' in header                 # (the mapping table at the top)
