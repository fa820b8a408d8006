"""The shrinkage covariance of the mean restated in numpy longdouble, for the tests of
``mxe_bins_eig_shrunk``: the intensity of Schaefer and Strimmer (2005) with the target "diagonal, unequal variances", its
numerator and denominator, the condition figure of the numerator, the shrunk covariance and the augmented matrix whose
Gram matrix it is.  Also the bins the tests use: AR(1)-correlated columns with variances over three decades."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(float).eps

#: (n_bins, n_data) of the device tests; the host test checks 0 < lambda_raw < 1 for each of them
SHAPES = [(24, 40), (12, 5), (130, 65), (4, 7), (2000, 8), (64, 200), (7, 1), (16, 512), (5, 63), (5, 64)]


def ar1_bins(m, n, rho=0.9, seed=0, offset=0.3):
    """m bins of n values: AR(1) along the data axis with coefficient ``rho``, standard deviations from 1 down to 1e-1.5
    (variances over three decades), around a mean of ``offset`` standard deviations"""
    rng = np.random.RandomState(1000 * seed + 7 * m + n)
    e = rng.randn(m, n)
    y = np.empty((m, n))
    y[:, 0] = e[:, 0]
    for j in range(1, n):
        y[:, j] = rho * y[:, j - 1] + np.sqrt(1.0 - rho * rho) * e[:, j]
    sd = 10.0 ** (-1.5 * np.arange(n) / max(n - 1, 1))
    return (y + offset) * sd[None, :]


def centred(b):
    """(b - mean, mean) of longdouble bins.  The mean of data that lie 10^6 standard deviations from zero is known to
    10^6 eps_longdouble = 1e-13 of a standard deviation only -- 500 eps of binary64; the mean of the deviations, which
    are of the size of the standard deviation, takes what is left of it away."""
    mean = b.mean(axis=0)
    x = b - mean
    rest = x.mean(axis=0)
    return x - rest, mean + rest


def intensity(bins):
    """dict: ``lam`` (clipped), ``raw``, ``num``, ``den`` (the two sums over i != j, in the units of the formulas: Var(r)
    and r^2), ``kappa`` (the cancellation of the numerator), ``used`` (columns with s_j > 0); all longdouble arithmetic"""
    b = np.asarray(bins, dtype=LD)
    m, n = b.shape
    x = centred(b)[0]
    s2 = (x * x).sum(axis=0) / LD(m - 1)
    used = s2 > 0
    z = x[:, used] / np.sqrt(s2[used])
    G1 = z.T @ z                                   # m w
    G2 = (z * z).T @ (z * z)
    off = ~np.eye(G1.shape[0], dtype=bool)
    wbar = G1 / LD(m)
    r = wbar * LD(m) / LD(m - 1)
    var_r = LD(m) / LD(m - 1) ** 3 * (G2 - LD(m) * wbar ** 2)
    num, den = var_r[off].sum(), (r[off] ** 2).sum()
    pos, neg = G2[off].sum(), (LD(m) * wbar[off] ** 2).sum()
    if den > 0:
        raw = num / den
        lam = min(LD(1), max(LD(0), raw))
    else:
        raw, lam = LD('nan'), LD(1)
    kappa = (pos + neg) / (pos - neg) if pos != neg else LD('inf')
    return dict(lam=lam, raw=raw, num=num, den=den, kappa=kappa, used=used)


def cov_parts(bins):
    """X = (bins - mean) / sqrt(m (m - 1)), C = X^T X, c = diag(C) and the mean, longdouble"""
    b = np.asarray(bins, dtype=LD)
    m = b.shape[0]
    x, mean = centred(b)
    X = x / np.sqrt(LD(m) * LD(m - 1))
    C = X.T @ X
    return X, C, np.diag(C).copy(), mean


def shrunk_cov(bins, lam):
    """C* = (1 - lam) X^T X + lam diag(c), longdouble"""
    _, C, c, _ = cov_parts(bins)
    lam = LD(lam)
    return (LD(1) - lam) * C + lam * np.diag(c)


def augmented(bins, lam):
    """Y = [sqrt(1 - lam) X ; sqrt(lam) diag(sqrt(c))], longdouble: Y^T Y = C*"""
    X, _, c, _ = cov_parts(bins)
    lam = LD(lam)
    return np.vstack([np.sqrt(LD(1) - lam) * X, np.sqrt(lam) * np.diag(np.sqrt(c))])


def ar1_true_cov_of_mean(m, n, rho):
    """the covariance of the mean of ``ar1_bins(m, n, rho)``: the law the bins are drawn from, over m"""
    sd = 10.0 ** (-1.5 * np.arange(n) / max(n - 1, 1))
    idx = np.arange(n)
    return sd[:, None] * sd[None, :] * rho ** np.abs(idx[:, None] - idx[None, :]) / m


def fresh_noise(cov, n_draws, seed):
    """n_draws vectors from N(0, cov)"""
    L = np.linalg.cholesky(cov)
    return np.random.RandomState(seed).randn(n_draws, cov.shape[0]) @ L.T


def chi2_per_direction(T, sigma, noise):
    """the mean over the draws of sum_k ((T e)_k / sigma_k)^2 / rank: 1 for errors that are right"""
    w = (np.asarray(noise) @ np.asarray(T).T) / np.asarray(sigma)[None, :]
    return float((w * w).sum(axis=1).mean() / len(sigma))


def eig_float(C):
    """(sigma ascending, T rows) of a covariance, LAPACK in binary64: the yardstick of the calibration only"""
    lam, V = np.linalg.eigh(np.asarray(C, dtype=float))
    keep = lam > 1e-12 * lam[-1]
    return np.sqrt(lam[keep]), V[:, keep].T


def lambda_bound(m, ref, c):
    """|lambda_dev - lambda_ref| <= c (m + 4) eps kappa lambda_ref: the rounding of an m-term sum with cancellation kappa"""
    return float(c * (m + 4) * EPS * ref['kappa'] * ref['lam'])
