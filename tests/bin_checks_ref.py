"""numpy / longdouble restatement of ``bins_check_kernel`` (mxe_bincheck.hip.h): the blocking ladder and the
standardised moments of the block means.  A helper of tests/test_bin_checks_host.py and tests/test_gpu_bin_checks.py: it
needs no GPU."""
import numpy as np

EPS = np.finfo(float).eps
LD = np.longdouble


def n_levels(n_bins):
    return int(n_bins).bit_length() - 1


def ladder_ref(bins, T=None, rank=None):
    """one set: bins (n_bins, n_data), the bin index being Monte Carlo time.  ``T`` (n_data, n_data) and ``rank``: the
    columns are y[b][k] = sum_j T[k][j] (bins[b][j] - mean[j]) for k < rank and zeros behind; both None: y = bins - mean.
    Per level k = 0 .. floor(log2 n_bins) - 1: n_k = n_bins >> k blocks of 2^k bins (a remainder dropped), block means B_q,
    mu_p = mean_q (B_q - mean B)^p.  Returns err2 = mu_2 / (n_k - 1), skew = mu_3 / mu_2^1.5, kurt = mu_4 / mu_2^2 - 3, each
    (L, n_data) longdouble; mu_2 == 0: 0, NaN, NaN."""
    b = np.asarray(bins, dtype=LD)
    m, n = b.shape
    y = b - (b.sum(axis=0) / LD(m))[None, :]
    if T is not None:
        Tk = np.array(T, dtype=LD).reshape(n, n)
        Tk[int(rank):] = 0
        y = y @ Tk.T
    L = n_levels(m)
    err2 = np.zeros((L, n), dtype=LD)
    skew = np.full((L, n), np.nan, dtype=LD)
    kurt = np.full((L, n), np.nan, dtype=LD)
    for k in range(L):
        bk, nk = 1 << k, m >> k
        B = y[:nk * bk].reshape(nk, bk, n).sum(axis=1) / LD(bk)
        d = B - (B.sum(axis=0) / LD(nk))[None, :]
        mu2, mu3, mu4 = [(d ** p).sum(axis=0) / LD(nk) for p in (2, 3, 4)]
        ok = mu2 > 0
        err2[k][ok] = mu2[ok] / LD(nk - 1)
        skew[k][ok] = mu3[ok] / mu2[ok] ** LD(1.5)
        kurt[k][ok] = mu4[ok] / mu2[ok] ** 2 - 3
    return dict(err2=err2, skew=skew, kurt=kurt)


def ar1_bins(n_bins, n_data, rho, seed, scale=1e-3, offset=3.0):
    """AR(1) bins x_i = rho x_i-1 + sqrt(1 - rho^2) e_i of unit variance per column, mixed by a fixed random n_data x
    n_data matrix, scaled and offset"""
    rng = np.random.RandomState(seed)
    e = rng.randn(n_bins, n_data)
    x = np.empty_like(e)
    x[0] = e[0]
    c = np.sqrt(1.0 - rho * rho)
    for i in range(1, n_bins):
        x[i] = rho * x[i - 1] + c * e[i]
    mix = rng.randn(n_data, n_data)
    return offset + scale * (x @ mix)


def gates(got, ref, err2_abs=0.0):
    """the largest violations (<= 1 passes) of  |d err2| <= 1e-10 err2 + err2_abs,  |d skew| <= 1e-9,
    |d kurt| <= 1e-9 (1 + |kurt|);  NaN must meet NaN.  ``err2_abs``: an array like err2, or 0.  Returns
    (dict of the three ratios, dict of the three largest plain errors: relative, absolute, absolute)."""
    e_ref = np.asarray(ref['err2'], dtype=LD)
    de = np.abs(np.asarray(got['err2'], dtype=LD) - e_ref)
    worst, plain = {}, {}
    worst['err2'] = float(np.max(de / np.maximum(LD(1e-10) * e_ref + err2_abs, LD(1e-300)) * (de > 0)))
    with np.errstate(divide='ignore', invalid='ignore'):
        plain['err2'] = float(np.nanmax(np.where(e_ref > 0, de / e_ref, 0)))
    for name, rel in (('skew', 0.0), ('kurt', 1.0)):
        r = np.asarray(ref[name], dtype=LD)
        g = np.asarray(got[name], dtype=LD)
        assert np.array_equal(np.isnan(r), np.isnan(g)), name + ': NaN where the reference has none, or the reverse'
        there = ~np.isnan(r)
        if not there.any():
            worst[name] = plain[name] = 0.0
            continue
        d = np.abs(g[there] - r[there])
        worst[name] = float(np.max(d / (LD(1e-9) * (1 + rel * np.abs(r[there])))))
        plain[name] = float(np.max(d))
    return worst, plain
