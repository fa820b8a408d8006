#!/usr/bin/env python3
"""Generate bins_truth.npz: small matrices of Monte Carlo bins for ``mxe_bins_eig`` with their means and the singular
values of the centred, scaled matrix in 40 digits.

Needs no reference checkout: numpy (fixed ``RandomState`` seeds) builds each bin matrix in binary64, the centred and
scaled matrix ``X = (bins - mean) / sqrt(n_bins (n_bins - 1))`` is formed in binary64 too, and mpmath
(``svd_r(..., compute_uv=False)`` at 40 digits) decomposes THAT matrix; the values are rounded to binary64.  The mean
is the exact sum of the binary64 bins divided at 40 digits, rounded once (numpy's own mean is off by up to a few ulp,
which the centring of bins with a large mean and a small spread would magnify).  The GPU tests (tests/test_gpu_bins.py) read
only the .npz.

Per case ``<name>`` the file holds ``bins_<name>`` (n_bins x n_data), ``mean_<name>`` (n_data), ``X_<name>``
(n_bins x n_data, the binary64 matrix that was decomposed), ``S_<name>`` (min(n_bins, n_data) values, descending) and
``rank_<name>`` (the rank in exact arithmetic).  ``names`` lists the cases.

  well_96x48        Gaussian bins around a smooth mean: full rank 48, condition ~ 4
  graded_96x48      zero-mean Gaussian bins, column j scaled by 10**(-10 j / 47): sigma over 10 decades, every one
                    determined to high RELATIVE accuracy by the matrix
  short_24x40       n_bins < n_data: rank n_bins - 1 = 23 (the centred rows add up to zero)
  dup_80x36         columns 30..35 are copies of columns 0..5: rank 30
  const_64x32       column 7 is the same value in every bin: a zero-variance direction, rank 31

The file is written with fixed zip time stamps, so a second run reproduces it bit for bit.

Usage:  python tests/golden/make_golden_bins_truth.py
"""

import os
import time

import numpy as np

from make_golden_svd import truth, write_npz

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'bins_truth.npz')


def cases():
    out = []
    rng = np.random.RandomState(201)
    smooth = -0.5 * np.exp(-np.linspace(0, 3, 48)) - 0.1
    out.append(('well_96x48', smooth[None, :] + 1e-2 * rng.randn(96, 48), 48))
    rng = np.random.RandomState(202)
    out.append(('graded_96x48', rng.randn(96, 48) * (10.0 ** (-10.0 * np.arange(48) / 47.0))[None, :], 48))
    rng = np.random.RandomState(203)
    out.append(('short_24x40', -0.3 + 1e-2 * rng.randn(24, 40), 23))
    rng = np.random.RandomState(204)
    b = 0.7 + 1e-3 * rng.randn(80, 36)
    b[:, 30:] = b[:, :6]
    out.append(('dup_80x36', b, 30))
    rng = np.random.RandomState(205)
    b = -0.2 + 1e-2 * rng.randn(64, 32)
    b[:, 7] = -0.4375
    out.append(('const_64x32', b, 31))
    return out


def exact_mean(bins):
    import mpmath as mp
    mp.mp.dps = 40
    n_bins, n_data = bins.shape
    return np.array([float(mp.fsum(mp.mpf(float(x)) for x in bins[:, j]) / n_bins) for j in range(n_data)])


def main():
    arrays, names = {}, []
    for name, bins, rank in cases():
        bins = np.ascontiguousarray(bins, dtype=np.float64)
        n_bins, n_data = bins.shape
        t0 = time.time()
        mean = exact_mean(bins)
        X = (bins - mean[None, :]) / np.sqrt(float(n_bins) * (n_bins - 1))
        S = truth(X)
        arrays['bins_' + name] = bins
        arrays['mean_' + name] = mean
        arrays['X_' + name] = X
        arrays['S_' + name] = S
        arrays['rank_' + name] = np.array(rank)
        names.append(name)
        Sl = np.linalg.svd(X, compute_uv=False)
        print('%-14s %3d x %3d  S_0 %.3e  S_rank %.3e  next %.3e  LAPACK-truth %.2e S_0  (%.1f s)'
              % (name, n_bins, n_data, S[0], S[rank - 1], S[rank] if rank < len(S) else 0.0,
                 np.abs(Sl - S).max() / S[0], time.time() - t0))
    arrays['names'] = np.array(names)
    write_npz(OUT, arrays)
    print('bins_truth.npz: %d bytes' % os.path.getsize(OUT))


if __name__ == '__main__':
    main()
