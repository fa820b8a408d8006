#!/usr/bin/env python3
"""Generate svd_truth.npz: small adversarial matrices for the device SVD and their singular values in 40 digits.

Unlike the other generators this one needs no reference checkout: numpy (fixed ``RandomState`` seeds) builds each
matrix in binary64, and mpmath (``svd_r(..., compute_uv=False)`` at 40 digits) decomposes THAT binary64 matrix; the
values are rounded to binary64.  The GPU tests (tests/test_gpu_svd_matrices.py) and the CPU check of the fixture
(tests/test_svd_truth_fixture.py) read only the .npz.

Per case ``<name>`` the file holds ``K_<name>`` (m x n), ``omega_<name>`` (n points, linspace(-5, 5, n); 0 for n = 1)
and ``S_<name>`` (min(m, n) values, descending).  ``names`` lists the cases.

  graded_48x72, graded_64x96   S = 10**linspace(1, -17, m) between random orthogonal factors
  graded_tall_72x48            the same with more rows than columns
  odd_rank_40x60               33 outer products with weights 10**linspace(0, -10, 33): rank 33, the rest exactly 0
                               in exact arithmetic (1e-17 rounding noise in the binary64 matrix)
  clustered_32x50              values 1 (x8), 1e-3 (x8), 1e-6 (x8), the other 8 zero
  perm_diag_40x40              a permutation matrix times diag(1..40)
  eye_40x40                    all values equal: the tie-break of the final ordering
  rank3_dup_30x45              rank 3, duplicated columns, two zero columns and one zero row
  one_row_1x37, one_col_37x1, one_by_one_1x1   truth is the 2-norm
  narrow_5x3, narrow_3x5, narrow_63x65, narrow_65x63   Gaussian (wave-size edges, odd rank of the QR stage)
  zeros_7x9                    all zero

The file is written with fixed zip time stamps, so a second run reproduces it bit for bit.

Usage:  python tests/golden/make_golden_svd.py
"""

import io
import os
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'svd_truth.npz')


def orth(rng, n, k):
    """n x k with orthonormal columns (to binary64 rounding)"""
    q, r = np.linalg.qr(rng.randn(n, k))
    return q * np.sign(np.diag(r))[None, :]


def with_spectrum(seed, m, n, s):
    rng = np.random.RandomState(seed)
    k = len(s)
    return (orth(rng, m, k) * np.asarray(s)[None, :]) @ orth(rng, n, k).T


def cases():
    out = []
    out.append(('graded_48x72', with_spectrum(101, 48, 72, 10.0 ** np.linspace(1, -17, 48))))
    out.append(('graded_64x96', with_spectrum(102, 64, 96, 10.0 ** np.linspace(1, -17, 64))))
    out.append(('graded_tall_72x48', with_spectrum(103, 72, 48, 10.0 ** np.linspace(1, -17, 48))))
    rng = np.random.RandomState(104)
    K = np.zeros((40, 60))
    for wgt in 10.0 ** np.linspace(0, -10, 33):
        u, v = rng.randn(40), rng.randn(60)
        K += wgt * np.outer(u / np.linalg.norm(u), v / np.linalg.norm(v))
    out.append(('odd_rank_40x60', K))
    out.append(('clustered_32x50', with_spectrum(105, 32, 50, np.repeat([1.0, 1e-3, 1e-6], 8))))
    rng = np.random.RandomState(106)
    out.append(('perm_diag_40x40', np.eye(40)[rng.permutation(40)] @ np.diag(np.arange(1.0, 41.0))))
    out.append(('eye_40x40', np.eye(40)))
    rng = np.random.RandomState(107)
    B = rng.randn(30, 3) @ rng.randn(3, 45)
    B[:, 7] = B[:, 3]
    B[:, 40] = B[:, 3]
    B[:, 11] = 2.0 * B[:, 5]
    B[:, 20] = 0.0
    B[:, 44] = 0.0
    B[13, :] = 0.0
    out.append(('rank3_dup_30x45', B))
    rng = np.random.RandomState(108)
    out.append(('one_row_1x37', rng.randn(1, 37)))
    out.append(('one_col_37x1', rng.randn(37, 1)))
    out.append(('one_by_one_1x1', rng.randn(1, 1)))
    for m, n in ((5, 3), (3, 5), (63, 65), (65, 63)):
        out.append(('narrow_%dx%d' % (m, n), np.random.RandomState(1000 * m + n).randn(m, n)))
    out.append(('zeros_7x9', np.zeros((7, 9))))
    return out


def truth(K):
    import mpmath as mp
    mp.mp.dps = 40
    m, n = K.shape
    if not K.any():
        return np.zeros(min(m, n))
    A = mp.matrix(m, n)
    for i in range(m):
        for j in range(n):
            A[i, j] = mp.mpf(float(K[i, j]))
    if m < n:
        A = A.T
    S = mp.svd_r(A, compute_uv=False)
    return np.sort(np.array([float(S[i]) for i in range(min(m, n))]))[::-1].copy()


def write_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member (the file is reproducible bit for bit)"""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    arrays = {}
    names = []
    for name, K in cases():
        K = np.ascontiguousarray(K, dtype=np.float64)
        t0 = time.time()
        S = truth(K)
        n = K.shape[1]
        arrays['K_' + name] = K
        arrays['omega_' + name] = np.linspace(-5.0, 5.0, n) if n > 1 else np.zeros(1)
        arrays['S_' + name] = S
        names.append(name)
        Sl = np.linalg.svd(K, compute_uv=False)
        print('%-20s %3d x %3d  S_0 %.3e  S_min %.3e  LAPACK-truth %.2e S_0  (%.1f s)'
              % (name, K.shape[0], K.shape[1], S[0], S[-1], np.abs(Sl - S).max() / max(S[0], 1e-300), time.time() - t0))
    arrays['names'] = np.array(names)
    write_npz(OUT, arrays)
    print('svd_truth.npz: %d bytes' % os.path.getsize(OUT))


if __name__ == '__main__':
    main()
