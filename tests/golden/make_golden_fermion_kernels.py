#!/usr/bin/env python3
"""Generate fermion_kernels.npz: 40-digit truth for the fills and the blur matrix every ordinary run goes through.

Like the kernel part of make_golden_boson.py, but it needs nothing beyond this repository and mpmath: the grids come
from maxent_amd's own mesh classes, their binary64 values are stored, and every truth is formed with mpmath at 40
digits FROM THE STORED VALUES (never from a formula for the grid), then rounded to binary64.  beta = 40.

  tau        36 points: linspace(0, beta, 33) with 1e-7, beta - 1e-7 and beta / 3 sorted in
  tau_one    the one-point grid [beta / 3]                       (37 imaginary times in all)
  w_hyp67    HyperbolicOmegaMesh(-10, 10, 67)
  w_wide41   linspace(-60, 60, 41): beta |w| up to 2400, most entries below the smallest binary64 number
  w_zero     [-1e-3, 0, 1e-300, 3]
  iw         (2 n + 1) pi / beta, n = 0..15

  K_tau_<w>, K_tau_one_<w>   K(tau, w) = -e^{-tau w} / (1 + e^{-beta w}) on every (tau grid, omega grid) pair
  K_iw_<w>                   1 / (i w_n - w), stacked [Re K ; Im K] (32 rows), on hyp67 and zero

  The blur matrix, by the steps of maxent_amd.preblur.get_preblur (Gaussian; divided by the delta-weighted sums
  over its first index; then by the delta-weighted sums over the second index), with the mesh's own ``delta``,
  on lin<n> = DataOmegaMesh(linspace(-5, 5, n)), n in PB_N, and hyp<n> = HyperbolicOmegaMesh(-5, 5, n), n >= 3, for
  the widths pb_b.  The sums run over the whole matrix; only the rows pb_rows_<n> = {0, 1, n//2, n-2, n-1} are stored:
  pb_w_<mesh>, pb_delta_<mesh>, pb_B_<mesh>  (widths x stored rows x n)
  and pb_Blo_<mesh>, the truth minus its binary64 value pb_B rounded to binary64 again: pb_B + pb_Blo is the truth to
  about 32 digits, for the tests that hold an extended-precision restatement against it.

The file is written with fixed zip time stamps and sorted keys: a second run gives the same bytes.

Usage:  python tests/golden/make_golden_fermion_kernels.py        (a few minutes)
"""

import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from maxent_amd.omega_meshes import DataOmegaMesh, HyperbolicOmegaMesh          # noqa: E402

BETA = 40.0
N_IW = 16
PB_N = (2, 3, 255, 257, 513)
PB_B = (1e-3, 0.05, 0.3, 50.0)
DPS = 40


def stored_rows(n):
    return np.array(sorted({0, 1, n // 2, n - 2, n - 1}), dtype=np.int64)


def truth_tau(tau, w, mp):
    b = mp.mpf(BETA)
    out = np.empty((len(tau), len(w)))
    for i, t in enumerate(tau):
        t = mp.mpf(float(t))
        for j, x in enumerate(w):
            x = mp.mpf(float(x))
            out[i, j] = float(-mp.exp(-t * x) / (1 + mp.exp(-b * x)))
    return out


def truth_iw(iw, w, mp):
    re, im = np.empty((len(iw), len(w))), np.empty((len(iw), len(w)))
    for i, n_ in enumerate(iw):
        n_ = mp.mpf(float(n_))
        for j, x in enumerate(w):
            z = 1 / mp.mpc(-mp.mpf(float(x)), n_)
            re[i, j], im[i, j] = float(z.real), float(z.imag)
    return np.concatenate([re, im])


def truth_preblur(w, delta, b, rows, mp):
    """get_preblur(omega, b)[rows], every step in 40 digits"""
    n = len(w)
    w = [mp.mpf(float(x)) for x in w]
    d = [mp.mpf(float(x)) for x in delta]
    b = mp.mpf(float(b))
    norm = mp.sqrt(2 * mp.pi * b ** 2)
    # B = exp(-diff ** 2 / 2 / b ** 2) / sqrt(2 pi b ** 2), diff[i][j] = w_j - w_i (equal for (i, j) and (j, i))
    G = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            G[i][j] = G[j][i] = mp.exp(-(w[j] - w[i]) ** 2 / 2 / b ** 2) / norm
    # B = B / dot(delta, B)[:, newaxis]
    c = [sum(d[k] * G[k][i] for k in range(n)) for i in range(n)]
    B1 = [[G[i][j] / c[i] for j in range(n)] for i in range(n)]
    # B = B / dot(B, delta)[newaxis, :]
    s = [sum(B1[j][k] * d[k] for k in range(n)) for j in range(n)]
    hi, lo = np.empty((len(rows), n)), np.empty((len(rows), n))
    for r, i in enumerate(rows):
        for j in range(n):
            x = B1[i][j] / s[j]
            hi[r, j] = float(x)
            lo[r, j] = float(x - mp.mpf(hi[r, j]))
    return hi, lo


def save(path, arrays):
    """an .npz with sorted members and fixed time stamps (numpy's savez stamps the members with the clock)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(arrays[key]), allow_pickle=False)


def main():
    import mpmath as mp
    mp.mp.dps = DPS
    tau = np.sort(np.concatenate([np.linspace(0, BETA, 33), [1e-7, BETA - 1e-7, BETA / 3]]))
    tau_one = np.array([BETA / 3])
    grids = dict(hyp67=np.array(HyperbolicOmegaMesh(omega_min=-10, omega_max=10, n_points=67)),
                 wide41=np.linspace(-60, 60, 41), zero=np.array([-1e-3, 0.0, 1e-300, 3.0]))
    iw = (2 * np.arange(N_IW) + 1) * np.pi / BETA
    out = dict(beta=np.float64(BETA), tau=tau, tau_one=tau_one, iw=iw, pb_b=np.array(PB_B), pb_n=np.array(PB_N))
    for name, w in grids.items():
        out['w_' + name] = w
        out['K_tau_' + name] = truth_tau(tau, w, mp)
        out['K_tau_one_' + name] = truth_tau(tau_one, w, mp)
        if name != 'wide41':
            out['K_iw_' + name] = truth_iw(iw, w, mp)
    for n in PB_N:
        rows = stored_rows(n)
        out['pb_rows_%d' % n] = rows
        meshes = [('lin%d' % n, DataOmegaMesh(np.linspace(-5, 5, n)))]
        if n >= 3:
            meshes.append(('hyp%d' % n, HyperbolicOmegaMesh(omega_min=-5, omega_max=5, n_points=n)))
        for name, mesh in meshes:
            w, delta = np.array(mesh, dtype=float), np.array(mesh.delta, dtype=float)
            out['pb_w_' + name], out['pb_delta_' + name] = w, delta
            both = [truth_preblur(w, delta, b, rows, mp) for b in PB_B]
            out['pb_B_' + name] = np.stack([hi for hi, _ in both])
            out['pb_Blo_' + name] = np.stack([lo for _, lo in both])
            print('%s done' % name, flush=True)
    path = os.path.join(HERE, 'fermion_kernels.npz')
    save(path, out)
    print('fermion_kernels: %d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
