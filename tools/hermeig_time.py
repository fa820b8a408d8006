"""Device time of ``mxe_hermitian_eig`` beside ``numpy.linalg.eigh`` on the same arrays on the same host:
random Hermitian matrices, real and complex -- A_out of a 16 x 16 job on 500 frequencies (500 matrices), the same job at
every alpha of a mesh of 100 (50 000 matrices), and the largest matrices the kernel takes.  Needs a GPU.

    python tools/hermeig_time.py
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maxent_amd import device


def main():
    rng = np.random.default_rng(1)
    for cplx in (False, True):
        for n_mat, m in ((500, 16), (50000, 16), (500, 2), (500, 64), (2000, 64)):
            X = rng.standard_normal((n_mat, m, m))
            if cplx:
                X = X + 1j * rng.standard_normal((n_mat, m, m))
            X = 0.5 * (X + np.conj(np.swapaxes(X, 1, 2)))
            for _ in range(2):
                device.hermitian_eig(X)                       # warm up: code object, allocations
            ms, wall = [], []
            for _ in range(5):
                t = {}
                t0 = time.perf_counter()
                got = device.hermitian_eig(X, timing=t)
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(t['ms'])
            lap, lap_eig = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                lam, V = np.linalg.eigh(X)
                lap_eig.append(1e3 * (time.perf_counter() - t0))
                np.einsum('bik,bk,bjk->bij', V, np.maximum(lam, 0), np.conj(V))
                lap.append(1e3 * (time.perf_counter() - t0))
            assert np.all(got['info'] >= 0)
            print(json.dumps(dict(cplx=cplx, n_mat=n_mat, m=m, kernel_ms=sorted(ms), call_ms=sorted(wall), eigh_ms=sorted(lap_eig),
                                  eigh_and_projection_ms=sorted(lap), max_sweeps=int(got['info'].max()),
                                  max_eigenvalue_gap=float(np.abs(got['lambda'] - lam).max()))), flush=True)


if __name__ == '__main__':
    main()
