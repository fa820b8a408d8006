"""device time (fill + preblur-free SVD, between the events of the library) of the bosonic entries and of
mxe_kernel_svd_data, next to mxe_kernel_svd at equal shape and to host LAPACK (one BLAS thread, as KernelSVD.svd):
100 x 200 and 200 x 500, beta = 40; third call of each (the first loads the code object)"""
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import maxent_amd as mx
from maxent_amd import device, kernels

BETA = 40.0


def third(f):
    for _ in range(2):
        f()
    t0 = time.perf_counter()
    r = f()[0]
    return r, (time.perf_counter() - t0) * 1e3


for n_tau, n_w in ((100, 200), (200, 500)):
    tau = np.linspace(0, BETA, n_tau)
    om = mx.HyperbolicOmegaMesh(-10, 10, n_w)
    w, d = np.asarray(om), om.delta
    nu = 2 * np.pi * np.arange(n_tau // 2) / BETA            # stacked: n_tau rows
    Kb = np.asarray(mx.BosonicTauKernel(tau, om, beta=BETA).K)
    cases = [('mxe_kernel_svd (fermionic tau)', lambda: device.kernel_svd(tau, w, d, BETA), None),
             ('mxe_kernel_svd_boson', lambda: device.kernel_svd_boson(tau, w, d, BETA), Kb),
             ('mxe_kernel_svd_boson_iw', lambda: device.kernel_svd_boson_iw(nu, w, d),
              np.asarray(mx.BosonicIOmegaKernel(nu, om).K)),
             ('mxe_kernel_svd_data (bosonic tau matrix)', lambda: device.kernel_svd_data(Kb, w, d), Kb)]
    for name, f, K in cases:
        r, wall = third(f)
        line = '%d x %d %-42s device %.3f ms, call %.2f ms, n_s %d, qr_rank %d, sweeps %d' % (
            n_tau, n_w, name, r['ms'], wall, len(r['S']), r['qr_rank'], r['sweeps'])
        if K is not None:
            with kernels._one_blas_thread():
                t0 = time.perf_counter()
                np.linalg.svd(K, full_matrices=False)
                line += '; host LAPACK %.2f ms' % ((time.perf_counter() - t0) * 1e3)
        print(line, flush=True)
