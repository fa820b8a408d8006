"""device time (fill + preblur-free SVD, between the events of the library) of mxe_kernel_svd_legendre next to host
LAPACK (one BLAS thread, as KernelSVD.svd) on the same matrix: 30 x 200 (beta = 40) and 80 x 500 (beta = 40), and the
count of singular values >= 1e-14 at the three shapes of DESIGN.md 4p; third call of each (the first loads the code
object)"""
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import maxent_amd as mx
from maxent_amd import device, kernels


def third(f):
    for _ in range(2):
        f()
    t0 = time.perf_counter()
    r = f()[0]
    return r, (time.perf_counter() - t0) * 1e3


for beta, n_l, n_w, timed in ((40.0, 30, 200, True), (40.0, 40, 200, False), (40.0, 80, 500, True), (100.0, 120, 500, False)):
    om = mx.HyperbolicOmegaMesh(-10, 10, n_w)
    w, d, l = np.asarray(om), om.delta, np.arange(n_l)
    K = np.asarray(mx.LegendreKernel(l, om, beta=beta).K)
    with kernels._one_blas_thread():
        t0 = time.perf_counter()
        S = np.linalg.svd(K, full_matrices=False)[1]
        host = (time.perf_counter() - t0) * 1e3
    line = 'beta %g, %d x %d: %d singular values >= 1e-14 (LAPACK)' % (beta, n_l, n_w, int((S >= 1e-14).sum()))
    if timed:
        r, wall = third(lambda: device.kernel_svd_legendre(l, w, d, beta))
        line += '; mxe_kernel_svd_legendre device %.3f ms, call %.2f ms, n_s %d, qr_rank %d, sweeps %d; host LAPACK %.2f ms' % (
            r['ms'], wall, len(r['S']), r['qr_rank'], r['sweeps'], host)
    print(line, flush=True)
