"""Times of a default-model scan at the size of DESIGN.md 4v: 16 x 16 elements x 8 models x 100 alphas x 500 omega points.

1. ``mxe_evidence_reduce`` alone on 2048 scans of synthetic rows handed in from the host (the event pair spans the two
   kernels only): its device time and that time as bytes of H per second, for the three row modes.
2. ``ElementwiseMaxEnt.default_model_scan`` on a synthetic 16 x 16 job: the solve (``kernel_ms``), the reduction where the
   rows lie (``reduce_ms``), one more ``mxe_logdet`` over the last launch (wall clock), the whole call (wall clock).
One JSON line each."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maxent_amd as mx
from maxent_amd import device, model_scan, synthetic


def reduce_alone(n_elem=256, n_mod=8, n_alpha=100, n_omega=500, repeat=5):
    rng = np.random.RandomState(0)
    ns = n_elem * n_mod
    n_s = 4
    ctx = device.DeviceContext(rng.randn(6, n_s), np.linspace(1.0, 0.1, n_s), np.linalg.qr(rng.randn(n_omega, n_s))[0])
    H = rng.rand(ns, n_alpha, n_omega) + 0.5
    logp = -60.0 - 30.0 * rng.rand(ns, n_alpha)
    lq = model_scan.log_measure(np.logspace(3, -2, n_alpha))
    off = np.arange(n_elem + 1) * n_mod
    pick = rng.randint(0, n_alpha, size=ns)
    for mode in (0, 1, 2):
        ms = []
        for _ in range(repeat):
            t = {}
            ctx.evidence_reduce(off, logp, lq, H=H, row_mode=mode, pick=pick if mode == 2 else None, want=('mean', 'between'), timing=t)
            ms.append(t['ms'])
        ms = sorted(ms)[len(ms) // 2]
        read = H.nbytes if mode == 0 else ns * n_omega * 8
        print(json.dumps(dict(what='mxe_evidence_reduce alone', row_mode=mode, scans=ns, n_alpha=n_alpha, n_omega=n_omega,
                              median_ms=round(ms, 4), H_bytes_read=read, TB_per_s=round(read / ms / 1e9, 3))))
    ctx.close()


def whole_scan(n_orb=16, n_tau=60, n_mod=8, n_alpha=100, n_omega=500):
    tau, omega, K, Gmat, _ = synthetic.matrix_G(n_orb, n_tau, n_omega)
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.set_error(synthetic.SIGMA)
    ew.alpha_mesh = synthetic.alpha_mesh(n_alpha)
    models = [mx.GaussianDefaultModel(omega, 0.0, w) for w in np.linspace(1.0, 4.5, n_mod)]
    for attempt in range(2):                    # (the second call: contexts and code objects are there)
        t0 = time.perf_counter()
        out = ew.default_model_scan(models, keep_models=False)
        wall = (time.perf_counter() - t0) * 1e3
    info = out['info']
    from maxent_amd.batch_solver import BatchSolver
    ctx = BatchSolver._pooled[0].ctxs[0] if BatchSolver._pooled else None           # (the solver of the last phase)
    logdet_ms = None
    if ctx is not None:
        t0 = time.perf_counter()
        ctx.logdet()
        logdet_ms = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps(dict(what='ElementwiseMaxEnt.default_model_scan', elements=n_orb * n_orb, models=n_mod, n_alpha=n_alpha,
                          n_omega=n_omega, n_tau=n_tau, solve_kernel_ms=round(info['kernel_ms'], 3),
                          reduce_ms=round(info['reduce_ms'], 3), launches=info['launches'], reduce_launches=info['reduce_launches'],
                          logdet_wall_ms_last_phase=logdet_ms, whole_call_wall_ms=round(wall, 1),
                          weights_00=np.round(out['weight'][0, 0], 3).tolist())))


if __name__ == '__main__':
    reduce_alone()
    if len(sys.argv) < 2 or sys.argv[1] != 'reduce':
        whole_scan()
