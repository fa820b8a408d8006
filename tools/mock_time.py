"""Times of a parametric bootstrap at the size of DESIGN.md 4w: 16 x 16 elements x 200 mocks x 200 tau x 500 omega points.

1. ``mxe_mock_data`` alone on 256 sets (the event pair spans the kernel only) and the wall clock of the whole call, which
   is the kernel plus the copies: the mock rows come back to the host and go down again as data of the scans.
2. ``mxe_resample_quantiles`` alone on 256 groups of 200 synthetic rows handed in from the host: its device time and that
   time as bytes of H per second, beside ``mxe_resample_reduce`` on the same rows.
3. ``ElementwiseMaxEnt.parametric_bootstrap`` on a synthetic job (``whole``: n_orb, n_mock, n_alpha from the command line).
One JSON line each."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maxent_amd as mx
from maxent_amd import device, synthetic


def median(ms):
    return sorted(ms)[len(ms) // 2]


def mock_alone(n_sets=256, n_mock=200, n_tau=200, n_omega=500, repeat=5):
    tau, omega = synthetic.grids(n_tau, n_omega)
    K = np.ascontiguousarray(mx.TauKernel(tau=tau, omega=omega, beta=synthetic.BETA).K)
    rng = np.random.RandomState(0)
    H0 = rng.rand(n_sets, n_omega) / n_omega
    err = np.full((n_sets, n_tau), synthetic.SIGMA)
    ms, wall = [], []
    for _ in range(repeat):
        t = {}
        t0 = time.perf_counter()
        got = device.mock_data(K, H0, err, 1, np.arange(n_sets), n_mock, timing=t)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(t['ms'])
    print(json.dumps(dict(what='mxe_mock_data alone', sets=n_sets, n_mock=n_mock, n_tau=n_tau, n_omega=n_omega,
                          kernel_median_ms=round(median(ms), 4), call_wall_median_ms=round(median(wall), 2),
                          mock_rows_bytes=int(got['G'].nbytes))))


def quantiles_alone(n_groups=256, n_rows=200, n_omega=500, repeat=5):
    rng = np.random.RandomState(0)
    n_s = 4
    ctx = device.DeviceContext(rng.randn(6, n_s), np.linspace(1.0, 0.1, n_s), np.linalg.qr(rng.randn(n_omega, n_s))[0])
    H = rng.rand(n_groups * n_rows, n_omega) + 0.5
    off = np.arange(n_groups + 1) * n_rows
    mq, mr = [], []
    for _ in range(repeat):
        t = {}
        ctx.resample_quantiles(off, (0.16, 0.5, 0.84), H=H, timing=t)
        mq.append(t['ms'])
        ctx.resample_reduce(off, np.ones(n_groups), H=H, want=('mean', 'var'), timing=t)
        mr.append(t['ms'])
    ctx.close()
    print(json.dumps(dict(what='mxe_resample_quantiles alone', groups=n_groups, rows_per_group=n_rows, n_omega=n_omega,
                          quantiles_median_ms=round(median(mq), 4), TB_per_s=round(2 * H.nbytes / median(mq) / 1e9, 3),
                          reduce_median_ms=round(median(mr), 4), H_bytes=int(H.nbytes))))


def whole(n_orb=16, n_mock=200, n_alpha=20, n_tau=200, n_omega=500):
    tau, omega, K, Gmat, _ = synthetic.matrix_G(n_orb, n_tau, n_omega)
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    ew.set_G_tau_data(tau, Gmat)
    ew.omega = omega
    ew.set_error(synthetic.SIGMA)
    ew.alpha_mesh = synthetic.alpha_mesh(n_alpha)
    res = ew.run()
    t0 = time.perf_counter()
    out = ew.parametric_bootstrap(res, n_mock=n_mock, seed=1)
    wall = (time.perf_counter() - t0) * 1e3
    info = out['info']
    print(json.dumps(dict(what='ElementwiseMaxEnt.parametric_bootstrap', elements=n_orb * n_orb, n_mock=n_mock, n_alpha=n_alpha,
                          n_tau=n_tau, n_omega=n_omega, solve_kernel_ms=round(info['kernel_ms'], 3),
                          reduce_ms=round(info['reduce_ms'], 3), mock_ms=round(info['mock_ms'], 4), mock_bytes=info['mock_bytes'],
                          launches=info['launches'], reduce_launches=info['reduce_launches'], whole_call_wall_ms=round(wall, 1),
                          n_used_min=int(np.min(out['n_used'])), p_value_00=float(out['chi2_p_value'][0, 0]))))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'alone'
    if what == 'alone':
        mock_alone()
        quantiles_alone()
    else:
        whole(*[int(a) for a in sys.argv[2:]])
