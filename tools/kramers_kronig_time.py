"""Times the device Kramers-Kronig transform (mxe_kramers_kronig) in two cases:

  (a) the self-energy guide's call (doc/guide/sigma_continuator.rst: np_interp_A=10000, np_omega=4000, 6 blocks):
      6 spectra, 10 000 -> 4 000 points
  (b) every alpha of the BASELINE batch (256 elements x 100 alphas): 25 600 spectra, 500 -> 2 000 points

For each: the device time of the sums (``out_ms``: the kernels between two events, no copies) and the end-to-end
time of ``maxent_amd.kramers_kronig`` (host clock: allocation, both copies and the kernels), median of --reps calls
after one warm-up call.  --numpy also times the numpy restatement of case (a) on the host, once.

    python tools/kramers_kronig_time.py [--reps 5] [--numpy] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maxent_amd import device                # noqa: E402

CASES = {'a': (6, 10000, 4000), 'b': (25600, 500, 2000)}
PEAK_F64 = 78.6e12                           # f64 vector (= matrix) peak of the MI355X, flop/s


def kk_numpy(A, w, w_out):
    j = np.arange(len(w))
    D = (w[np.minimum(j + 1, len(w) - 1)] - w[np.maximum(j - 1, 0)]) * 0.5
    C = D[None, :] / (w_out[:, None] - w[None, :] + 1j * D[None, :])
    return A @ C.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--numpy', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if device.device_count() < 1:
        raise SystemExit('no HIP device visible: nothing to time')
    out = {}
    for name, (n_spec, n_w, n_out) in CASES.items():
        rng = np.random.RandomState(1)
        w = np.linspace(-10.0, 10.0, n_w)
        w_out = np.linspace(-1.0, 1.0, n_out) if name == 'a' else np.linspace(-10.0, 10.0, n_out)
        A = rng.rand(n_spec, n_w)
        j = np.arange(n_w)
        wt = (w[np.minimum(j + 1, n_w - 1)] - w[np.maximum(j - 1, 0)]) * 0.5
        device.kramers_kronig(w, wt, wt, w_out, A)                 # warm-up: code object, allocator
        kern, e2e = [], []
        for _ in range(args.reps):
            t = {}
            t0 = time.perf_counter()
            G = device.kramers_kronig(w, wt, wt, w_out, A, timing=t)
            e2e.append((time.perf_counter() - t0) * 1e3)
            kern.append(t['ms'])
        # the FMAs alone: 2 per (spectrum, output, input) pair, 2 flops each
        flop = 4.0 * n_spec * n_out * n_w
        r = dict(n_spec=n_spec, n_w=n_w, n_out=n_out, launches=t['launches'],
                 kernel_ms=float(np.median(kern)), kernel_ms_all=kern,
                 end_to_end_ms=float(np.median(e2e)), end_to_end_ms_all=e2e,
                 result_MB=G.nbytes / 1e6, fma_floor_ms=flop / PEAK_F64 * 1e3,
                 fma_share_of_peak=flop / PEAK_F64 * 1e3 / float(np.median(kern)))
        if args.numpy and name == 'a':
            t0 = time.perf_counter()
            Gn = kk_numpy(A, w, w_out)
            r['numpy_ms'] = (time.perf_counter() - t0) * 1e3
            r['max_rel_diff_vs_numpy'] = float(np.abs(Gn - G).max() / np.abs(Gn).max())
        out[name] = r
        print('case (%s) %6d spectra, %5d -> %4d points: kernel %.3f ms, end to end %.2f ms (%d launch(es), %.0f MB '
              'result; FMA floor %.3f ms = %.0f%% of the kernel)%s'
              % (name, n_spec, n_w, n_out, r['kernel_ms'], r['end_to_end_ms'], r['launches'], r['result_MB'],
                 r['fma_floor_ms'], 100 * r['fma_share_of_peak'],
                 ', numpy %.0f ms' % r['numpy_ms'] if 'numpy_ms' in r else ''), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
