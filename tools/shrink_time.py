#!/usr/bin/env python3
"""Time the shrinkage covariance of Monte Carlo bins: ``mxe_bins_eig_shrunk`` with the intensity
estimated, ``mxe_bins_eig`` on the same bins (the path without shrinkage: the yardstick), and numpy on the host.

    python tools/shrink_time.py [--runs 5] [--cases 1x1000x200,1x1000x512,256x130x65]

Per case one JSON line.  ``shrunk_ms``: device time of all kernels of the call (events around them), the smallest of
``--runs`` warm calls.  ``shrunk_call_s`` / ``plain_call_s``: wall time of the whole library call (finiteness pass,
copies, kernels), the smallest of the runs -- ``mxe_bins_eig`` has no device timer, the two calls compare here.
``numpy_f64_s``: the intensity by the same two Gram products in binary64 numpy; ``numpy_longdouble_s``: the reference of
the tests (tests/shrinkage_ref.py), timed on one set and scaled to all.  The intensity kernels take well under 1 % of
the call: their own times come from a kernel trace of this script (``rocprofv3 --kernel-trace --stats -- python
tools/shrink_time.py --cases ...``: shrink_prep_kernel, shrink_gram_kernel, shrink_lambda_kernel), not from a difference
of two calls.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from maxent_amd import device               # noqa: E402
import shrinkage_ref                        # noqa: E402


def make_bins(n_sets, m, n, rho=0.9, seed=3):
    rng = np.random.RandomState(seed)
    e = rng.randn(n_sets, m, n)
    for j in range(1, n):
        e[..., j] = rho * e[..., j - 1] + np.sqrt(1.0 - rho * rho) * e[..., j]
    return (e + 0.3) * 10.0 ** (-1.5 * np.arange(n) / max(n - 1, 1))


def intensity_f64(b):
    m = b.shape[0]
    x = b - b.mean(axis=0)
    z = x / np.sqrt((x * x).sum(axis=0) / (m - 1))
    G1, G2 = z.T @ z, (z * z).T @ (z * z)
    off = ~np.eye(b.shape[1], dtype=bool)
    return m / (m - 1.0) * (G2 - G1 * G1 / m)[off].sum() / (G1 * G1)[off].sum()


def best(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0, r))
    return min(t for t, _ in out), out[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--cases', default='1x1000x200,1x1000x512,256x130x65')
    a = ap.parse_args()
    for case in a.cases.split(','):
        n_sets, m, n = (int(v) for v in case.split('x'))
        bins = make_bins(n_sets, m, n)
        device.bins_eig_shrunk(bins, 0.0, 'auto')                     # warm-up (code object load)
        device.bins_eig(bins, 0.0)
        ms_auto = []

        def auto():
            t = {}
            r = device.bins_eig_shrunk(bins, 0.0, 'auto', timing=t)
            ms_auto.append(t['ms'])
            return r
        shrunk_call, st = best(auto, a.runs)
        lam = float(np.mean([s['shrinkage'] for s in st]))
        plain_call, pl = best(lambda: device.bins_eig(bins, 0.0), a.runs)
        f64, raw = best(lambda: [intensity_f64(b) for b in bins], max(1, min(a.runs, 3)))
        ld, _ = best(lambda: shrinkage_ref.intensity(bins[0]), 1)
        print(json.dumps(dict(
            n_sets=n_sets, n_bins=m, n_data=n, runs=a.runs, shrunk_ms=min(ms_auto),
            shrunk_call_s=shrunk_call, plain_call_s=plain_call,
            numpy_f64_s=f64, numpy_longdouble_s=ld * n_sets, lambda_mean=lam,
            lambda_vs_numpy=float(np.max(np.abs(np.array([s['shrinkage_raw'] for s in st]) / np.array(raw) - 1.0))),
            rank_shrunk=int(min(s['rank'] for s in st)), rank_plain=int(min(s['rank'] for s in pl)),
            sweeps_shrunk=int(max(s['sweeps'] for s in st)), sweeps_plain=int(max(s['sweeps'] for s in pl)),
            threads=os.environ.get('OMP_NUM_THREADS'))), flush=True)


if __name__ == '__main__':
    main()
