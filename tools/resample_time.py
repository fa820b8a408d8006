#!/usr/bin/env python3
"""Time ``ElementwiseMaxEnt.resample_errors`` on the job of tools/bins_prep_time.py (M x M elements, ``--n-bins`` bins of
``--n-tau`` imaginary times) with a jackknife of ``--block`` bins per block, against what a user does without it: a
Python loop over the resamples, each ``set_G_tau_data(mean_r)`` + ``set_cov(C)`` + ``run()`` on the same object.

    python tools/resample_time.py [--m 16] [--n-bins 1024] [--n-tau 200] [--block 64] [--runs 3] [--loop-resamples 17] [--kernel-only]

Both warm, in this process.  ``--loop-resamples``: how many resamples of the loop are timed (0: no loop; fewer than all: scaled).
``--kernel-only``: one warm-up and one call of ``resample_errors`` and nothing else (for a kernel trace).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maxent_amd as mx                     # noqa: E402
from maxent_amd import resampling           # noqa: E402
from bins_prep_time import make_bins        # noqa: E402


def fresh():
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    return ew


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', type=int, default=16)
    ap.add_argument('--n-bins', type=int, default=1024)
    ap.add_argument('--n-tau', type=int, default=200)
    ap.add_argument('--block', type=int, default=64)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loop-resamples', type=int, default=17)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    tau, bins = make_bins(a.m, a.n_bins, a.n_tau)
    ew = fresh()
    ew.set_G_tau_bins(tau, bins)
    windows = [(-2.0, 0.0), (0.0, 2.0)]
    out = ew.resample_errors(bins, block=a.block, windows=windows)             # warm-up
    if a.kernel_only:
        t0 = time.perf_counter()
        out = ew.resample_errors(bins, block=a.block, windows=windows)
        print(json.dumps(dict(resample_errors_s=time.perf_counter() - t0, info={k: v for k, v in out['info'].items() if k != 'left_out'})))
        return
    wall, infos = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        out = ew.resample_errors(bins, block=a.block, windows=windows)
        wall.append(time.perf_counter() - t0)
        infos.append(out['info'])
    n_res = out['n_resamples']
    n_alpha = len(np.asarray(ew.maxent_diagonal.alpha_mesh))
    res = dict(elements=a.m * a.m, n_bins=a.n_bins, n_tau=a.n_tau, block=a.block, n_resamples=n_res,
               scans=a.m * a.m * (n_res + 1), n_alpha=n_alpha, runs=a.runs,
               resample_errors_s=statistics.median(wall), resample_errors_min_s=min(wall), resample_errors_max_s=max(wall),
               solve_kernel_ms=statistics.median(i['kernel_ms'] for i in infos),
               reduce_ms=statistics.median(i['reduce_ms'] for i in infos),
               bins_resample_ms=statistics.median(i['resample_ms'] for i in infos),
               launches=infos[-1]['launches'], reduce_launches=infos[-1]['reduce_launches'],
               n_datasets=infos[-1]['n_datasets'], n_used_min=int(np.nanmin(out['n_used'])),
               threads=os.environ.get('OMP_NUM_THREADS'))
    if a.loop_resamples > 0:
        # the loop a user writes today: the covariance of the full sample once, then per resample mean -> set_cov -> run
        counts = resampling.resample_counts('jackknife', a.n_bins, block=a.block)
        k = min(a.loop_resamples, len(counts))
        t0 = time.perf_counter()
        mean = bins.mean(axis=0)
        X = (bins - mean).reshape(a.n_bins, a.m * a.m, a.n_tau)
        C = np.stack([X[:, e, :].T @ X[:, e, :] for e in range(a.m * a.m)]).reshape(a.m, a.m, a.n_tau, a.n_tau) / (a.n_bins * (a.n_bins - 1.0))
        t_cov = time.perf_counter() - t0
        eh = fresh()
        t0 = time.perf_counter()
        for r in range(k):
            w = counts[r] / float(counts[r].sum())
            eh.set_G_tau_data(tau, np.tensordot(w, bins, axes=(0, 0)))
            eh.set_cov(C)
            eh.run().A_out
        t_loop = time.perf_counter() - t0
        res.update(loop_resamples_timed=k, loop_cov_s=t_cov, loop_s=t_loop * len(counts) / float(k) + t_cov,
                   speedup=(t_loop * len(counts) / float(k) + t_cov) / statistics.median(wall))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
