#!/usr/bin/env python3
"""Time the preparation of an element-wise job from Monte Carlo bins: the device path (``set_G_tau_bins`` up to the
first launch: mean and covariance eigenbasis of every element from one ``mxe_bins_eig`` call) against the host path
(mean and np.cov-style covariance of every element, then ``TauMaxEnt.set_cov`` -- ``np.linalg.eigh`` -- per element).

    python tools/bins_prep_time.py [--m 16] [--n-bins 1024] [--n-tau 200] [--runs 5] [--host-elements 8] [--kernel-only]

Both are timed warm, in this process, as the median of ``--runs`` runs after one warm-up.  The host path is timed on
``--host-elements`` elements and scaled to all M x M (it is a loop over elements, each the same work; 0: all of
them, 256 x 0.7 s per run at the default size).  ``library_call_s``: ``device.bins_eig`` alone on stacked bins.  Prints one JSON
line.  ``--kernel-only``: one warm-up and one timed call of the device path and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maxent_amd as mx                     # noqa: E402
from maxent_amd import device               # noqa: E402


def make_bins(M, n_bins, n_tau, seed=7):
    rng = np.random.RandomState(seed)
    tau = np.linspace(0.0, 40.0, n_tau)
    G = -0.5 * (np.exp(-tau) + np.exp(-(40.0 - tau)))
    z = rng.randn(n_bins, M, M, n_tau)
    for t in range(1, n_tau):                  # AR(1) along tau, amplitude decaying
        z[..., t] = 0.5 * z[..., t - 1] + np.sqrt(0.75) * z[..., t]
    return tau, G[None, None, None, :] + 2e-3 * np.exp(-np.log(5.0) * np.arange(n_tau) / (n_tau - 1)) * z


def device_prep(tau, bins):
    ew = mx.ElementwiseMaxEnt(use_hermiticity=False)
    ew.set_verbosity(mx.VerbosityFlags.Quiet)
    t0 = time.perf_counter()
    ew.set_G_tau_bins(tau, bins)
    return time.perf_counter() - t0, ew


def host_prep(tau, bins, elements):
    """what a user does today, per element: mean, covariance of the mean (one matrix product), set_cov (eigh)"""
    n_bins = bins.shape[0]
    t_cov = t_eig = 0.0
    for (i, j) in elements:
        tm = mx.TauMaxEnt()
        tm.set_verbosity(mx.VerbosityFlags.Quiet)
        t0 = time.perf_counter()
        b = bins[:, i, j, :]
        mean = b.mean(axis=0)
        X = b - mean
        C = X.T @ X / (n_bins * (n_bins - 1.0))
        t1 = time.perf_counter()
        tm.set_G_tau_data(tau, mean)
        tm.set_cov(C)
        t2 = time.perf_counter()
        t_cov += t1 - t0
        t_eig += t2 - t1
    return t_cov, t_eig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', type=int, default=16)
    ap.add_argument('--n-bins', type=int, default=1024)
    ap.add_argument('--n-tau', type=int, default=200)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--host-elements', type=int, default=8)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    tau, bins = make_bins(a.m, a.n_bins, a.n_tau)
    device_prep(tau, bins)                                            # warm-up (code object load, first allocations)
    if a.kernel_only:
        t, ew = device_prep(tau, bins)
        sw = [st['sweeps'] for st in ew.bin_statistics.values()]
        print(json.dumps(dict(device_prep_s=t, sweeps_min=min(sw), sweeps_max=max(sw))))
        return
    dev, sweeps, ranks = [], None, None
    for _ in range(a.runs):
        t, ew = device_prep(tau, bins)
        dev.append(t)
        sweeps = [st['sweeps'] for st in ew.bin_statistics.values()]
        ranks = [st['rank'] for st in ew.bin_statistics.values()]
    # the library call alone, on bins that are stacked already: finiteness pass, copy to the device, kernel, copy back
    stack = np.ascontiguousarray(bins.transpose(1, 2, 0, 3).reshape(a.m * a.m, a.n_bins, a.n_tau))
    call = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        device.bins_eig(stack, 1e-14)
        call.append(time.perf_counter() - t0)
    del stack
    n_host = a.m * a.m if a.host_elements <= 0 else min(a.host_elements, a.m * a.m)
    elements = [(k % a.m, (k // a.m) % a.m) for k in range(n_host)]
    host_prep(tau, bins, elements[:1])                                # warm-up
    host = []
    for _ in range(a.runs):
        t_cov, t_eig = host_prep(tau, bins, elements)
        host.append((t_cov + t_eig, t_cov, t_eig))
    scale = a.m * a.m / float(len(elements))
    h = sorted(host)[len(host) // 2]
    print(json.dumps(dict(
        elements=a.m * a.m, n_bins=a.n_bins, n_tau=a.n_tau, runs=a.runs,
        device_prep_s=statistics.median(dev), device_prep_min_s=min(dev), device_prep_max_s=max(dev),
        library_call_s=statistics.median(call),
        host_prep_s=h[0] * scale, host_cov_s=h[1] * scale, host_set_cov_s=h[2] * scale,
        host_elements_timed=len(elements), speedup=h[0] * scale / statistics.median(dev),
        sweeps_min=min(sweeps), sweeps_max=max(sweeps), rank_min=min(ranks), rank_max=max(ranks),
        threads=os.environ.get('OMP_NUM_THREADS'))))


if __name__ == '__main__':
    main()
