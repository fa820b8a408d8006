#!/usr/bin/env python3
"""Where a launch of linefit_kernel spends its time, from the in-kernel stamp build.

    make -C maxent_amd/csrc prof
    MAXENT_AMD_LIB=maxent_amd/lib/libmaxent_hip_prof.so python tools/profile_linefit.py [--n-orb 16] [--n-alpha 100]

Stages the benchmark's batch (cfg4 by default), launches it once and then mxe_select_launch and mxe_select3_launch, each a
few times; prints for the last launch of each the time lane 0 of every wave reached each stamp, as the median over the
workgroups, in cycles of the shader clock since the workgroup's entry.  Reads SHARES and the order of the waves, not run time
(the stamped build is slower than the shipped one, which executes no stamp).
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('MAXENT_AMD_LIB', os.path.join(ROOT, 'maxent_amd', 'lib', 'libmaxent_hip_prof.so'))
import bench                      # noqa: E402
from maxent_amd import device     # noqa: E402

STAMPS = ['entry', 'logarithms | barrier', 'running sums | barrier', 'ranking | barrier', 'candidate fits (+ analyzers)',
          'barrier', 'pick', 'rows copied']

ap = argparse.ArgumentParser()
ap.add_argument('--n-orb', type=int, default=16)
ap.add_argument('--n-omega', type=int, default=500)
ap.add_argument('--n-alpha', type=int, default=100)
ap.add_argument('--repeat', type=int, default=5)
args = ap.parse_args()
batch = bench.build_batch(args.n_orb, 200, args.n_omega, args.n_alpha, 0)
ctx = bench.stage(batch, 0)
n_chain = len(batch['elems'])
ctx.upload_chains(np.arange(n_chain, dtype=np.int32), batch['alphas'], batch['v0'])
ctx.launch()
ctx.sync()
lib = device.load_library()
lib.mxe_prof_linefit_fetch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
print('library %s' % os.environ['MAXENT_AMD_LIB'])
print('%d scans x %d alphas, rows of %d; cycles since entry, median over the workgroups (lane 0 of each wave)' %
      (n_chain, args.n_alpha, args.n_omega))
for name, launch in (('mxe_select_launch(0)', lambda: ctx.select_launch(0)),
                     ('mxe_select3_launch(0, 0.2)', lambda: ctx.select3_launch(0, 0.2))):
    for _ in range(args.repeat):
        launch()
        ctx.sync()
    prof = np.zeros((n_chain, 4, 10), dtype=np.int64)
    rc = lib.mxe_prof_linefit_fetch(ctx._h, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    assert rc == 0, rc
    t = prof[:, :, :8] - prof[:, :1, :1]                   # since wave 0 entered
    med = np.median(t, axis=0)
    wall = (prof[:, :, 9].max(axis=1) - prof[:, :, 8].min(axis=1)) * 0.01        # 100 MHz clock -> us
    span = (prof[:, :, 9].max() - prof[:, :, 8].min()) * 0.01
    print('\n%s' % name)
    print('  %-30s' % 'stamp' + ''.join('    wave%d' % w for w in range(4)) + '   step (slowest wave)')
    prev = 0.0
    for s in range(8):
        worst = med[:, s].max()
        print('  %-30s' % STAMPS[s] + ''.join(' %8.0f' % med[w, s] for w in range(4)) + '   %8.0f' % (worst - prev))
        prev = worst
    print('  workgroup entry to exit: median %.2f us, max %.2f us; first entry to last exit of the grid %.2f us' %
          (np.median(wall), wall.max(), span))
ctx.close()
