"""gj2_solve64_f32 with the packed trailing update (two columns per v_pk_fma_f32, the multiplier in both halves) against the
scalar form of the same function: tools/split_check.hip, a stand-alone HIP program, runs both for N = 16, 20, 24, 28, 32 -- an
odd and an even number of remaining columns occur at some step of each -- on random positive definite systems scaled to a
unit diagonal.  Each half of a packed multiply-add is the multiply-add it replaces, so z agrees bit for bit."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.fixture(scope='module')
def figures(tmp_path_factory):
    if HIPCC is None:
        pytest.skip('no hipcc')
    exe = str(tmp_path_factory.mktemp('split_check') / 'split_check')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', os.path.join(ROOT, 'tools', 'split_check.hip'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        m = re.match(r'(\w+) (\S+)$', line)
        if m:
            out[m.group(1)] = float(m.group(2))
    return out


@pytest.mark.parametrize('n', [16, 20, 24, 28, 32])
def test_packed_trailing_update_gives_the_same_bits(figures, n):
    f = figures
    assert f['solve_values_per_size'] >= 1024
    assert f['solve_%d_mismatches' % n] == 0
    assert f['solve_%d_residual' % n] < 1e-4          # (and it is a solution: binary32, condition ~1e3)
