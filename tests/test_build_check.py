"""Build-time guarantees of the shipped kernels: no instantiation spills registers beyond the one documented
allowance (``make -C maxent_amd/csrc check``: hipcc's own resource report)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'), reason='no hipcc')
def test_no_shipped_kernel_spills():
    r = subprocess.run(['make', '--no-print-directory', '-C', os.path.join(ROOT, 'maxent_amd', 'csrc'), 'check'],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    # (only the report lines of the check: other output -- a path, say -- may contain the word too)
    found = [(l, re.search(r' scratch +(\d+) B occupancy ', l)) for l in r.stdout.splitlines()]
    report = [(l, int(m.group(1))) for l, m in found if m]
    lines = [l for l, _ in report]
    assert len(lines) >= 20
    for l, scratch in report:
        assert scratch == 0 or ('chain_kernel_mcILi32ELi2' in l and scratch <= 200) or \
            ('chain_kernel_mcILi32ELi1' in l and 'ELi8EE' in l and scratch <= 64) or \
            ('chain_kernel_mcILi64ELi1' in l and scratch <= 192) or \
            ('chain_kernelILi1ELi4EdLb1' in l and scratch <= 32) or \
            ('chain_kernel_lv' in l and scratch <= 16), l            # (the allowances of the Makefile, documented there)
    assert not any('chain_kernel_mcILi48' in l or 'chain_kernelILi8' in l for l in lines)
