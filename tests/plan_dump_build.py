"""The stand-alone build of tools/plan_dump.cpp that the host tests of the planners share (test_launch_plan_host.py,
test_finish_plan_host.py, test_kernel_build_host.py): the system compiler, with the address and undefined-behaviour sanitizers where it links them.
Built once per session, whichever file asks first."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = None


def plan_dump_binary(tmp_path_factory):
    global _built
    if _built is None:
        cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
        assert cxx, 'no C++ compiler'
        out = str(tmp_path_factory.mktemp('plan_dump') / 'plan_dump')
        base = [cxx, '-std=c++17', '-O1', '-g', os.path.join(ROOT, 'tools', 'plan_dump.cpp'), '-o', out]
        r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print('plan_dump: built WITHOUT sanitizers (%s)' % r.stdout.strip().splitlines()[-1:])
            subprocess.check_call(base)
        _built = out
    return _built


def run_plan_dump(binary, text, *args):
    r = subprocess.run([binary, *args], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout
