"""csrc/tri_row_touch.h on the CPU: the enumeration of the z lines the row-fused triangle attention touches per k-group, against the lines
its walk reads.  Compiles tests/tri_row_touch_host.cpp (a stand-alone program that includes the header) with the system C++ compiler, or
hipcc where there is none, and runs it for the row lengths at which something changes - one position, one short of / exactly / one past
the 32 positions of a wave, exactly one touch stride (64), ragged (97), one short of and exactly the longest row (351, 352) - and both
stride orders (starting node: positions contiguous, zl = 192; ending node: zl = L 192).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 31, 32, 33, 64, 97, 351, 352]


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    src = os.path.join(ROOT, 'tests', 'tri_row_touch_host.cpp')
    exe = str(tmp_path_factory.mktemp('tri_row_touch') / 'tri_row_touch_host')
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    inc = '-I' + os.path.join(ROOT, 'abx_amd', 'csrc')
    if cxx:
        cmd = [cxx, '-O1', '-std=c++17', '-Wall', inc, src, '-o', exe]
    else:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        cmd = [hipcc, '-x', 'c++', '-O1', '-std=c++17', '-Wall', inc, src, '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize('order', ['row', 'column'])
@pytest.mark.parametrize('L', LENGTHS)
def test_touch_lines_are_the_walk_lines(prog, L, order):
    zl = 192 if order == 'row' else L * 192
    r = subprocess.run([prog, str(L), str(zl)], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert f'{L * 6} lines touched, {L * 192} floats walked, 0 failures' in r.stdout
