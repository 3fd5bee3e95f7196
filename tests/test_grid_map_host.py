"""csrc/grid_map.h on the CPU: the XCD-contiguous workgroup remap that fifteen kernels apply to blockIdx.x.  Compiles
tests/grid_map_host.cpp (a stand-alone program that includes the header) with the system C++ compiler, or hipcc where there is none, and
runs it for every grid size from 1 to 4096 and for 8 k - 1, 8 k, 8 k + 1 around large k up to the grids of the headline workload (100
samples of L = 352: 193 600 blocks of 64 pair rows, 580 800 tiles of the 768-wide projection; 2^20 and 1.2 M beyond them): the map is a
permutation, every XCD's blocks take one contiguous range, the ranges are ordered by XCD and their sizes differ by at most one.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE_K = [513, 24200, 72600, 131072, 150000]


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    src = os.path.join(ROOT, 'tests', 'grid_map_host.cpp')
    exe = str(tmp_path_factory.mktemp('grid_map') / 'grid_map_host')
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


@pytest.mark.parametrize('sizes', [['1-4096'], [f'{8 * k - 1}-{8 * k + 1}' for k in LARGE_K]], ids=['1..4096', 'large'])
def test_remap_is_a_permutation_with_one_ordered_range_per_xcd(prog, sizes):
    r = subprocess.run([prog] + sizes, capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    n = 4096 if sizes == ['1-4096'] else 3 * len(LARGE_K)
    assert f'{n} grid sizes, 0 failures' in r.stdout
