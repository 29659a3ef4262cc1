"""The launch arithmetic of the GEMM kernels (csrc/launch_geometry.hpp: grids, XCD padding, the slicing of the weight-gradient GEMMs'
rows over their slab) under AddressSanitizer and UBSan.  The header is plain C++, free of HIP, so the rules that decide a weight
gradient's summation order are swept on the CPU (tests/native/launch_geometry_driver.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_launch_geometry_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'launch_geometry')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
           os.path.join(ROOT, 'tests', 'native', 'launch_geometry_driver.cpp')]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'geometry ok' in r.stdout
