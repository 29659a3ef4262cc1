"""The host-side plan builder (csrc/plan.cpp) on long, forward-only plans (64 < L <= 128) under AddressSanitizer and UBSan: the
counterpart of test_plan_sanitizers.py, whose sweep stops at L = 64."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_long_plan_builder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'long_plan_asan')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
           os.path.join(ROOT, 'tests', 'native', 'long_plan_asan_driver.cpp'), os.path.join(ROOT, 'cliora_amd', 'csrc', 'plan.cpp')]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'long plans ok' in r.stdout
