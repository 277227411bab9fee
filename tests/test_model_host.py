"""No GPU: the host-only logic of the dm_model runtime (deepmod_amd/csrc/modelplan.inc) - which DM_ERANGE word a launch writes and which marker or sync
reports it (include/deepmod_hip.h, at DM_MARKS), and the grid of a classifier launch.  tests/test_gpu_range_contract.py holds the same contract on the
device; here the bookkeeping runs alone, under the sanitizers."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_range_slots_and_launch_grid_under_address_sanitizer(tmp_path):
    """tests/modelplan_asan_driver.cpp, built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically: the three
    scripted marker sequences of tests/test_gpu_range_contract.py, three seeded random walks of 20,000 launches, markers, waits and syncs against a plain
    list of the poisoned launches not yet reported (each reported exactly once, never by a marker recorded before it, none left after a sync; the words in
    a heap block of exactly RANGE_SLOTS ints), and launch_grid on every item count up to 4 x cap + 3 for caps 1, 2, 128, 255, 256."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'modelplan_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-o', exe, os.path.join(ROOT, 'tests', 'modelplan_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'MODELPLAN-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
