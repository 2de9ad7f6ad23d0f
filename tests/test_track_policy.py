"""The stepper's per-batch policy (ssrs_amd/csrc/track_policy.h) on a CPU, fed with read-back slots as the host loop
feeds them: a periodic shuffle of a settled batch asks for no window scan, real sorts do, stable_roam and since_shuffle
space the shuffles and keep the launches long, and deal_upper still bounds the lists (tests/track_policy_driver.cpp)."""
import os
import re
import subprocess

from ssrs_amd.csrc import build

DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'track_policy_driver.cpp')


def test_periodic_shuffles_reuse_the_windows_and_the_bound_holds(tmp_path):
    exe = str(tmp_path / 'track_policy_driver')
    subprocess.run([build.hipcc(), '-std=c++17', '-O2', '-Wall', '-Werror', DRIVER, '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r'(\d+) scenarios, (\d+) checks, 0 failures', out.stdout)
    assert m and int(m.group(1)) == 19 and int(m.group(2)) > 1000, out.stdout
