"""The deal plan of the wander sort (ssrs_amd/csrc/track_plan.h) on a CPU: the slots per list, the deal
k_deal_sorted makes and the host's bound on the longest list after it agree over a sweep of batch sizes,
windows in use, run shapes, block widths and both deals (tests/track_plan_driver.cpp)."""
import os
import re
import subprocess

from ssrs_amd.csrc import build

DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'track_plan_driver.cpp')


def test_deal_plan_fits_the_lists_and_the_hosts_bound(tmp_path):
    exe = str(tmp_path / 'track_plan_driver')
    subprocess.run([build.hipcc(), '-std=c++17', '-O2', '-Wall', '-Werror', DRIVER, '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r'(\d+) cases, 0 failures', out.stdout)
    assert m and int(m.group(1)) > 50000, out.stdout
