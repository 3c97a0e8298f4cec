"""copy_run16, the row copy of launch_copy and of the bare items of k_window_mix, as host code under AddressSanitizer
(tools/copy_run_host_check.py builds a stand-alone program from the header's own text): no byte outside a window row is
read, none outside a destination row written, at every alignment and row length around the 16-byte run."""
import os
import subprocess
import sys

from conftest import ROOT


def test_copy_run16_stays_inside_its_rows():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "copy_run_host_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "4480 cases" in r.stdout, r.stdout
