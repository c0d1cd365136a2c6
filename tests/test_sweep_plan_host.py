"""How the maps of one hx_map2alm_multi / hx_map2alm_list call are cut into sweeps (csrc/hx_sweep_plan.h): a host function,
pinned by a host program.  No GPU."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_plan_host(tmp_path):
    exe = tmp_path / "t_sweep_plan"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "csrc", "test_sweep_plan.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
