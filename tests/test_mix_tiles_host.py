"""The order in which the symmetric mixing-matrix product visits its block tiles (csrc/hx_mix_tiles.h): a host function,
pinned by a host program.  No GPU."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mix_tiles_host(tmp_path):
    exe = tmp_path / "t_mix_tiles"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "csrc", "test_mix_tiles.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
