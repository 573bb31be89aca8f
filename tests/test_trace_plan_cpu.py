"""The backtrace planner and the LDS arithmetic it shares with the kernels (wfa-gpu_amd/csrc/trace_layout.h) are plain C++: compiled
here with the host compiler alone -- no HIP header -- and swept by tests/trace_plan_check.cpp (CPU-only test, not `-m gpu`)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trace_plans_fit_the_device_and_keep_their_mapping(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "trace_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "wfa-gpu_amd", "csrc"),
                            os.path.join(ROOT, "tests", "trace_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "trace_plan_check ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
