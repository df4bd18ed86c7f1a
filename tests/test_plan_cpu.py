"""Launch planning (csrc/rtw_plan.h, host code) checked on the CPU by tests/native/plan_check.cpp: k_path's unit sizes, sum slots,
passes and launches, and the wavefront pipeline's batch size, lanes, trace workgroup and tail schedule for the headline frame,
BASELINE configs 3 and 5 and a few knobs (RTW_BLOCKSUM_BYTES, RTW_LANES, RTW_POOL_PATHS, RTW_FUSED)."""
import os
import subprocess


def test_plans(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(root, "tests", "native", "plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.count("path ") == 6 and out.stdout.count("wavefront ") == 4, out.stdout
