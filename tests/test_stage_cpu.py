"""CPU suite of the staging slab that the host variants of the query family share (raytracing_weekend_amd/csrc/rtw_stage_plan.h): the
layout function under the sanitizers, over every family's section list."""
import os
import subprocess

from raytracing_weekend_amd import abi


def test_stage_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-o", exe, os.path.join(abi.REPO_DIR, "tests", "native", "stage_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "stage_plan_check ok" in out.stdout, out.stdout + out.stderr[-2000:]
