"""CPU suite of the owner of device allocations (raytracing_weekend_amd/csrc/rtw_devbuf.h DevBuf): the header under the sanitizers, over
counting stand-ins for the three runtime functions it calls (tests/native/devbuf_check.cpp). No HIP library is linked."""
import os
import subprocess

from raytracing_weekend_amd import abi

ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # for hip/hip_runtime_api.h: declarations only


def test_devbuf_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "devbuf_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-o", exe,
                           os.path.join(abi.REPO_DIR, "tests", "native", "devbuf_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "devbuf_check ok" in out.stdout, out.stdout + out.stderr[-2000:]
