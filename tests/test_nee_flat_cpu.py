"""The straight-line light sample of k_path's one-light instantiation without a GPU: csrc/rtw_nee.h, which the kernel calls too,
beside a transcription of shade_a's nested form (tests/native/nee_flat_check.cpp, which lists the inputs: a million random vertices
around the Cornell box's light and every edge of the predicate singly and in pairs, on all three axes). `has` must be equal
everywhere and every output equal in bits where it holds; a control with one & of the predicate turned into | must be rejected. A
stand-alone program, built plainly and with the address and undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_native_nee_flat_check(tmp_path, kind):
    exe = str(tmp_path / "nee_flat_check")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + FLAGS[kind]
    if " fma " in open("/proc/cpuinfo").read():
        cmd.append("-mfma")  # fmaf as one instruction (same result as the library's, much faster)
    subprocess.check_call(cmd + ["-o", exe, os.path.join(ROOT, "tests", "native", "nee_flat_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("nee_flat_check ok"), r.stdout + r.stderr
