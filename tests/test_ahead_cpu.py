"""k_path's reserve of camera rays and its gated bounds test without a GPU: the integer bookkeeping of csrc/rtw_ahead.h, which the
kernel calls too, checked by tests/native/ahead_check.cpp - a simulated wave of 64 lanes over units of 1, 2, 4 and 8 blocks, sample
counts around the block size, K = 1, 2, 3. A stand-alone program, built plainly and with the address and undefined-behaviour
sanitizers, and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_native_ahead_check(tmp_path, kind):
    exe = str(tmp_path / "ahead_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[kind] +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "ahead_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ahead_check ok", r.stdout + r.stderr
