"""The kernel choice (csrc/rtw_variants.h: the table of shipped instantiations and the selectors that pick a row for a scene, a
generator and a pass) checked on the CPU by tests/native/variants_check.cpp. A scene sent to the wrong instantiation of k_path is a
wrong image, not an error, so every combination of the selectors' inputs is compared with the rules written out a second time, every
row must be chosen by some input, and no input may choose a row the kernel refuses to compile. The program's `row` mode names the row
of a scene blob: tests/test_gpu_variants.py asserts with it which row each of its cases runs."""
import os
import subprocess

import pytest

from raytracing_weekend_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(directory):
    path = os.path.join(str(directory), "variants_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", path,
                           os.path.join(ROOT, "tests", "native", "variants_check.cpp")])
    return path


def run(exe, args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("RTW_")}
    e.update(env or {})
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=e)
    print(out.stdout, out.stderr[-3000:])
    return out


def row_of(exe, blob_path, rng_kind, estimator, list_pass, width, height, max_depth, env=None):
    """{'pipeline': ..., 'k_path': ..., 'k_first': ...} of a scene blob in a file"""
    out = run(exe, ["row", blob_path, rng_kind, estimator, int(list_pass), width, height, max_depth], env)
    assert out.returncode == 0, out.stderr[-3000:]
    return dict(kv.split("=") for kv in out.stdout.split())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory.mktemp("variants"))


def test_every_input_chooses_the_row_the_rules_give_and_every_row_is_chosen(exe):
    out = run(exe, ["rules"])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "rows k_path 20 k_first 12 k_shade 6 k_bounce 6 k_classify 2 k_trace 2 k_trace_bvh 9, each chosen" in out.stdout
    assert "rules: 24192 k_path inputs" in out.stdout  # 2 generators x 3 levels x 2 x 4 estimators x 3 x 6 x 7 generators x 2 shapes x 2


def test_rows_of_scene_blobs(exe, tmp_path):
    f = tmp_path / "cornell.blob"
    f.write_bytes(abi.build_scene(0, 64, 64))
    ref, mix = 0, 3  # include/rtw.h rtw_estimator
    assert row_of(exe, f, abi.RTW_RNG_PHILOX, ref, False, 64, 64, 6) == {"pipeline": "path", "k_path": "PATH_PHILOX_BOX", "k_first": "FIRST_PHILOX_HOT"}
    assert row_of(exe, f, abi.RTW_RNG_PHILOX, ref, True, 64, 64, 6)["k_path"] == "PATH_LIST_PHILOX_BOX"
    assert row_of(exe, f, abi.RTW_RNG_TEA_LCG, ref, False, 64, 64, 6)["k_path"] == "PATH_TEA_HOT"
    assert row_of(exe, f, abi.RTW_RNG_PHILOX, mix, False, 64, 64, 6)["k_path"] == "PATH_PHILOX_MIX"
    assert row_of(exe, f, abi.RTW_RNG_PHILOX, ref, False, 64, 64, 0)["pipeline"] == "wavefront"
    assert row_of(exe, f, abi.RTW_RNG_PHILOX, ref, False, 64, 64, 6, env={"RTW_PATH": "0"})["pipeline"] == "wavefront"
    # through the tree the box has no list shape: the one-light row that reads the headers (were k_path to run it)
    assert row_of(exe, f, abi.RTW_RNG_PHILOX, ref, False, 64, 64, 6, env={"RTW_BRUTE_MAX": "0"}) == {
        "pipeline": "wavefront", "k_path": "PATH_PHILOX_ONE", "k_first": "FIRST_PHILOX_HOT"}
