"""The list-shape predicate (csrc/rtw_scene.h: walk_shape, stored by prepare_scene as SceneInfo::walk_shape) checked on the CPU by
tests/native/shape_check.cpp. k_path walks a scene with the code compiled for the Cornell box's lists exactly when this id says so,
and that code tests record i as the kind the shape gives it: an id given to any other group table would make every pixel wrong. So
scene 0 must get the id at every frame size, every other scene of tests/test_scene_cpu.py must not, and no edit of the Cornell
group table may."""
import os
import subprocess

import pytest

from raytracing_weekend_amd import abi
from test_scene_cpu import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = 1  # rtw_scene.h WALK_SHAPE_CORNELL


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("shape") / "shape_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", path,
                           os.path.join(ROOT, "tests", "native", "shape_check.cpp")])
    return path


def run(exe, args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("RTW_")}
    e.update(env or {})
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=e)
    print(out.stdout, out.stderr[-3000:])
    return out


def test_cornell_box_has_the_shape_at_every_frame_size(exe, tmp_path):
    args = ["scene"]
    for w, h in ((64, 64), (800, 800), (1920, 1080)):
        f = tmp_path / f"cornell_{w}x{h}.blob"
        f.write_bytes(abi.build_scene(0, w, h))
        args += [f, CORNELL]
    out = run(exe, args)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.count(f"walk_shape {CORNELL}, 2 groups") == 3


def test_other_scenes_have_none(exe, tmp_path):
    names = sorted(n for n in SCENES if n != "scene0")
    assert {"scene1", "scene3"} <= set(names) and len(names) >= 15
    args = ["scene"]
    for n in names:
        f = tmp_path / f"{n}.blob"
        f.write_bytes(SCENES[n]())
        args += [f, 0]
    out = run(exe, args)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.count("walk_shape 0,") == len(names)


def test_cornell_box_walked_through_a_tree_has_none(exe, tmp_path):
    """RTW_BRUTE_MAX=0 sends scene 0 through the tree: no candidate lists, no walk image, no shape"""
    f = tmp_path / "cornell.blob"
    f.write_bytes(abi.build_scene(0, 64, 64))
    out = run(exe, ["scene", f, 0], env={"RTW_BRUTE_MAX": "0"})
    assert out.returncode == 0, out.stderr[-3000:]


def test_edited_group_tables_are_rejected(exe):
    out = run(exe, ["edits"])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "edits: 22 group tables" in out.stdout
