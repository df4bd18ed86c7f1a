"""Every row of k_path's and k_first's lists (csrc/rtw_variants.h) on the GPU (-m gpu): one case per row - a scene, a generator, an
estimator, and render (the frame rows) or render_adaptive (the list rows); k_first's rows under RTW_PATH=0. Before it renders, a
case asserts which row it selects: tests/native/variants_check.cpp works that out on the CPU from the very blob the case uploads, so a
case that drifts to another row fails instead of quietly testing something else. Then the image and the three counts must be the CPU
oracle's, bit for bit, as in tests/test_gpu_shape.py. 24 x 20 pixels are seven whole groups of 64 and one of 32; 32 samples are two
blocks of 16 and the least min_spp an adaptive call takes; the adaptive cases go on to a cap of 48 at threshold 0 (as
test_gpu_shape.py's list twin), where every pixel is the oracle's pixel at its own count. The oracle's frames are rendered once per
scene, generator, estimator and count, and shared by the k_path and k_first cases. The cases run from one test, which goes
on after a failing case and names each one that failed, as tests/test_gpu_paths.py runs its cases.

The other lists need no case here. k_shade, k_bounce and k_trace_bvh: tests/test_gpu_parity.py renders tree scenes against the oracle
with both generators at each feature level (test_matches_oracle and test_random_scenes_match_oracle: hot; the textured and media
scenes of test_textured_reference_scenes_match_oracle and test_tree_scene_with_volumes_matches_oracle: cold features;
test_corrected_estimators_match_oracle: the mixture estimator), and test_image_does_not_depend_on_the_launch_schedule runs the
workgroup sizes and LDS budgets that select k_trace_bvh's other rows. k_trace<true>: the RTW_PATH=0 legs of that test on scenes 0 and 3,
and the k_first cases below on scene 0; k_trace<false>: the RTW_PATH=0 legs of tests/test_gpu_camera.py on its moving sphere.
k_classify<true>: every k_path frame case below on a scene with a walk image; k_classify<false>: the small scene with moving spheres
(no walk image) of test_gpu_parity.py's test_random_scenes_match_oracle and test_gpu_camera.py's moving sphere under k_path."""
import numpy as np
import pytest

import lighting_ref as L
import oracle
from raytracing_weekend_amd import abi
from test_gpu_onelight import KNOBS, with_camera
from test_gpu_shape import blob_of as shape_blob_of, check as shape_check, edited_cornell
from test_variants_cpu import build_exe, row_of

pytestmark = pytest.mark.gpu
W, H, SPP, CAP, DEPTH = 24, 20, 32, 48, 6
P, T = abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG
REF, CORR, MIX = abi.RTW_EST_REFERENCE, abi.RTW_EST_CORRECTED, abi.RTW_EST_MIXTURE
_refs = {}
_blobs = {}

# row -> (scene, generator, estimator); the list rows: the same with render_adaptive and step_spp 16 (Philox) or 0 (TEA + LCG)
PATH_CASES = {
    "PHILOX_HOT": ("two_lights", P, REF), "TEA_HOT": (0, T, REF),
    "PHILOX_COLD": ("textured", P, REF), "TEA_COLD": (0, T, CORR),
    "PHILOX_MIX": (0, P, MIX), "TEA_MIX": ("textured", T, MIX),
    "PHILOX_MEDIA": (3, P, REF), "TEA_MEDIA": (3, T, REF),
    "PHILOX_ONE": ("one_light", P, REF), "PHILOX_BOX": (0, P, REF),
}
LIST_SCENE = {"PHILOX_ONE": "one_group"}  # (the list twin of the one-light row on the other one-light scene)
FIRST_CASES = {
    "PHILOX_HOT": (0, P, REF), "TEA_HOT": (1, T, REF),
    "PHILOX_COLD": (2, P, REF), "TEA_COLD": (3, T, REF),
    "PHILOX_MIX": (0, P, MIX), "TEA_MIX": ("textured", T, MIX),
}


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory.mktemp("variants"))


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def blob_of(scene):
    if scene not in _blobs:
        if scene == "one_light":
            c = L.LightCase([L.L_ABOVE], [L.RECEIVER, L.E_ABOVE, L.OCCLUDER], L.FOREIGN_PDF, 8, (L.REF,))
            _blobs[scene] = with_camera(c.blob, 0)
        elif scene == "two_lights":
            c = L.LightCase([L.L_ABOVE, L.L_SIDE], [L.RECEIVER, L.E_ABOVE, L.E_SIDE, L.OCCLUDER], L.FOREIGN_PDF, 8, (L.REF,))
            _blobs[scene] = with_camera(c.blob, 0)
        elif scene == "one_group":
            _blobs[scene] = edited_cornell(scene)
        elif scene == "textured":
            _blobs[scene] = oracle.textured_cornell(W, H)
        else:
            _blobs[scene] = abi.build_scene(scene, W, H)
    return _blobs[scene]


def reference(scene, spp, rng, est):
    """the oracle's frame and counts, rendered once"""
    key = (scene, spp, rng, est)
    if key not in _refs:
        img, st = oracle.render(blob_of(scene), abi.make_params(W, H, spp, DEPTH, rng_kind=rng, estimator=est), threads=16)
        img.setflags(write=False)
        _refs[key] = (img, (st.samples, st.segments, st.shadow_rays))
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_case(gpu, exe, tmp_path, monkeypatch, kernel, row, scene, rng, est, list_pass):
    env = {"RTW_PATH": "0"} if kernel == "k_first" else {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = tmp_path / "scene.blob"
    f.write_bytes(blob_of(scene))
    chosen = row_of(exe, f, rng, est, list_pass, W, H, DEPTH, env=env)
    assert chosen[kernel] == row and chosen["pipeline"] == ("path" if kernel == "k_path" else "wavefront"), chosen
    gpu.upload_scene(blob_of(scene))
    if not list_pass:
        img, st = gpu.render(abi.make_params(W, H, SPP, DEPTH, rng_kind=rng, estimator=est))
        ref, counts = reference(scene, SPP, rng, est)
        print(f"{row}: counts {(st.samples, st.segments, st.shadow_rays)}, oracle {counts}, {np.count_nonzero(_bits(img) != _bits(ref))} words differ")
        assert (st.samples, st.segments, st.shadow_rays) == counts
        assert np.array_equal(_bits(img), _bits(ref))
        return
    img, spp, _, st = gpu.render_adaptive(abi.make_params(W, H, CAP, DEPTH, rng_kind=rng, estimator=est), 0.0, min_spp=SPP, step_spp=16 if rng == P else 0)
    print(f"{row}: sample counts {np.unique(spp, return_counts=True)}, counts {(st.samples, st.segments, st.shadow_rays)}")
    assert st.samples == int(spp.astype(np.int64).sum())
    assert spp.max() == CAP and set(np.unique(spp)) <= {SPP, CAP}, np.unique(spp)  # (the list pass ran)
    for n in np.unique(spp):
        ref, _ = reference(scene, int(n), rng, est)
        m = spp == n
        assert np.array_equal(_bits(img[m]), _bits(ref[m])), f"spp {n}: {np.count_nonzero(_bits(img[m]) != _bits(ref[m]))} words differ"
    if (spp == CAP).all():
        assert (st.samples, st.segments, st.shadow_rays) == reference(scene, CAP, rng, est)[1]


def test_every_k_path_and_k_first_row_runs_its_own_code(gpu, exe, tmp_path, monkeypatch):
    """All 32 cases from one test, which goes on after a failing case and names each one that failed. Last, the frame that
    tests/test_gpu_shape.py used to render for "TEA + LCG runs the generic kernel" (96 x 64, 16 spp, depth 4), now with its row asserted."""
    failed = []
    cases = [("k_path", "PATH_", PATH_CASES), ("k_first", "FIRST_", FIRST_CASES)]
    for kernel, prefix, table in cases:
        for row, (scene, rng, est) in table.items():
            for list_pass in (False, True):
                name = prefix + ("LIST_" if list_pass else "") + row
                sc = LIST_SCENE.get(row, scene) if list_pass and kernel == "k_path" else scene
                monkeypatch.delenv("RTW_PATH", raising=False)
                try:
                    run_case(gpu, exe, tmp_path, monkeypatch, kernel, name, sc, rng, est, list_pass)
                except AssertionError as e:
                    failed.append(f"{name}: {str(e)[:300]}")
    monkeypatch.delenv("RTW_PATH", raising=False)
    try:
        f = tmp_path / "shape.blob"
        f.write_bytes(shape_blob_of(0))
        assert row_of(exe, f, T, REF, False, 96, 64, 4) == {"pipeline": "path", "k_path": "PATH_TEA_HOT", "k_first": "FIRST_TEA_HOT"}
        shape_check(gpu, 0, 96, 64, 16, 4, rng_kind=T)
    except AssertionError as e:
        failed.append(f"scene 0 with TEA + LCG at 96 x 64: {str(e)[:300]}")
    assert not failed, f"{len(failed)} of {sum(2 * len(t) for _, _, t in cases) + 1} cases failed:\n" + "\n".join(failed)
