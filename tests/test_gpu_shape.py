"""k_path's fixed-shape walks on the GPU (-m gpu): small renders, every one bit for bit against the CPU oracle - the image and the three
counts. Scene 0 (the Cornell box) with Philox runs the instantiation whose two list walks are compiled for the box's list shape (two
groups; 2 + 3 + 1 rectangles and a sphere, then the transformed box's 2 + 2 + 2 rectangles), as a frame, as an interleaved shard and
through render_adaptive's list twin. Scenes that still run the one-light instantiation but have other lists must take the walk that
reads the group headers: a one-light scene of three rectangles, the box's rectangles moved into the identity group (one group), and
a wall retyped so that the counts are 1, 3, 2. Chosen wrongly, the fixed walk would test records as the wrong kind, or read records
that are not there, and every pixel would differ. (TEA + LCG runs the generic kernel: tests/test_gpu_variants.py renders that frame.) The oracle's frames are rendered once per case
and shared."""
import numpy as np
import pytest

import lighting_ref as L
import oracle
from raytracing_weekend_amd import abi
from test_gpu_onelight import KNOBS, with_camera

pytestmark = pytest.mark.gpu
W, H = 96, 64
RECT_X, RECT_Z = 2, 4  # include/rtw.h rtw_prim_type
_refs = {}
_blobs = {}


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def edited_cornell(edit):
    parts = abi.parse_scene(abi.build_scene(0, W, H))
    prims = list(parts["prims"])
    if edit == "one_group":  # the box's six rectangles as they lie, untransformed: one group of 4 + 5 + 3 rectangles and a sphere
        box = [p for p in prims if p.xform != 0]
        assert len(box) == 6
        for p in box:
            p.xform = 0
    else:  # the first wall with an x normal becomes a z-rectangle with the same numbers: the identity group counts 1, 3, 2
        wall = next(p for p in prims if p.xform == 0 and p.type == RECT_X)
        wall.type = RECT_Z
        assert sum(p.xform == 0 and p.type == RECT_X for p in prims) == 1
    parts["prims"] = prims
    return abi.assemble_scene(parts)


def blob_of(scene):
    if scene not in _blobs:
        if scene == "one_light":
            c = L.LightCase([L.L_ABOVE], [L.RECEIVER, L.E_ABOVE, L.OCCLUDER], L.FOREIGN_PDF, 8, (L.REF,))
            _blobs[scene] = with_camera(c.blob, 0)
        elif scene in ("one_group", "retyped_wall"):
            _blobs[scene] = edited_cornell(scene)
        else:
            _blobs[scene] = abi.build_scene(scene, W, H)
    return _blobs[scene]


def reference(scene, w, h, spp, depth, **kw):
    """the oracle's frame and counts, rendered once"""
    key = (scene, w, h, spp, depth, tuple(sorted(kw.items())))
    if key not in _refs:
        img, st = oracle.render(blob_of(scene), abi.make_params(w, h, spp, depth, **kw), threads=16)
        img.setflags(write=False)
        _refs[key] = (img, (st.samples, st.segments, st.shadow_rays))
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(gpu, scene, w, h, spp, depth, **kw):
    gpu.upload_scene(blob_of(scene))
    img, st = gpu.render(abi.make_params(w, h, spp, depth, **kw))
    ref, counts = reference(scene, w, h, spp, depth, **kw)
    print(f"{scene} {w}x{h} {spp} spp depth {depth} {kw}: counts {(st.samples, st.segments, st.shadow_rays)}, oracle {counts}, "
          f"{np.count_nonzero(_bits(img) != _bits(ref))} words differ")
    assert (st.samples, st.segments, st.shadow_rays) == counts
    assert np.array_equal(_bits(img), _bits(ref)), f"{np.count_nonzero(_bits(img) != _bits(ref))} words differ"
    return counts


@pytest.mark.parametrize("spp,depth", [(17, 50), (16, 4)])
def test_cornell_frame(gpu, spp, depth):
    """17 samples end inside the second block; the counts are the fixed-shape instantiation's per-wave counters"""
    counts = check(gpu, 0, W, H, spp, depth)
    assert counts[2] > 0  # (light samples were probed: the any-hit walk ran)


@pytest.mark.parametrize("spp,depth", [(17, 50), (16, 4)])
def test_cornell_interleaved_shard(gpu, spp, depth):
    """shard 1 of 3: rows 1, 4, 7, ..."""
    check(gpu, 0, W, H, spp, depth, row0=1, row_stride=3)


@pytest.mark.parametrize("depth", [50, 4])
def test_cornell_adaptive_list_twin(gpu, depth):
    """render_adaptive with threshold 0, min_spp 32 and cap 64 (as tests/test_gpu_onelight.py, which says why): the passes after the
    first 32 samples run the LIST twin of the fixed-shape instantiation. Every pixel is the oracle's pixel at its own sample count;
    where every pixel went to the cap, the counts are the oracle's at the cap."""
    cap = 64
    gpu.upload_scene(blob_of(0))
    img, spp, _, st = gpu.render_adaptive(abi.make_params(W, H, cap, depth), 0.0, min_spp=32)
    assert st.samples == int(spp.astype(np.int64).sum())
    assert spp.max() == cap, np.unique(spp)  # (the list passes ran)
    for n in np.unique(spp):
        ref, _ = reference(0, W, H, int(n), depth)
        m = spp == n
        assert np.array_equal(_bits(img[m]), _bits(ref[m])), f"spp {n}: {np.count_nonzero(_bits(img[m]) != _bits(ref[m]))} words differ"
    print(f"adaptive depth {depth}: sample counts {np.unique(spp, return_counts=True)}, counts {(st.samples, st.segments, st.shadow_rays)}")
    if (spp == cap).all():
        assert (st.samples, st.segments, st.shadow_rays) == reference(0, W, H, cap, depth)[1]


def test_one_light_scene_of_another_shape_falls_back(gpu):
    """one listed light over three untransformed rectangles: the one-light instantiation, the walk that reads the headers"""
    counts = check(gpu, "one_light", 64, 64, 8, 8)
    assert counts[2] > 0


@pytest.mark.parametrize("scene", ["one_group", "retyped_wall"])
def test_edited_cornell_lists_fall_back(gpu, scene):
    """the Cornell box with one group instead of two, and with the identity group's counts 1, 3, 2 instead of 2, 3, 1"""
    counts = check(gpu, scene, W, H, 16, 4)
    assert counts[2] > 0
