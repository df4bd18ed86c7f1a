"""k_path's one-light instantiation on the GPU (-m gpu): small renders, every one bit for bit against the CPU oracle - the image and the
three counts. Scene 0 (the Cornell box: one listed rectangle light, the reference estimator) with Philox runs the new instantiation,
as a frame, as an interleaved shard and through render_adaptive's list twin; TEA + LCG, a scene with two listed lights, a scene with
none under a sky, and the corrected estimator must fall back to the generic instantiations: chosen wrongly, the one-light code would
skip the light-index draw and the scale by the number of lights, or sample a light that is not there, and the bits would differ. The
oracle's frames are rendered once per case and shared."""
import ctypes as C

import numpy as np
import pytest

import lighting_ref as L
import oracle
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu
KNOBS = ("RTW_PATH", "RTW_PATH_UNIT_BLOCKS", "RTW_PATH_FINE_BLOCKS", "RTW_BLOCKSUM_BYTES", "RTW_CULL", "RTW_BRUTE_MAX", "RTW_LDS_KB")
W, H = 96, 64
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


def with_camera(blob, sky):
    """The blob of a lighting_ref case (whose camera is one ray) under a lens-free perspective camera above the receiver plane that
    looks down at the origin and sees the emitters, and with the header's sky light as given."""
    n = C.sizeof(abi.SceneHeader)
    h = abi.SceneHeader.from_buffer_copy(blob[:n])
    h.camera_type, h.sky_light = abi.RTW_CAM_PERSPECTIVE, sky
    h.camera.lens_radius, h.camera.time0, h.camera.time1 = 0.0, 0.0, 0.0
    for a, (o, ll, hz, vt) in enumerate(zip((0.5, 1.5, -7.0), (-3.5, -2.5, -1.0), (8.0, 0.0, 0.0), (0.0, 5.0, 1.0))):
        h.camera.origin[a], h.camera.lower_left[a], h.camera.horizontal[a], h.camera.vertical[a] = o, ll, hz, vt
    return bytes(h) + blob[n:]


def blob_of(scene):
    if scene not in _blobs:
        if scene == "two_lights":
            c = L.LightCase([L.L_ABOVE, L.L_SIDE], [L.RECEIVER, L.E_ABOVE, L.E_SIDE, L.OCCLUDER], L.FOREIGN_PDF, 8, (L.REF,))
            _blobs[scene] = with_camera(c.blob, 0)
        elif scene == "sky":
            c = L.LightCase([], [L.RECEIVER, L.OCCLUDER, L.E_UNLISTED], L.FOREIGN_PDF, 8, (L.REF,))
            _blobs[scene] = with_camera(c.blob, 1)
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


@pytest.mark.parametrize("rng", [abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG], ids=["philox", "tea_lcg"])
@pytest.mark.parametrize("spp,depth", [(17, 50), (16, 4)])
def test_cornell_frame(gpu, rng, spp, depth):
    """17 samples end inside the second block; Philox runs the one-light instantiation, TEA + LCG the generic one"""
    counts = check(gpu, 0, W, H, spp, depth, rng_kind=rng)
    assert counts[2] > 0  # (light samples were probed)


@pytest.mark.parametrize("spp,depth", [(17, 50), (16, 4)])
def test_cornell_interleaved_shard(gpu, spp, depth):
    """shard 1 of 3: rows 1, 4, 7, ..."""
    check(gpu, 0, W, H, spp, depth, row0=1, row_stride=3)


@pytest.mark.parametrize("depth", [50, 4])
def test_cornell_adaptive_list_twin(gpu, depth):
    """render_adaptive with threshold 0: the passes after the first min_spp samples run the LIST twin of the one-light instantiation.
    Every pixel is the oracle's pixel at its own sample count; where every pixel went to the cap, the counts are the oracle's at the
    cap. min_spp 32 and cap 64: rtw_render_adaptive takes no min_spp below 2 * RTW_SUM_BLOCK = 32 (it refuses 16 with an error), and
    a cap equal to min_spp would leave no list pass to run."""
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


@pytest.mark.parametrize("scene", ["two_lights", "sky"])
def test_other_light_lists_fall_back(gpu, scene):
    """two listed lights (the index draw, the scale by 2, the records from memory) and no light under a sky: the generic instantiation"""
    counts = check(gpu, scene, 64, 64, 8, 8)
    assert (counts[2] > 0) == (scene == "two_lights")


def test_corrected_estimator_falls_back(gpu):
    """scene 0 under the corrected estimator runs the cold instantiation, whatever its light list"""
    check(gpu, 0, W, H, 16, 4, estimator=L.CORR)
