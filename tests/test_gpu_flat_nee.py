"""The one-light instantiation's straight-line light sample on the GPU (-m gpu; csrc/rtw_nee.h): small renders, 64 x 64 at depth 6,
every one bit for bit against the CPU oracle - the image and the three counts. shadow_rays is the number of lanes whose sample had
`has`, so the counts test the combined predicate directly; the image tests every output that is read under it.

Scene 0 runs the fixed-shape instantiation as a frame, as an interleaved shard and through render_adaptive's list twin. One-light
scenes built from tests/lighting_ref.py's rectangles run the twin that reads the list headers, with the sampled rectangle on each of
the three axes, and with vertices that fail each test of the predicate: a Lambertian of albedo 0 (f == 0), a light whose normal
faces away from the receiver but towards a ceiling (costa <= 0 on the one, > 0 on the other), and a ceiling above the plane of a
light that faces down. TEA + LCG and a scene with two listed lights must still take the generic text. The oracle's frames are
rendered once per case and shared."""
import numpy as np
import pytest

import lighting_ref as L
import oracle
from raytracing_weekend_amd import abi
from test_gpu_onelight import KNOBS, with_camera

pytestmark = pytest.mark.gpu
W, H, DEPTH = 64, 64, 6
CEILING = L.Rect(1, (-1000.0, 1000.0, -1000.0, 1000.0), 4.0, "lambert", L.ALBEDO, flip=1)
BLACK_WALL = L.Rect(2, (-1000.0, 1000.0, 0.0, 1000.0), 3.0, "lambert", (0.0, 0.0, 0.0), flip=1)
L_Z = L.Light((-2.0, 0.5, -4.0), (4.0, 0.0, 0.0), (0.0, 1.5, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 3.0))  # L.E_UNLISTED's rectangle
SIDE_PDF = (0, (0.5, 3.0, -1.0, 1.0), 3.0)   # L.E_SIDE's rectangle: the X generator
Z_PDF = (2, (-2.0, 2.0, 0.5, 2.0), -4.0)     # L.E_UNLISTED's: the Z generator
# name: (lights, rects, pdf_rect)
SCENES = {
    "y_light": ([L.L_ABOVE], [L.RECEIVER, L.E_ABOVE, L.OCCLUDER], L.FOREIGN_PDF),
    "x_light": ([L.L_SIDE], [L.RECEIVER, L.E_SIDE, L.OCCLUDER], SIDE_PDF),
    "z_light": ([L_Z], [L.RECEIVER, L.E_UNLISTED, L.OCCLUDER], Z_PDF),
    "black_wall": ([L.L_ABOVE], [L.RECEIVER, L.E_ABOVE, BLACK_WALL], L.ABOVE_PDF),
    "faces_away": ([L.L_BEHIND], [L.RECEIVER, L.E_ABOVE, CEILING], L.ABOVE_PDF),
    "above_the_light": ([L.L_ABOVE], [L.RECEIVER, L.E_ABOVE, CEILING], L.ABOVE_PDF),
    "two_lights": ([L.L_ABOVE, L.L_SIDE], [L.RECEIVER, L.E_ABOVE, L.E_SIDE, L.OCCLUDER], L.FOREIGN_PDF),
}
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


def blob_of(scene):
    if scene not in _blobs:
        if scene in SCENES:
            lights, rects, pdf_rect = SCENES[scene]
            _blobs[scene] = with_camera(L.LightCase(lights, rects, pdf_rect, DEPTH, (L.REF,)).blob, 0)
        else:
            _blobs[scene] = abi.build_scene(scene, W, H)
    return _blobs[scene]


def reference(scene, spp, **kw):
    """the oracle's frame and counts, rendered once"""
    key = (scene, spp, tuple(sorted(kw.items())))
    if key not in _refs:
        img, st = oracle.render(blob_of(scene), abi.make_params(W, H, spp, DEPTH, **kw), threads=16)
        img.setflags(write=False)
        _refs[key] = (img, (st.samples, st.segments, st.shadow_rays))
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(gpu, scene, spp, **kw):
    gpu.upload_scene(blob_of(scene))
    img, st = gpu.render(abi.make_params(W, H, spp, DEPTH, **kw))
    ref, counts = reference(scene, spp, **kw)
    print(f"{scene} {spp} spp {kw}: counts {(st.samples, st.segments, st.shadow_rays)}, oracle {counts}, "
          f"{np.count_nonzero(_bits(img) != _bits(ref))} words differ")
    assert (st.samples, st.segments, st.shadow_rays) == counts, scene
    assert np.array_equal(_bits(img), _bits(ref)), f"{scene}: {np.count_nonzero(_bits(img) != _bits(ref))} words differ"
    return counts


def test_cornell_frame(gpu):
    """17 samples end inside the second block"""
    counts = check(gpu, 0, 17)
    assert 0 < counts[2] < counts[1]  # (some light samples were probed, some vertices took none)


def test_cornell_interleaved_shard(gpu):
    """shard 1 of 3: rows 1, 4, 7, ..."""
    check(gpu, 0, 17, row0=1, row_stride=3)


def test_cornell_adaptive_list_twin(gpu):
    """render_adaptive with threshold 0, min_spp 32 and cap 64 (the smallest pair it takes with a list pass to run): the passes after the
    first 32 samples run the LIST twin. Every pixel is the oracle's pixel at its own sample count; where every pixel went to the cap,
    the counts are the oracle's at the cap."""
    cap = 64
    gpu.upload_scene(blob_of(0))
    img, spp, _, st = gpu.render_adaptive(abi.make_params(W, H, cap, DEPTH), 0.0, min_spp=32)
    assert st.samples == int(spp.astype(np.int64).sum())
    assert spp.max() == cap, np.unique(spp)  # (the list passes ran)
    for n in np.unique(spp):
        ref, _ = reference(0, int(n))
        m = spp == n
        assert np.array_equal(_bits(img[m]), _bits(ref[m])), f"spp {n}: {np.count_nonzero(_bits(img[m]) != _bits(ref[m]))} words differ"
    print(f"adaptive: sample counts {np.unique(spp, return_counts=True)}, counts {(st.samples, st.segments, st.shadow_rays)}")
    if (spp == cap).all():
        assert (st.samples, st.segments, st.shadow_rays) == reference(0, cap)[1]


def test_one_light_on_each_axis(gpu):
    """lists that are not the Cornell box's: the twin that reads the list headers; the sampled rectangle lies on a Y, an X and a Z plane
    (one test for the three scenes: check names the scene it fails on)"""
    for scene in ("y_light", "x_light", "z_light"):
        counts = check(gpu, scene, 16)
        assert counts[2] > 0, scene


def test_vertices_that_fail_the_predicate(gpu):
    """f == 0 on the black wall; costa <= 0 on the receiver under a light that faces up and on the ceiling above one that faces down. The
    other surface of each scene passes the tests, so has holds on some lanes of a wave and not on others."""
    for scene in ("black_wall", "faces_away", "above_the_light"):
        counts = check(gpu, scene, 16)
        assert 0 < counts[2] < counts[1], scene


def test_tea_lcg_and_two_lights_take_the_generic_text(gpu):
    check(gpu, 0, 16, rng_kind=abi.RTW_RNG_TEA_LCG)
    counts = check(gpu, "two_lights", 16)
    assert counts[2] > 0
