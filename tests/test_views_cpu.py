"""CPU suite of the views (include/rtw.h rtw_views / rtw_views_device): the ABI and Python surface, the referee against itself, the
cameras of bake.py, the planning header under the sanitizers, and the condition that keeps the GPU suite's bit-for-bit test from
comparing black frames."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import radiance_ref as R
import view_ref as V
from raytracing_weekend_amd import abi, bake

HEADER = os.path.join(abi.REPO_DIR, "include", "rtw.h")
BOTH = (abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG)


def cam(view_or_array):
    a = view_or_array.camera if isinstance(view_or_array, abi.View) else None
    f = np.frombuffer(bytes(a), np.float32) if a is not None else np.asarray(view_or_array, np.float32)
    names = ("origin", "u", "v", "w", "lower_left", "horizontal", "vertical")
    out = {k: f[3 * i:3 * i + 3].astype(np.float64) for i, k in enumerate(names)}
    out.update(lens_radius=float(f[21]), time0=float(f[22]), time1=float(f[23]))
    return out


def central_ray(c, s=0.5, t=0.5):
    d = c["lower_left"] + s * c["horizontal"] + t * c["vertical"] - c["origin"]
    return d / np.linalg.norm(d)


# ---------------------------------------------------------------- the ABI and the Python surface
def test_struct_sizes_header_text_and_version():
    assert C.sizeof(abi.View) == 112 and C.sizeof(abi.ViewParams) == 32 and C.sizeof(abi.Camera) == 96
    assert abi.View.camera_type.offset == 96 and abi.View.seed.offset == 100 and abi.View.reserved.offset == 104
    assert [n for n, _ in abi.ViewParams._fields_] == ["width", "height", "spp", "max_depth", "rng_kind", "sample_offset", "estimator", "reserved"]
    text = open(HEADER).read()
    assert re.search(r"#define RTW_ABI_VERSION 5\b", text) and abi.RTW_ABI_VERSION == 5
    assert re.search(r"\} rtw_view;\s*/\* 112 B \*/", text) and re.search(r"\} rtw_view_params;\s*/\* 32 B \*/", text)
    assert "int rtw_views(rtw_ctx* ctx, const rtw_view* views, size_t n_views, const rtw_view_params* params, float* rgba_out, rtw_stats* stats);" in text
    assert re.search(r"int rtw_views_device\(rtw_ctx\* ctx, const rtw_view\* d_views, size_t n_views, const rtw_view_params\* params, void\* d_rgba, "
                     r"void\* hip_stream,\s*rtw_stats\* stats\);", text)
    for phrase in ("is a perspective camera", "(v * height + y) * width + x", "width * y + x", "RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES",
                   "leaves *stats alone", "n_views = 0 is RTW_OK"):
        assert phrase in text, phrase


def test_symbols_are_exported_and_a_null_context_is_an_error():
    lib = abi.load_hip()
    assert "rtw_views" in abi.HIP_SYMBOLS and "rtw_views_device" in abi.HIP_SYMBOLS
    assert lib.rtw_abi_version() == 5
    vp = abi.make_view_params(4, 4, 1, 1)
    v = abi.View()
    out = np.zeros(64, np.float32)
    assert lib.rtw_views(None, C.byref(v), 1, C.byref(vp), out.ctypes.data, None) == -1
    assert lib.rtw_views_device(None, C.byref(v), 1, C.byref(vp), out.ctypes.data, None, None) == -1
    assert lib.rtw_views(None, None, 0, None, None, None) == -1 and not out.any()


def test_python_side_validation():
    blob = R.scene("scene0")
    v = abi.scene_view(blob, seed=7)
    h = abi.parse_scene(blob)["header"]
    assert bytes(v.camera) == bytes(h.camera) and v.camera_type == h.camera_type and v.seed == 7 and tuple(v.reserved) == (0, 0)
    assert abi.scene_view(blob).seed == 0x6314759 and abi.make_view(h.camera, seed=2 ** 32 + 5).seed == 5
    a = np.arange(24, dtype=np.float32)
    w = abi.make_view(a, abi.RTW_CAM_ORTHOGRAPHIC, 9)
    assert np.array_equal(np.frombuffer(bytes(w.camera), np.float32), a) and (w.camera_type, w.seed) == (2, 9)
    w.camera.origin[0] = 5.0
    assert a[0] == 0.0 and h.camera.origin[0] == abi.parse_scene(blob)["header"].camera.origin[0]  # copies
    for bad in (3, -1, 7, 1.0, True, None):
        with pytest.raises(ValueError):
            abi.make_view(h.camera, bad)
    with pytest.raises(ValueError):
        abi.make_view(np.zeros(23, np.float32))
    for kw in (dict(width=0), dict(width=-3), dict(height=0), dict(spp=0), dict(spp=1.5), dict(width=True), dict(height="4")):
        args = dict(width=4, height=4, spp=1, max_depth=1)
        args.update(kw)
        with pytest.raises(ValueError):
            abi.make_view_params(**args)
    p = abi.make_view_params(7, 5, 3, 2, rng_kind=1, sample_offset=4, estimator=2)
    assert (p.width, p.height, p.spp, p.max_depth, p.rng_kind, p.sample_offset, p.estimator, p.reserved) == (7, 5, 3, 2, 1, 4, 2, 0)
    assert len(abi.view_array(v)) == 1 and len(abi.view_array([v, w])) == 2 and len(abi.view_array([])) == 0
    arr = abi.view_array([v, w])
    assert abi.view_array(arr) is arr and bytes(arr)[112:] == bytes(w)
    for bad in ([h.camera], [v, None], [a]):
        with pytest.raises(ValueError):
            abi.view_array(bad)


# ---------------------------------------------------------------- the referee
@pytest.mark.parametrize("rng_kind", BOTH)
def test_the_referee_of_the_scenes_own_camera_is_the_oracles_render(rng_kind):
    for name in ("scene0", "scene1"):
        blob = R.scene(name)
        assert V.view_blob(blob, abi.scene_view(blob)) == blob
        params = abi.make_view_params(V.W, V.H, 8, 5, rng_kind=rng_kind, sample_offset=3)
        frames, seg, shadow = V.expect(blob, [abi.scene_view(blob, seed=77)], params)
        img, st = oracle.render(blob, abi.make_params(V.W, V.H, 8, 5, seed=77, rng_kind=rng_kind, sample_offset=3))
        assert frames.shape == (1, V.H, V.W, 4) and np.array_equal(frames[0].view(np.uint32), img.view(np.uint32))
        assert (seg, shadow) == (st.segments, st.shadow_rays) and seg > 0
        # two views: the frames in order, the counts summed; another camera gives another frame
        other = V.cameras(name)[1]
        f2, s2, sh2 = V.expect(blob, [other, abi.scene_view(blob, seed=77)], params)
        assert np.array_equal(f2[1].view(np.uint32), img.view(np.uint32)) and not np.array_equal(f2[0], f2[1]) and s2 > seg and sh2 >= shadow


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("name", V.SCENES)
def test_every_test_camera_sees_the_scene(name, rng_kind):
    """The condition of the GPU suite's bit-for-bit test: in the oracle's frame at least half of every view's pixels are non-zero."""
    blob, views, params, frames, seg, shadow = V.case(name, rng_kind)
    lit = [V.lit_fraction(f) for f in frames]
    print(name, rng_kind, "non-zero fractions", lit, "segments", seg, "shadow rays", shadow)
    assert [v.camera_type for v in views] == [0, 1, 2] and len({v.seed for v in views}) == 3
    assert views[0].camera.lens_radius > 0 and np.isfinite(frames).all() and (frames[..., 3] == 1.0).all()
    assert min(lit) >= V.MIN_LIT, lit
    if name == "random_volumes_motion":
        assert (views[1].camera.time0, views[1].camera.time1) == (0.25, 0.75)


def test_the_orthographic_test_camera_is_the_host_descriptions():
    c = cam(V.cameras("scene0")[2])
    # the origin enters twice (camera.cuh:52): rays start at lower_left + s horizontal + t vertical + origin, x and y in [8, 548]
    lo = c["lower_left"] + c["origin"]
    hi = lo + c["horizontal"] + c["vertical"]
    assert np.allclose(np.minimum(lo, hi)[:2], (8, 8)) and np.allclose(np.maximum(lo, hi)[:2], (548, 548)) and np.allclose(c["w"], (0, 0, -1))
    e = cam(V.cameras("scene0")[1])
    assert not e["lower_left"].any() and not e["horizontal"].any() and not e["vertical"].any() and np.allclose(e["w"], (0, 0, -1))


# ---------------------------------------------------------------- bake's cameras
def test_look_at_aims_the_frame_centre_at_the_target_and_steps_by_a_pixel():
    frm, to = np.array([13.0, 2.0, 3.0]), np.array([1.0, 0.5, -2.0])
    a = bake.look_at(frm, to, (0, 1, 0), 35.0, 1.5, aperture=0.2, focus_dist=9.0, t0=0.25, t1=0.5)
    assert a.dtype == np.float32 and a.shape == (24,)
    c = cam(a)
    # the ray through the frame's centre passes through `to`
    d = central_ray(c)
    want = (to - frm) / np.linalg.norm(to - frm)
    assert np.allclose(d, want, atol=1e-6)
    t = np.dot(to - frm, d)
    assert np.linalg.norm(frm + t * d - to) < 1e-4
    # a pixel step is horizontal / width (and vertical / height): the rays through neighbouring pixel centres differ by exactly that
    width, height = 48, 32
    def through(x, y):
        return c["lower_left"] + ((x + 0.5) / width) * c["horizontal"] + ((y + 0.5) / height) * c["vertical"]
    assert np.allclose(through(11, 7) - through(10, 7), c["horizontal"] / width, atol=1e-9)
    assert np.allclose(through(10, 8) - through(10, 7), c["vertical"] / height, atol=1e-9)
    # ioPerspectiveCamera's frame: orthonormal, the frame at the focus distance, sized by the field of view and the aspect
    for p, q in (("u", "v"), ("v", "w"), ("u", "w")):
        assert abs(np.dot(c[p], c[q])) < 1e-6 and abs(np.linalg.norm(c[p]) - 1) < 1e-6
    hh = np.tan(np.radians(35.0) / 2)
    assert np.allclose(c["vertical"], 2 * hh * 9.0 * c["v"], rtol=1e-5) and np.allclose(c["horizontal"], 2 * 1.5 * hh * 9.0 * c["u"], rtol=1e-5)
    assert np.allclose(c["lower_left"] + c["horizontal"] / 2 + c["vertical"] / 2, frm - 9.0 * c["w"], atol=1e-4)
    assert np.allclose(c["w"], -want, atol=1e-6) and c["u"][1] == 0.0
    assert (c["lens_radius"], c["time0"], c["time1"]) == (np.float32(0.1), 0.25, 0.5)
    d0 = cam(bake.look_at(frm, to, (0, 1, 0), 35.0, 1.5))
    assert (d0["lens_radius"], d0["time0"], d0["time1"]) == (0.0, 0.0, 0.0)
    # the host description builds the same camera: scene 0's and scene 1's, rebuilt from what their frames say
    for scene in (0, 1):
        h = cam(abi.scene_view(abi.build_scene(scene, 200, 100)))
        pivot = h["lower_left"] + h["horizontal"] / 2 + h["vertical"] / 2
        f = np.linalg.norm(pivot - h["origin"])
        vfov = np.degrees(2 * np.arctan(np.linalg.norm(h["vertical"]) / (2 * f)))
        mine = cam(bake.look_at(h["origin"], pivot, (0, 1, 0), vfov, np.linalg.norm(h["horizontal"]) / np.linalg.norm(h["vertical"]), focus_dist=f))
        for k in ("origin", "u", "v", "w", "lower_left", "horizontal", "vertical"):
            assert np.allclose(mine[k], h[k], rtol=1e-5, atol=1e-5 * f), (scene, k)


def test_cube_views_look_along_the_six_axes():
    pos = (3.0, -2.0, 5.0)
    views = bake.cube_views(pos, seed=11)
    assert len(views) == 6 and all(isinstance(v, abi.View) and v.camera_type == 0 and v.seed == 11 for v in views)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    assert [d for d, _ in bake.CUBE_FACES] == axes
    for v, axis in zip(views, axes):
        c = cam(v)
        assert np.allclose(c["origin"], pos) and np.allclose(central_ray(c), axis, atol=1e-6) and c["lens_radius"] == 0.0
        # 90 degrees, aspect 1: the frame's edges are at 45 degrees from the axis, so the faces tile the sphere
        for s, t in ((0, 0.5), (1, 0.5), (0.5, 0), (0.5, 1)):
            assert abs(np.dot(central_ray(c, s, t), axis) - np.sqrt(0.5)) < 1e-6
        assert abs(np.linalg.norm(c["horizontal"]) - 2) < 1e-6 and abs(np.linalg.norm(c["vertical"]) - 2) < 1e-6
    assert [v.seed for v in bake.cube_views(pos, seed=range(6))] == list(range(6))
    with pytest.raises(ValueError):
        bake.cube_views(pos, seed=[1, 2])


@pytest.mark.parametrize("name", ["scene0", "scene1"])
def test_orbit_views_turn_the_cameras_frame_about_its_centre(name):
    blob = R.scene(name)
    n = 8
    views = bake.orbit_views(blob, n, seed=5)
    h = abi.parse_scene(blob)["header"]
    assert len(views) == n and bytes(views[0].camera) == bytes(h.camera)  # view 0: the blob's camera byte for byte
    assert all(v.camera_type == h.camera_type and v.seed == 5 for v in views)
    c0 = cam(views[0])
    pivot = c0["lower_left"] + c0["horizontal"] / 2 + c0["vertical"] / 2
    dist = np.linalg.norm(c0["origin"] - pivot)
    half = cam(views[n // 2])
    assert np.allclose(half["origin"], 2 * pivot - c0["origin"], atol=1e-4 * max(1.0, dist))  # mirrored through the pivot
    assert np.allclose(half["u"], -c0["u"], atol=1e-6) and np.allclose(half["w"], -c0["w"], atol=1e-6) and np.allclose(half["v"], c0["v"], atol=1e-6)
    axis = c0["v"] / np.linalg.norm(c0["v"])
    for k, v in enumerate(views):
        c = cam(v)
        p = c["lower_left"] + c["horizontal"] / 2 + c["vertical"] / 2
        assert np.allclose(p, pivot, atol=1e-4 * max(1.0, dist))  # the pivot stays, every view looks at it
        assert abs(np.linalg.norm(c["origin"] - pivot) - dist) < 1e-4 * max(1.0, dist) and np.allclose(c["v"], c0["v"], atol=1e-6)
        assert abs(np.dot(c["origin"] - c0["origin"], axis)) < 1e-4 * max(1.0, dist)  # the origin stays in its plane
        assert np.allclose(central_ray(c), (pivot - c["origin"]) / dist, atol=1e-5)
        ang = np.degrees(np.arctan2(np.dot(np.cross(c0["w"], c["w"]), axis), np.dot(c0["w"], c["w"]))) % 360.0
        assert abs(ang - 360.0 * k / n) < 1e-3, (k, ang)
        assert (c["lens_radius"], c["time0"], c["time1"]) == (c0["lens_radius"], c0["time0"], c0["time1"])
        assert np.allclose([np.linalg.norm(c[q]) for q in ("horizontal", "vertical")], [np.linalg.norm(c0[q]) for q in ("horizontal", "vertical")], rtol=1e-6)
    assert len(bake.orbit_views(blob, 1)) == 1 and [v.seed for v in bake.orbit_views(blob, 3, seed=[4, 5, 6])] == [4, 5, 6]
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError):
            bake.orbit_views(blob, bad)


# ---------------------------------------------------------------- the planning header, under the sanitizers
def test_plan_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "view_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-o", exe, os.path.join(abi.REPO_DIR, "tests", "native", "view_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "view_plan_check ok" in out.stdout, out.stdout + out.stderr[-2000:]
