"""CPU suite of the view guides (include/rtw.h rtw_views_guides / rtw_denoise_views and their device variants): the ABI and the Python
surface, the refusals that need no device, the planning header under the sanitizers, the float32 restatement of the per-frame
filter, and the condition that keeps the GPU suite's bit-for-bit test from comparing empty guides."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guides_ref
import radiance_ref as R
import view_guides_ref as VG
import view_ref as V
from raytracing_weekend_amd import abi

HEADER = os.path.join(abi.REPO_DIR, "include", "rtw.h")
NEW = ("rtw_views_guides", "rtw_views_guides_device", "rtw_denoise_views", "rtw_denoise_views_device")


def test_header_declares_the_four_functions_and_the_abi_version_stays():
    text = open(HEADER).read()
    assert re.search(r"#define RTW_ABI_VERSION 5\b", text) and abi.RTW_ABI_VERSION == 5
    assert ("int rtw_views_guides(rtw_ctx* ctx, const rtw_view* views, size_t n_views, const rtw_view_params* params, const rtw_guides* out, "
            "rtw_stats* stats);") in text
    assert re.search(r"int rtw_views_guides_device\(rtw_ctx\* ctx, const rtw_view\* d_views, size_t n_views, const rtw_view_params\* params, "
                     r"const rtw_guides\* d_out,\s*void\* hip_stream, rtw_stats\* stats\);", text)
    assert re.search(r"int rtw_denoise_views\(rtw_ctx\* ctx, const float\* rgba_in, const float\* albedo, const float\* normal, float\* rgba_out, "
                     r"size_t n_views,\s*int32_t width, int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal\);", text)
    assert re.search(r"int rtw_denoise_views_device\(rtw_ctx\* ctx, const float\* rgba_in, const float\* albedo, const float\* normal, float\* rgba_out, "
                     r"size_t n_views,\s*int32_t width, int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal,\s*"
                     r"void\* hip_stream\);", text)
    for phrase in ("(v * height + y) * width + x", "a tap never reads another view", "is a perspective camera", "It allocates nothing per call",
                   "samples = segments = n_views*width*height*spp", "all four of its pointers NULL"):
        assert phrase in text, phrase
    # the structs the calls take are the ones that were there
    assert C.sizeof(abi.View) == 112 and C.sizeof(abi.ViewParams) == 32 and C.sizeof(abi.Guides) == 4 * C.sizeof(C.c_void_p)
    assert [n for n, _ in abi.Guides._fields_] == ["albedo", "normal", "depth", "prim"]


def test_symbols_are_exported_with_argtypes_and_a_null_context_is_an_error():
    lib = abi.load_hip()
    for name in NEW:
        assert name in abi.HIP_SYMBOLS and getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    assert len(lib.rtw_views_guides.argtypes) == 6 and len(lib.rtw_views_guides_device.argtypes) == 7
    assert len(lib.rtw_denoise_views.argtypes) == 12 and len(lib.rtw_denoise_views_device.argtypes) == 13
    vp = abi.make_view_params(4, 4, 1, 1)
    v = abi.View()
    buf = np.zeros(4 * 64, np.float32)
    g = abi.Guides(albedo=buf.ctypes.data)
    assert lib.rtw_views_guides(None, C.byref(v), 1, C.byref(vp), C.byref(g), None) == -1
    assert lib.rtw_views_guides_device(None, C.byref(v), 1, C.byref(vp), C.byref(g), None, None) == -1
    assert lib.rtw_views_guides(None, None, 0, None, None, None) == -1
    p = buf.ctypes.data
    assert lib.rtw_denoise_views(None, p, p + 256, p + 512, p + 768, 1, 4, 4, 1, 0.5, 0.4, 0.5) == -1
    assert lib.rtw_denoise_views_device(None, p, p + 256, p + 512, p + 768, 1, 4, 4, 1, 0.5, 0.4, 0.5, None) == -1
    assert not buf.any()


def test_python_side_validation_needs_no_device():
    class NoLibrary(abi.Renderer):
        def __init__(self):  # the argument checks come before the first call into the library
            self.lib, self.ctx, self.devices = None, C.c_void_p(), [0]
    r = NoLibrary()
    view = abi.scene_view(R.scene("scene0"))
    for kw in (dict(which=()), dict(which=("albedo", "colour")), dict(width=0), dict(height=-2), dict(spp=0), dict(spp=1.5)):
        args = dict(width=4, height=4, spp=4)
        args.update(kw)
        with pytest.raises(ValueError):
            r.views_guides([view], **args)
    with pytest.raises(ValueError):
        r.views_guides([None], 4, 4)
    with pytest.raises(ValueError):
        r.views_guides([view], 2 ** 15, 2 ** 16)
    with pytest.raises(ValueError):
        r.views_guides_device(1, 0, {"beauty": 16}, 4, 4)
    f = np.zeros((2, 4, 4, 4), np.float32)
    for bad in ((f[0], f[0], f[0]), (f, f[:1], f), (f, f, f[..., :3]), (f[..., :3], f[..., :3], f[..., :3])):
        with pytest.raises(ValueError):
            r.denoise_views(*bad)


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "view_guides_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-o", exe, os.path.join(abi.REPO_DIR, "tests", "native", "view_guides_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "view_guides_plan_check ok" in out.stdout, out.stdout + out.stderr[-2000:]


def test_the_frames_of_the_denoiser_test_differ_and_the_per_frame_filter_keeps_them_apart():
    """What the GPU suite's denoiser test rests on, on the CPU: the three frames and their guides differ, and the float32 restatement
    of rtw_denoise_guided, run on the three frames stacked into one image of three times the height, differs from the per-frame
    result at the frame borders - a filter whose taps stray into the neighbouring view would be caught."""
    frames, alb, nrm = VG.distinct_frames(3, VG.H, VG.W)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(alb[1], alb[2]) and not np.array_equal(nrm[0], nrm[2])
    per_frame = np.stack([guides_ref.atrous_guided(f, a, n, iterations=2) for f, a, n in zip(frames, alb, nrm)])
    stacked = guides_ref.atrous_guided(frames.reshape(-1, VG.W, 4), alb.reshape(-1, VG.W, 4), nrm.reshape(-1, VG.W, 4), iterations=2).reshape(frames.shape)
    assert np.isfinite(per_frame).all() and not np.array_equal(per_frame, frames)
    assert not np.array_equal(stacked[0, -1], per_frame[0, -1]) and not np.array_equal(stacked[1, 0], per_frame[1, 0])
    assert np.array_equal(per_frame[..., 3], frames[..., 3])  # alpha copied


@pytest.mark.parametrize("name", V.SCENES)
def test_every_test_camera_meets_the_scene(name):
    """The condition of the GPU suite's bit-for-bit test, where the oracle can referee it: a non-zero pixel of the all-emitter frame is
    a front-face hit, a lower bound of the fraction of pixels with prim >= 0. Every view is held to MIN_HIT here but scene1's
    environment view, whose front-face fraction says little (view_guides_ref.UNSETTLED): that one is held to MIN_HIT on the
    referee's own output in the GPU suite, as all the others are again."""
    blob, views = R.scene(name), VG.cameras(name)
    got = [VG.front_face_hits(blob, v) for v in views]
    print(name, "front-face fractions and primitives", got)
    assert [v.camera_type for v in views] == [0, 1, 2] and len({v.seed for v in views}) == 3 and views[0].camera.lens_radius > 0
    for k, (frac, prims) in enumerate(got):
        assert (frac >= VG.MIN_HIT and len(prims) >= 2) or (name, k) in VG.UNSETTLED, (name, k, frac, prims)
    assert len(VG.UNSETTLED) == 1
    if name == "random_volumes_motion":  # the odd-shape test's frames, and the view with times of its own
        assert max(VG.front_face_hits(blob, v, 7, 5)[0] for v in views) >= 0.5
        assert (views[1].camera.time0, views[1].camera.time1) == (0.25, 0.75)
    if name != "scene3":
        assert all(bytes(a) == bytes(b) for a, b in zip(views, V.cameras(name)))  # view_ref's cameras as they are
