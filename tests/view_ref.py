"""Helper of the view tests (include/rtw.h rtw_views), not a test: the oracle as the referee of a frame, and the test cameras.

Frame v of rtw_views is defined as rtw_render's frame of the uploaded scene with views[v]'s camera and camera type written into the
blob's header, under views[v].seed. The oracle renders exactly that, so it referees frames, segment and shadow-ray counts as it
stands. The cameras are defined once, here: per scene (a) the scene's own camera with a lens, (b) an environment camera inside the
scene, (c) an orthographic camera built the way the host description's ioOrthographicCamera builds it. In the oracle's frame at
least half of every view's pixels are non-zero (tests/test_views_cpu.py asserts it), so that a bit-for-bit comparison never compares
black frames."""
import ctypes as C
import functools

import numpy as np

import oracle
import radiance_ref as R
from raytracing_weekend_amd import abi

_HDR = C.sizeof(abi.SceneHeader)
SCENES = R.SCENES  # scene0, scene1, scene3, textured_cornell, random_volumes_motion: radiance_ref.scene's blobs
W, H, SPP, DEPTH = 24, 16, 48, 8  # the frames of the bit-for-bit test
SEEDS = (0x6314759, 12345, 0xfeedbeef)  # of views (a), (b), (c)
MIN_LIT = 0.5  # the fraction of a view's pixels that must be non-zero in the oracle's frame


def view_blob(blob, view):
    """The blob with the view's camera and camera type in its header; everything else as it is."""
    h = abi.SceneHeader.from_buffer_copy(blob[:_HDR])
    h.camera = abi.Camera.from_buffer_copy(bytes(view.camera))
    h.camera_type = view.camera_type
    return bytes(h) + blob[_HDR:]


def expect(blob, views, params, threads=4):
    """The oracle's answer for rtw_views(views, params): ((n, height, width, 4) float32 frames, summed segments, summed shadow rays).
    `params` is an abi.ViewParams."""
    frames = np.empty((len(views), params.height, params.width, 4), np.float32)
    seg = shadow = 0
    for i, v in enumerate(views):
        p = abi.make_params(params.width, params.height, params.spp, params.max_depth, seed=v.seed, rng_kind=params.rng_kind,
                            sample_offset=params.sample_offset, estimator=params.estimator)
        frames[i], st = oracle.render(view_blob(blob, v), p, threads=threads)
        seg, shadow = seg + st.segments, shadow + st.shadow_rays
    return frames, seg, shadow


def _f3(a):
    return np.asarray(a, np.float64).astype(np.float32).reshape(3)


def _frame(frm, to, up):
    """ioCamera's frame in float32: w = normalize(from - to), u = normalize(cross(up, w)), v = cross(w, u)."""
    def norm(v):
        return (np.float32(1.0) / np.sqrt(np.float32(np.dot(v, v)))) * v
    frm, to, up = _f3(frm), _f3(to), _f3(up)
    w = norm(frm - to)
    u = norm(np.cross(up, w).astype(np.float32))
    v = np.cross(w, u).astype(np.float32)
    return frm, u, v, w


def environment_camera(frm, to, up, t0=0.0, t1=0.0):
    """ioEnvironmentCamera: position and frame; lower_left, horizontal and vertical are 0."""
    frm, u, v, w = _frame(frm, to, up)
    z = np.zeros(3, np.float32)
    return np.concatenate([frm, u, v, w, z, z, z, np.array([0.0, t0, t1], np.float32)]).astype(np.float32)


def orthographic_camera(frm, to, up, height, width, t0=0.0, t1=0.0):
    """ioOrthographicCamera: lower_left = origin - (width / 2) u - (height / 2) v - w, horizontal = width u, vertical = height v."""
    f = np.float32
    frm, u, v, w = _frame(frm, to, up)
    hh, hw = f(height) / f(2.0), f(width) / f(2.0)
    ll = frm - hw * u - hh * v - w
    return np.concatenate([frm, u, v, w, ll, (f(2.0) * hw) * u, (f(2.0) * hh) * v, np.array([0.0, t0, t1], np.float32)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cameras(name):
    """The three views of scene `name`, seeds SEEDS. In random_volumes_motion view (b) has time0 = 0.25 and time1 = 0.75: the view's
    own times are what a frame uses."""
    blob = R.scene(name)
    a = abi.scene_view(blob, SEEDS[0])
    if name == "scene1":
        a.camera.lens_radius = 0.05
        b = environment_camera((0, 2, 0), (4, 1, 0), (0, 1, 0))
        c = orthographic_camera((3, 4, 1.5), (3, 3, 1.5), (0, 0, 1), 12.0, 12.0)
    else:  # the box scenes' cameras (the random scene's content sits in the same cube)
        a.camera.lens_radius = 6.0
        t0, t1 = (0.25, 0.75) if name == "random_volumes_motion" else (0.0, 0.0)
        b = environment_camera((278, 278, 278), (278, 278, 555), (0, 1, 0), t0, t1)
        if name == "random_volumes_motion":
            # that scene has a floor and no walls, and half of the box camera's rays leave it: this one looks down on the floor, from
            # y = 499 (the origin enters twice) over x, z in [8, 548]
            c = orthographic_camera((139, 250, 139), (139, 249, 139), (0, 0, 1), 540.0, 540.0)
        else:
            c = orthographic_camera((139, 139, -400), (139, 139, -399), (0, 1, 0), 540.0, 540.0)
    return (a, abi.make_view(b, abi.RTW_CAM_ENVIRONMENT, SEEDS[1]), abi.make_view(c, abi.RTW_CAM_ORTHOGRAPHIC, SEEDS[2]))


def lit_fraction(frame):
    return float((frame[..., :3] != 0).any(-1).mean())


@functools.lru_cache(maxsize=None)
def case(name, rng_kind, estimator=0):
    """(blob, views, params, expected frames, segments, shadow rays) of one scene, generator and estimator; computed once."""
    blob, views = R.scene(name), list(cameras(name))
    params = abi.make_view_params(W, H, SPP, DEPTH, rng_kind=rng_kind, estimator=estimator)
    return (blob, views, params) + expect(blob, views, params)
