"""Helper of the view-guide tests (include/rtw.h rtw_views_guides / rtw_denoise_views), not a test: the referees, which are existing
entry points and not under test, and the condition that keeps a bit-for-bit comparison from comparing empty guides.

The guides of view v are defined as what rtw_render_guides writes for the scene with views[v] in its header under views[v].seed;
frame v of rtw_denoise_views as rtw_denoise_guided of frame v alone. The cameras are view_ref's but one (cameras)."""
import functools

import numpy as np

import guides_ref
import oracle
import view_ref as V
from raytracing_weekend_amd import abi

W, H, SPP = V.W, V.H, 16  # the frames of the bit-for-bit test
MIN_HIT = 0.2  # the fraction of a view's pixels that must have prim >= 0 in the referee's guides, with at least two distinct ids
# A lower bound of a view's hit fraction can be had on the CPU: in the oracle's 1-spp frame of all_emitters(view_blob(...)), sky off,
# a non-zero pixel is a front-face hit (front_face_hits; tests/test_views_guides_cpu.py holds every view to MIN_HIT by it). For
# view (b) of scene1 that bound is 0.02 and settles nothing: its hit fraction is established on the referee, in the GPU suite.
UNSETTLED = {("scene1", 1)}


def same(a, b):
    """Equal shapes, dtypes and bits (float32 or int32)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def front_face_hits(blob, view, w=W, h=H):
    """(fraction of the pixels of the view whose first sample meets a front face, the primitives met): the oracle's 1-spp frame of the
    all-emitter scene with the view's camera, every primitive showing its index as its colour."""
    n = len(abi.parse_scene(blob)["prims"])
    cols = [((i % 255 + 1) / 256.0, (i // 255 + 1) / 256.0, 0.25) for i in range(n)]  # exact in float32
    img, _ = oracle.render(guides_ref.all_emitters(V.view_blob(blob, view), cols), abi.make_params(w, h, 1, 5, seed=view.seed), threads=4)
    lit = img[..., 2] != 0
    code = (np.rint(img[..., 0][lit] * 256.0).astype(np.int64) - 1) + 255 * (np.rint(img[..., 1][lit] * 256.0).astype(np.int64) - 1)
    return float(lit.mean()), sorted(set(code.tolist()))


@functools.lru_cache(maxsize=None)
def cameras(name):
    """view_ref.cameras(name) - three views, three seeds, the three camera kinds, lenses, one view with times of its own - with one
    view replaced: scene3's orthographic camera looks along the box's axis, so the walls, floor and ceiling are edge-on, the boxes
    are media (which guides skip) and the referee's prim guide holds the back wall alone. Tilted a little towards -x and -y it
    sees the walls and the floor as well (front_face_hits: 0.74 of the pixels, five primitives)."""
    a, b, c = V.cameras(name)
    if name == "scene3":
        c = abi.make_view(V.orthographic_camera((139, 139, -400), (129, 129, -300), (0, 1, 0), 540.0, 540.0), abi.RTW_CAM_ORTHOGRAPHIC, V.SEEDS[2])
    return (a, b, c)


def referee_guides(gpu, blob, views, w, h, spp, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, which=abi.GUIDES):
    """rtw_render_guides per view, after upload_scene(view_blob(blob, v)) and with seed = v.seed, stacked along a leading view axis.
    Leaves `blob` itself uploaded (under the knobs of the caller's environment)."""
    out = {k: [] for k in which}
    for v in views:
        gpu.upload_scene(V.view_blob(blob, v))
        g = gpu.render_guides(abi.make_params(w, h, spp, 0, seed=v.seed, rng_kind=rng_kind, sample_offset=sample_offset), which=which)
        for k in which:
            out[k].append(g[k])
    gpu.upload_scene(blob)
    return {k: np.stack(v) for k, v in out.items()}


def hit_fractions(prim):
    """Per view of an (n, h, w) prim guide: (fraction of pixels with prim >= 0, number of distinct primitive ids)."""
    return [(float((p >= 0).mean()), len(np.unique(p[p >= 0]))) for p in prim]


def referee_denoise(gpu, frames, albedo, normal, iterations, **sigmas):
    """rtw_denoise_guided per frame."""
    return np.stack([gpu.denoise_guided(f, a, n, iterations=iterations, **sigmas) for f, a, n in zip(frames, albedo, normal)])


def distinct_frames(n, h, w, seed=5):
    """n frames of different content with their guides, as rtw_denoise_views takes them: noisy colour in [0, 1], albedo and normal
    piecewise constant with noise, every frame from its own stream. A tap that strays into a neighbouring frame reads other values."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    frames, alb, nrm = (np.empty((n, h, w, 4), np.float32) for _ in range(3))
    for v in range(n):
        edge = ((xs * (v + 2) + ys * (3 - v)) // 7) % 3
        frames[v] = rng.random((h, w, 4), dtype=np.float32)
        alb[v] = (edge[..., None] * np.float32(0.3) + rng.random((h, w, 4), dtype=np.float32) * np.float32(0.1 * (v + 1)))
        nrm[v] = (np.float32(1.0) - edge[..., None] * np.float32(0.4) + rng.random((h, w, 4), dtype=np.float32) * np.float32(0.05 * (v + 1)))
        frames[v, ..., 3] = np.float32(0.25 * (v + 1))
    return frames, alb, nrm
