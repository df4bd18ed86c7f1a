"""Helper of the radiance-query tests (include/rtw.h rtw_radiance), not a test: the oracle as the referee of a user ray.

A radiance query is a camera path whose camera ray is replaced. The oracle's perspective camera with horizontal = vertical = 0 and
lens_radius = 0 makes every pixel's ray origin = cam.origin, dir = (0 * s + lower_left) - origin, and its generator is keyed by
pixel = width * y + x. So a blob whose header carries ray i as its camera, rendered with width = 1, height = k + 1, rows [k, k + 1),
is "ray i with stream key k": the mean in the library's summation order and the segment and shadow-ray counts of that ray alone.
rtw_params.row0 and height are int32, so keys from 2^31 - 1 on cannot be a row of a one-pixel-wide image: their samples come from
rtwo_trace_pixel at (x, y) = (k mod 2^16, k div 2^16) of a 65536-wide image (the same key k = 65536 * y + x, the same ray at every
pixel), summed here in the library's order - the equality test_radiance_cpu.py checks on a small key - and carry no counts."""
import ctypes as C
import functools

import numpy as np

import geometry_ref as G
import oracle
from raytracing_weekend_amd import abi

SUM_BLOCK, SUM_UNIT = 16, 128  # RTW_SUM_BLOCK, RTW_SUM_BLOCK * RTW_SUM_UNIT_BLOCKS
_HDR = C.sizeof(abi.SceneHeader)


def ray_blob(blob, o, ll):
    """The blob with its camera replaced by the ray from o through ll; time0 / time1 stay as they are."""
    h = abi.SceneHeader.from_buffer_copy(blob[:_HDR])
    h.camera_type = abi.RTW_CAM_PERSPECTIVE
    h.camera.lens_radius = 0.0
    for a in range(3):
        h.camera.origin[a] = float(o[a])
        h.camera.lower_left[a] = float(ll[a])
        h.camera.horizontal[a] = 0.0
        h.camera.vertical[a] = 0.0
    return bytes(h) + blob[_HDR:]


def make_rays(o, ll, estimator=0):
    """(n, 8) float32 rays whose direction carries the bits of the oracle's camera ray: d = (float32(0) + ll) - o in float32,
    tmin = the estimator's start distance, tmax = 1e27f."""
    o, ll = np.asarray(o, np.float32), np.asarray(ll, np.float32)
    d = (np.float32(0) + ll) - o
    n = len(o)
    tmin = np.float32(1e-6 if estimator == 0 else 1e-3)
    return np.concatenate([o, d, np.full((n, 1), tmin, np.float32), np.full((n, 1), np.float32(1e27), np.float32)], axis=1).astype(np.float32)


def special_origins(blob):
    """World-space centres of the dielectric spheres and of the media: origins inside the glass and inside a medium."""
    parts = abi.parse_scene(blob)
    out = []
    for p in parts["prims"]:
        mat = parts["materials"][p.material]
        if p.type == abi.PRIM_SPHERE and mat.type == abi.MAT_DIELECTRIC:
            c = np.array([p.p[0], p.p[1], p.p[2]], np.float64)
        elif p.type == abi.PRIM_VOLUME_SPHERE:
            c = np.array([p.p[0], p.p[1], p.p[2]], np.float64)
        elif p.type == abi.PRIM_VOLUME_BOX:
            c = 0.5 * (np.array([p.p[0], p.p[1], p.p[2]], np.float64) + np.array([p.p[3], p.p[4], p.p[5]], np.float64))
        else:
            continue
        m = np.array(list(parts["xforms"][p.xform].m), np.float64).reshape(3, 4)
        out.append(m[:, :3] @ c + m[:, 3])
    return np.array(out, np.float64).reshape(-1, 3)


def pairs(blob, n, seed=G.RAY_SEED):
    """n pairs (o, ll) of float32 points: geometry_ref.scene_rays' origins with a point along each direction, the first few
    origins replaced by points inside the glass spheres and the media (at most n / 4 of them)."""
    rays, _, _ = G.scene_rays(blob, seed, n)
    o = rays[:, 0:3].copy()
    inside = special_origins(blob)[: n // 4]
    o[: len(inside)] = inside.astype(np.float32)
    ll = (o + rays[:, 3:6] * np.float32(1.75)).astype(np.float32)
    return o, ll


def sum_in_order(samples, spp):
    """float32 mean of (spp, 3) sample radiances in the library's order: samples inside blocks of 16, block sums inside units of
    128 samples, unit sums, then the division by float32(spp)."""
    s = np.asarray(samples, np.float32)
    total = np.zeros(3, np.float32)
    for u0 in range(0, spp, SUM_UNIT):
        usum = np.zeros(3, np.float32)
        for b0 in range(u0, min(u0 + SUM_UNIT, spp), SUM_BLOCK):
            bsum = np.zeros(3, np.float32)
            for i in range(b0, min(b0 + SUM_BLOCK, u0 + SUM_UNIT, spp)):
                bsum = (bsum + s[i]).astype(np.float32)
            usum = (usum + bsum).astype(np.float32)
        total = (total + usum).astype(np.float32)
    return (total / np.float32(spp)).astype(np.float32)


def trace_samples(blob, o, ll, key, spp, depth, seed, rng_kind, sample_offset, estimator):
    """(spp, 3) float32: rtwo_trace_pixel's radiance of samples sample_offset ... of the ray with stream key `key` (any 32-bit key)."""
    lib = oracle.load()
    rb = ray_blob(blob, o, ll)
    x, y = key & 0xffff, key >> 16
    p = abi.make_params(65536, y + 1, spp, depth, seed=seed, rng_kind=rng_kind, sample_offset=sample_offset, estimator=estimator)
    out = np.zeros((spp, 3), np.float32)
    for s in range(spp):
        rc = lib.rtwo_trace_pixel(rb, len(rb), C.byref(p), x, y, sample_offset + s, out[s].ctypes.data)
        assert rc == 0, rc
    return out


def expect(blob, o, ll, spp, depth, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0):
    """The oracle's answer for rays make_rays(o, ll): ((n, 4) float32 pixels, summed segments, summed shadow rays). The counts are
    None when a key lies beyond what a one-pixel-wide image can address (see the module text)."""
    n = len(o)
    pix = np.empty((n, 4), np.float32)
    seg = shadow = 0
    for i in range(n):
        k = (key_offset + i) & 0xffffffff
        if k < 2 ** 31 - 1:
            p = abi.make_params(1, k + 1, spp, depth, seed=seed, row0=k, row1=k + 1, rng_kind=rng_kind, sample_offset=sample_offset,
                                estimator=estimator)
            img, st = oracle.render(ray_blob(blob, o[i], ll[i]), p)
            pix[i] = img[0, 0]
            if seg is not None:
                seg, shadow = seg + st.segments, shadow + st.shadow_rays
        else:
            pix[i, :3] = sum_in_order(trace_samples(blob, o[i], ll[i], k, spp, depth, seed, rng_kind, sample_offset, estimator), spp)
            pix[i, 3] = 1.0
            seg = shadow = None
    return pix, seg, shadow


@functools.lru_cache(maxsize=None)
def scene(name):
    w = h = 32
    if name == "textured_cornell":
        return oracle.textured_cornell(w, h)
    if name == "random_volumes_motion":
        return oracle.random_scene(23, w, h, n_prims=40, volumes=True, motion=True)
    return abi.build_scene(int(name[5:]), w, h)


SCENES = ("scene0", "scene1", "scene3", "textured_cornell", "random_volumes_motion")
N, SPP, DEPTH, KEY = 96, 48, 8, 5  # the batch of the bit-for-bit test: one and a half waves


@functools.lru_cache(maxsize=None)
def case(name, rng_kind, estimator=0):
    """(blob, o, ll, rays, expected pixels, segments, shadow rays) of one scene, generator and estimator; computed once."""
    blob = scene(name)
    o, ll = pairs(blob, N)
    return (blob, o, ll, make_rays(o, ll, estimator)) + expect(blob, o, ll, SPP, DEPTH, rng_kind=rng_kind, estimator=estimator, key_offset=KEY)
