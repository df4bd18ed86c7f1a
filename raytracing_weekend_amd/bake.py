"""Lightmap baking on top of rtw_probe (include/rtw.h): the probes at the texel centres of an axis-aligned rectangle primitive, and
the baked map - irradiance or ambient occlusion - in the layout of an RTW_TEX_IMAGE of that primitive."""
import numpy as np

from . import abi

_RECTS = (abi.PRIM_RECT_X, abi.PRIM_RECT_Y, abi.PRIM_RECT_Z)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def rect_normal(parts, prim):
    """The world-space shading normal rtw_cast reports for rectangle `prim`: +-axis by the flip flag, under the inverse transpose of
    the primitive's transform and normalised in float32 (csrc/rtw_scene.h bake_hitrec's operations)."""
    p = parts["prims"][prim]
    axis = _RECTS.index(p.type)
    sign = np.float32(-1.0 if p.flip else 1.0)
    n = np.zeros(3, np.float32)
    n[axis] = sign
    if p.xform != 0:
        inv = np.array(list(parts["xforms"][p.xform].inv), np.float32)
        v = inv[4 * axis:4 * axis + 3] * sign  # the other two terms of the inverse transpose are products with 0
        dd = _f32(float(v[0]) * float(v[0]))
        dd = _f32(float(v[1]) * float(v[1]) + float(dd))  # fmaf: the product is exact in float64
        dd = _f32(float(v[2]) * float(v[2]) + float(dd))
        n = v * (np.float32(1.0) / np.sqrt(dd))
    return n.astype(np.float32)


def rect_probes(blob, prim, nu, nv, side=1, offset=1e-3):
    """(nv * nu, 8) float32 probes (position, normal, tmin, tmax) at the texel centres of the axis-aligned rectangle primitive `prim`
    of the scene blob, taken through the primitive's transform. The normal is `side` (+1 or -1) times the shading normal rtw_cast
    reports, the position is lifted by `offset` along it, tmin = 1e-6 and tmax = 1e27. Texel (i, j) - row j * nu + i - sits where
    rtw_cast's uv is ((i + 0.5) / nu, (j + 0.5) / nv), row 0 at v = 0: the baked map is an RTW_TEX_IMAGE of that primitive.
    Any other primitive kind raises ValueError."""
    parts = abi.parse_scene(blob)
    if not 0 <= prim < len(parts["prims"]) or parts["prims"][prim].type not in _RECTS:
        raise ValueError(f"rect_probes: primitive {prim} is not an axis-aligned rectangle")
    if nu <= 0 or nv <= 0 or side not in (1, -1):
        raise ValueError("rect_probes: nu and nv must be positive, side +1 or -1")
    p = parts["prims"][prim]
    a0, a1, b0, b1, k = (float(p.p[i]) for i in range(5))
    u = (np.arange(nu, dtype=np.float64) + 0.5) / nu
    v = (np.arange(nv, dtype=np.float64) + 0.5) / nv
    a, b = np.meshgrid(a0 + u * (a1 - a0), b0 + v * (b1 - b0))  # (nv, nu): row j holds v_j
    a, b = a.ravel(), b.ravel()
    kk = np.full_like(a, k)
    obj = {abi.PRIM_RECT_X: (kk, a, b), abi.PRIM_RECT_Y: (a, kk, b), abi.PRIM_RECT_Z: (a, b, kk)}[p.type]
    pts = np.stack(obj, axis=1)
    if p.xform != 0:
        m = np.array(list(parts["xforms"][p.xform].m), np.float64).reshape(3, 4)
        pts = pts @ m[:, :3].T + m[:, 3]
    n = rect_normal(parts, prim) * np.float32(side)
    out = np.empty((nv * nu, 8), np.float32)
    out[:, 0:3] = (pts + float(offset) * n.astype(np.float64)).astype(np.float32)
    out[:, 3:6] = n
    out[:, 6] = np.float32(1e-6)
    out[:, 7] = np.float32(1e27)
    return out


def bake_rect(renderer, blob, prim, nu, nv, spp, max_depth, side=1, offset=1e-3, **kw):
    """The (nv, nu, 4) float32 map of rectangle `prim`: Renderer.probe on rect_probes(blob, prim, nu, nv, side, offset) with spp samples
    per texel; **kw goes to Renderer.probe (mode="occlusion" bakes ambient occlusion). The blob must be the uploaded scene."""
    return renderer.probe(rect_probes(blob, prim, nu, nv, side, offset), spp, max_depth, **kw).reshape(nv, nu, 4)
