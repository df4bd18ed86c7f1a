"""Baking on top of rtw_probe and rtw_probe_sh (include/rtw.h): the probes at the texel centres of an axis-aligned rectangle primitive
and the baked map - irradiance or ambient occlusion - in the layout of an RTW_TEX_IMAGE of that primitive; the points of an
irradiance volume, the spherical-harmonic basis of rtw_probe_sh and the irradiance its nine coefficients give for a normal."""
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


def probe_grid(lo, hi, nx, ny, nz, tmin=1e-6, tmax=1e27):
    """(nx * ny * nz, 8) float32 points for Renderer.probe_sh: a regular grid from corner `lo` to corner `hi` (both included; an axis
    with one point sits at lo), x fastest, then y, then z - point (ix, iy, iz) is row (iz * ny + iy) * nx + ix. Floats 3..5 are 0,
    floats 6 and 7 are tmin and tmax."""
    if nx <= 0 or ny <= 0 or nz <= 0:
        raise ValueError("probe_grid: nx, ny and nz must be positive")
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    axes = [np.linspace(lo[k], hi[k], m) if m > 1 else np.array([lo[k]]) for k, m in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    out = np.zeros((nx * ny * nz, 8), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = x.ravel(), y.ravel(), z.ravel()
    out[:, 6] = np.float32(tmin)
    out[:, 7] = np.float32(tmax)
    return out


def sh_basis(normals):
    """(..., 9) float32: rtw_probe_sh's basis at (..., 3) directions, one float32 rounding per operation as the header writes it."""
    d = np.asarray(normals, np.float32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    f = np.float32
    return np.stack([np.full(x.shape, f(0.282094792), np.float32),
                     f(0.488602512) * y, f(0.488602512) * z, f(0.488602512) * x,
                     f(1.092548431) * (x * y), f(1.092548431) * (y * z),
                     f(0.315391565) * (f(3.0) * (z * z) - f(1.0)),
                     f(1.092548431) * (x * z), f(0.546274215) * ((x * x) - (y * y))], axis=-1).astype(np.float32)


def sh_irradiance(coeffs, normals):
    """Irradiance from rtw_probe_sh's coefficients, in float64: coeffs (..., 9, C) with any number of channels C (the float4's w
    included, if it is there), normals (..., 3) unit vectors broadcast against the leading axes -> (..., C).
    E(n) = pi c_0 Y_0 + (2 pi / 3) sum_m c_1m Y_1m(n) + (pi / 4) sum_m c_2m Y_2m(n): the radiance convolved with the clamped cosine
    (Ramamoorthi and Hanrahan's nine-coefficient irradiance)."""
    c = np.asarray(coeffs, np.float64)
    y = sh_basis(normals).astype(np.float64)
    band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return ((y * band)[..., :, None] * c).sum(axis=-2)
