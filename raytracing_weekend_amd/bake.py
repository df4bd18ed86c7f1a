"""Baking on top of rtw_probe and rtw_probe_sh (include/rtw.h): the probes at the texel centres of an axis-aligned rectangle primitive
and the baked map - irradiance or ambient occlusion - in the layout of an RTW_TEX_IMAGE of that primitive; the points of an
irradiance volume, the spherical-harmonic basis of rtw_probe_sh and the irradiance its nine coefficients give for a normal.
Cameras for rtw_views: look_at (the host description's perspective camera), the six faces of a cube map and a turntable.
The polylines of the paths rtw_paths recorded (path_segments)."""
import math

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


def bake_rect_adaptive(renderer, blob, prim, nu, nv, cap, max_depth, threshold, side=1, offset=1e-3, **kw):
    """bake_rect sampled to a noise target: Renderer.probe_adaptive on the same probes, every texel up to `cap` samples. Returns the
    (nv, nu, 4) float32 map, the (nv, nu) int32 samples each texel took and its (nv, nu) float32 error estimate; **kw goes to
    Renderer.probe_adaptive (min_spp, step_spp, mode, ...). The blob must be the uploaded scene."""
    out, spp, err = renderer.probe_adaptive(rect_probes(blob, prim, nu, nv, side, offset), cap, max_depth, threshold, **kw)
    return out.reshape(nv, nu, 4), spp.reshape(nv, nu), err.reshape(nv, nu)


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


def _normalize32(v):
    f = np.float32
    dd = f(f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(v[2] * v[2]))
    return (f(1.0) / np.sqrt(dd)) * v


def _cross32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)


def look_at(frm, to, up, vfov, aspect, aperture=0.0, focus_dist=1.0, t0=0.0, t1=0.0):
    """The 24 float32 of an rtw_camera (origin, u, v, w, lower_left, horizontal, vertical, lens_radius, time0, time1) of a perspective
    camera at `frm` looking at `to`, by the host description's ioPerspectiveCamera formulas in float32: w = normalize(frm - to),
    u = normalize(cross(up, w)), v = cross(w, u); vfov is top to bottom in degrees, aspect width over height; the lens radius is
    aperture / 2 and the frame stands at focus_dist: lower_left = frm - hw f u - hh f v - f w, horizontal = 2 hw f u, vertical =
    2 hh f v with hh = tan(vfov / 2), hw = aspect hh. abi.make_view takes the array."""
    f = np.float32
    frm, to, up = (np.asarray(a, np.float64).astype(np.float32).reshape(3) for a in (frm, to, up))
    w = _normalize32(frm - to)
    u = _normalize32(_cross32(up, w))
    v = _cross32(w, u)
    theta = f(vfov) * f(np.pi) / f(180.0)
    hh = np.tan(theta / f(2.0), dtype=np.float32)
    hw = f(aspect) * hh
    fd = f(focus_dist)
    ll = frm - (hw * fd) * u - (hh * fd) * v - fd * w
    hor = (f(2.0) * hw * fd) * u
    ver = (f(2.0) * hh * fd) * v
    return np.concatenate([frm, u, v, w, ll, hor, ver, [f(aperture) / f(2.0), f(t0), f(t1)]]).astype(np.float32)


# cube_views' faces, in order: the direction the face looks along and its up vector
CUBE_FACES = (((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)), ((0, -1, 0), (0, 0, 1)),
              ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)))


def cube_views(position, seed=0x6314759):
    """Six abi.View for Renderer.views: the 90 degree perspective cameras (aspect 1, no lens, focus distance 1) of a cube map at
    `position`, in the order +x, -x, +y, -y, +z, -z (CUBE_FACES: up is +y for the four side faces, -z for +y and +z for -y). `seed`
    is one seed for all six faces or a sequence of six."""
    pos = np.asarray(position, np.float64).reshape(3)
    seeds = [seed] * 6 if isinstance(seed, (int, np.integer)) else list(seed)
    if len(seeds) != 6:
        raise ValueError("cube_views: seed is one integer or six")
    return [abi.make_view(look_at(pos, pos + np.array(d, np.float64), up, 90.0, 1.0), abi.RTW_CAM_PERSPECTIVE, s)
            for (d, up), s in zip(CUBE_FACES, seeds)]


def orbit_views(blob, n, seed=0x6314759):
    """n abi.View for Renderer.views: a turntable of the scene blob's camera. View 0 is the blob's camera, copied and not recomputed;
    view k is that camera (its type, lens and times kept) rotated rigidly by 360 k / n degrees about the camera's v axis through
    the pivot lower_left + horizontal / 2 + vertical / 2, the centre of its frame: points (origin, lower_left) turn about the
    pivot, vectors (u, v, w, horizontal, vertical) about the origin; computed in double precision and rounded to float32 once. `seed` is one
    seed for every view or a sequence of n."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n <= 0:
        raise ValueError(f"orbit_views: n = {n!r}, expected a positive integer")
    seeds = [seed] * n if isinstance(seed, (int, np.integer)) else list(seed)
    if len(seeds) != n:
        raise ValueError("orbit_views: seed is one integer or n of them")
    base = abi.scene_view(blob, seeds[0])
    c = [float(x) for x in np.frombuffer(bytes(base.camera), np.float32)]
    fields = [c[3 * i:3 * i + 3] for i in range(7)]  # origin, u, v, w, lower_left, horizontal, vertical
    v, ll, hor, ver = fields[2], fields[4], fields[5], fields[6]
    pivot = [(ll[i] + hor[i] / 2.0) + ver[i] / 2.0 for i in range(3)]
    norm = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    axis = [v[i] / norm for i in range(3)]
    out = [base]
    for k in range(1, n):
        # Rodrigues' rotation in Python floats, every operation written out: the command-line tool's -orbit makes the same views
        ang = (2.0 * math.pi * float(k)) / float(n)
        cs, sn = math.cos(ang), math.sin(ang)
        omc = 1.0 - cs

        def rot(x):
            cr = [axis[1] * x[2] - axis[2] * x[1], axis[2] * x[0] - axis[0] * x[2], axis[0] * x[1] - axis[1] * x[0]]
            d = (axis[0] * x[0] + axis[1] * x[1]) + axis[2] * x[2]
            return [(x[i] * cs + cr[i] * sn) + axis[i] * (d * omc) for i in range(3)]
        cam = []
        for f, x in enumerate(fields):
            if f in (0, 4):  # points turn about the pivot, vectors about the origin
                r = rot([x[i] - pivot[i] for i in range(3)])
                cam += [pivot[i] + r[i] for i in range(3)]
            else:
                cam += rot(x)
        out.append(abi.make_view(np.array(cam + c[21:24], np.float64).astype(np.float32), base.camera_type, seeds[k]))
    return out


def path_segments(heads, vertices, miss_length=None):
    """The world-space polylines of the paths Renderer.paths / paths_views recorded, for plotting: one (m + 1, 3) float32 array per
    sample, in the arrays' order (ray-major), m = min(segments, max_records) the records the library wrote - the origins of its
    segments and then the end point o + t * d of the last one (float32, one rounding per operation). A sample without records gives
    a (0, 3) array. A path that leaves the scene ends on a miss, whose t is the segment's tmax (1e27 after the first segment):
    miss_length, where given, is the ray parameter such a last segment is drawn to instead."""
    heads, vertices = np.asarray(heads), np.asarray(vertices)
    if heads.dtype != abi.PATH_HEAD or vertices.dtype != abi.PATH_VERTEX or vertices.shape[:-1] != heads.shape:
        raise ValueError("path_segments: expected the (heads, vertices) pair of Renderer.paths or Renderer.paths_views")
    k = vertices.shape[-1]
    out = []
    for h, v in zip(heads.reshape(-1), vertices.reshape(-1, k)):
        m = min(int(h["segments"]), k)
        if m == 0:
            out.append(np.zeros((0, 3), np.float32))
            continue
        last = v[m - 1]
        t = np.float32(miss_length) if miss_length is not None and last["prim"] < 0 else last["t"]
        with np.errstate(over="ignore", invalid="ignore"):
            end = (last["o"] + (t * last["d"]).astype(np.float32)).astype(np.float32)
        out.append(np.concatenate([v["o"][:m], end[None, :]]).astype(np.float32))
    return out
