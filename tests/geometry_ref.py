"""A float64 numpy reference for closest hits and texture coordinates: a second reading of include/rtw.h and of the
reference's intersection and texture programs (geometry/sphere.cu, movingSphere.cu, ioMovingSphere.h, shaders/aarect{x,y,z}.cu,
texture/imageTexture.cu, get_sphere_uv), written without looking at oracle/rtw_oracle.c or the kernels. Shared by
test_geometry_cpu.py (the oracle against this file) and test_gpu_geometry.py (the kernels against this file).

What is modelled
  Ray in object space   o' = inv * o + inv_3, d' = inv * d (rtw_xform.inv, world -> object); t is the same parameter in both
                        spaces, so unnormalised directions carry over unchanged.
  Sphere                a = d'.d', b = oc.d', c = oc.oc - r^2, disc = b^2 - a c; roots (-b -+ sqrt(disc)) / a, the near one first,
                        accepted when tmin < t < tmax (sphere.cu:52-90).
  Moving sphere         the instance's child is a matrix-motion transform with the keys translate(C0) at time 0 and translate(C1)
                        at time 1 (ioMovingSphere.h:161-203): the object-space origin is moved back by C0 + s (C1 - C0), s = the RAY
                        time (clamped to the keys' [0, 1]); in that space the sphere's centre is C0 + (g - t0) / (t1 - t0) (C1 - C0)
                        with g = the GATHER time (movingSphere.cu:33-39, :66). The sphere is displaced twice; the project keeps
                        that ("Moving spheres keep the reference's matrix-motion transform on top of the moving centre").
  Rectangles            t = (k - o'_k) / d'_k, a = o'_a + t d'_a, b = o'_b + t d'_b, inside when a0 <= a <= a1 and b0 <= b <= b1;
                        x-rectangle: k = x, a = y, b = z; y-rectangle: k = y, a = x, b = z; z-rectangle: k = z, a = x, b = y.
  Closest hit           the minimum over (t, primitive index) of the candidates of primitive kinds 0 to 4 (volumes are skipped).
  Shading normal        rectangle: +-axis by its flip flag, taken to world space with the transposed world -> object matrix and
                        normalised; sphere: (P_world - C_object) / r taken to world space the same way and NOT normalised - the
                        world-space point minus the object-space centre. With a rigid transform that keeps the centre
                        in place this is the true normal rotated once more.
  Texture coordinates   sphere: u = 1 - (atan2(n.z, n.x) + pi) / (2 pi), v = (asin(n.y) + pi / 2) / pi of that shading normal
                        (SURVEY Q13 again: a transformed sphere's texture turns twice); rectangle: u = (a - a0) / (a1 - a0),
                        v = (b - b0) / (b1 - b0). An image's row 0 is at v = 0, its texel centres are at (i + 0.5) / width.

Conditioning (closest_hit's mask). Which primitive wins, and at which root, is only decided where fp32 cannot flip it. A candidate
is MARGINAL, at EPS = 1e-3, when the ray passes its sphere with | |perp|^2 - r^2 | < EPS r^2, meets its rectangle's plane within
EPS * extent of an edge (inside or outside), meets it with |d_k| < EPS |d|, or has a root within EPS * t of tmin or tmax. Two
more conditions come from the error model below, because a decision inside the tolerated error is no decision: a discriminant
within 2^-21 * e_disc of zero (8 error units; a small far sphere, |oc| >> r, is grazed long before EPS r^2 says so) and a root
within 2^-21 * unit of tmin or tmax are marginal too. Marginal candidates stay in the ranking, near misses included. A ray is
ILL-CONDITIONED when its best candidate is marginal or its two best candidates lie within EPS * t (or within 2^-21 of their units)
of each other. On such a ray an fp32 implementation may miss, or end at any candidate up to and including the second one that is
not marginal ("one of the two best candidates", with the marginal ones in front of them not counted).

Error unit (first-order forward error of the reference's formula evaluated in fp32, in units of 2^-24 = half an ulp's relative
size; `e_x` is the absolute error bound of x in those units, |.| and products are per component):
  transform    e_o' = 2 (|inv_k0 o_x| + |inv_k1 o_y| + |inv_k2 o_z| + |inv_k3|), e_d' = 2 (|inv_k0 d_x| + ...); zero for the identity.
               The cancellation in inv * o + inv_3 is what dominates for the Cornell boxes.
  motion       e_o' += |o'| + 2 |mt| + |o' - mt|; the centre: e_c = 2 |C0| + 3 |s (C1 - C0)| (static sphere: 0).
  sphere       e_oc = e_o' + e_c + |oc|;  e_a = 2 sum |d| e_d + 3 a;  e_b = sum (|d| e_oc + |oc| e_d) + 3 sum |oc d|;
               e_c = 2 sum |oc| e_oc + 3 sum oc^2 + r^2 + |c|;  e_disc = 2 |b| e_b + b^2 + a e_c + |c| e_a + |a c| + |disc|;
               e_s = e_disc / (2 s) + s, s = sqrt(disc);  e_num = e_b + e_s + |num|;  unit = e_num / a + |t| e_a / a + |t|.
  rectangle    unit = (e_o'_k + |k - o'_k|) / |d'_k| + |t| e_d'_k / |d'_k| + |t|.
The tolerance of the tests is |t - t64| <= K * 2^-24 * unit.

K. MEASURED_CONSTANT below is the largest |t32 - t64| / (2^-24 * unit) between closest_hit_fp32 and closest_hit - this file
against itself at two precisions - over the well-conditioned rays of all scenes of test_geometry_cpu.py (50 000 rays each),
measured on the CPU by `python tests/geometry_ref.py`: 1.026 (per scene 0.12 to 1.03; the fp32 evaluation picks the float64
primitive on every well-conditioned ray). test_geometry_cpu.py re-measures it per scene and holds it to that value.
K = K_FACTOR * MEASURED_CONSTANT = 4.104 with K_FACTOR = 4: the oracle and the kernels use fused multiply-adds where numpy rounds
twice and another, equally valid, operation order. No absolute time and no GPU number stands behind anything here.
"""
import ctypes as C

import numpy as np

from raytracing_weekend_amd import abi

EPS = 1e-3
EPS_UNIT = 2.0 ** -21
U = 2.0 ** -24
MEASURED_CONSTANT = 1.026  # `python tests/geometry_ref.py`: the largest of the per-scene constants (random19; 1.0260 to four places)
K_FACTOR = 4.0
K = K_FACTOR * MEASURED_CONSTANT

_PRIM = np.dtype([("type", "<i4"), ("material", "<i4"), ("xform", "<i4"), ("flip", "<i4"), ("p", "<f4", 12)])
_XFORM = np.dtype([("m", "<f4", 12), ("inv", "<f4", 12)])
# rectangle kind -> (k, a, b) axes (include/rtw.h rtw_prim_type; aarectx.cu:13-18, aarecty.cu:14-19, aarectz.cu:15-20)
RECT_AXES = {abi.PRIM_RECT_X: (0, 1, 2), abi.PRIM_RECT_Y: (1, 0, 2), abi.PRIM_RECT_Z: (2, 0, 1)}


def scene_tables(blob):
    """(prims, xforms) of a scene blob as numpy record arrays."""
    h = abi.SceneHeader.from_buffer_copy(blob[:C.sizeof(abi.SceneHeader)])
    prims = np.frombuffer(blob, _PRIM, h.n_prims, h.off_prims)
    xforms = np.frombuffer(blob, _XFORM, h.n_xforms, h.off_xforms)
    return prims, xforms


def _range_state(t, unit, tmin, tmax, strict_lo, lenient):
    """(inside or marginal, marginal) of a root t against (tmin, tmax); strict_lo: tmin < t (spheres) or tmin <= t (rectangles)."""
    m = np.maximum(EPS * np.abs(t), EPS_UNIT * unit)
    near = ((np.abs(t - tmin) < m) | (np.abs(t - tmax) < m)) & lenient
    inside = ((t > tmin) if strict_lo else (t >= tmin)) & (t < tmax)
    ok = np.isfinite(t)
    return (inside | near) & ok, near & ok


def _bounds(kind, P):
    """Object-space bounding spheres of m primitives of one kind (float64), generous: they only select the pairs worth testing."""
    if kind == abi.PRIM_SPHERE:
        return P[:, 0:3], P[:, 3]
    if kind == abi.PRIM_MOVING_SPHERE:  # o' - mt against the moving centre: the centre relative to o' is 2 C0 + (s + g) (C1 - C0)
        delta = P[:, 4:7] - P[:, 0:3]
        still = P[:, 8] == P[:, 7]
        span = np.where(still, 1.0, P[:, 8] - P[:, 7])
        g_a, g_b = np.where(still, 0.0, (0.0 - P[:, 7]) / span), np.where(still, 0.0, (1.0 - P[:, 7]) / span)  # gather times in [0, 1]
        g_lo, g_hi = np.minimum(g_a, g_b), np.maximum(g_a, g_b) + 1.0                                         # + ray times in [0, 1]
        mid, half = 0.5 * (g_lo + g_hi), 0.5 * (g_hi - g_lo)
        return 2.0 * P[:, 0:3] + mid[:, None] * delta, P[:, 3] + half * np.linalg.norm(delta, axis=1)
    ik, ia, ib = RECT_AXES[kind]
    c = np.zeros((P.shape[0], 3))
    c[:, ik], c[:, ia], c[:, ib] = P[:, 4], 0.5 * (P[:, 0] + P[:, 1]), 0.5 * (P[:, 2] + P[:, 3])
    return c, 0.5 * np.hypot(P[:, 1] - P[:, 0], P[:, 3] - P[:, 2])


def _pairs(o, d, cen, rad):
    """(ray, primitive) index pairs whose line passes the bounding sphere, enlarged by 5 % and by the cancellation of the expansion
    below: a superset of the pairs that can yield a candidate, marginal ones included. Float64 whatever the precision under test."""
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    oo, od = (o * o).sum(1), (o * dn).sum(1)
    cc, rr = (cen * cen).sum(1), rad * rad
    ri, mi = [], []
    chunk = max(1, 4_000_000 // max(1, cen.shape[0]))
    for lo in range(0, o.shape[0], chunk):
        hi = min(o.shape[0], lo + chunk)
        oc2 = oo[lo:hi, None] - 2.0 * (o[lo:hi] @ cen.T) + cc[None, :]
        b = od[lo:hi, None] - dn[lo:hi] @ cen.T
        keep = oc2 - b * b <= 1.1025 * rr[None, :] + 1e-9 * (oo[lo:hi, None] + cc[None, :])
        keep |= ~np.isfinite(oc2 - b * b)
        r_, m_ = np.nonzero(keep)
        ri.append(r_ + lo)
        mi.append(m_)
    return np.concatenate(ri), np.concatenate(mi)


def _closest(blob, rays, ray_time, gather_time, ft, pairs=None):
    prims, xforms = scene_tables(blob)
    rays = np.asarray(rays, dtype=np.float32)
    n = rays.shape[0]
    rt = np.zeros(n, np.float32) if ray_time is None else np.asarray(ray_time, np.float32)
    gt = np.zeros(n, np.float32) if gather_time is None else np.asarray(gather_time, np.float32)
    found = []  # (ray, prim, t, marginal, unit) of every candidate
    pairs = {} if pairs is None else pairs  # the pairs worth testing, kept for a second evaluation of the same rays
    surface = np.nonzero(prims["type"] <= abi.PRIM_RECT_Z)[0]
    o_w, d_w = rays[:, 0:3].astype(ft), rays[:, 3:6].astype(ft)
    tmin, tmax = rays[:, 6].astype(ft), rays[:, 7].astype(ft)
    with np.errstate(all="ignore"):
        for xi in np.unique(prims["xform"][surface]):
            inv = xforms["inv"][xi].reshape(3, 4).astype(ft)
            if np.array_equal(xforms["inv"][xi].reshape(3, 4), np.eye(3, 4, dtype=np.float32)):
                o, d = o_w, d_w
                e_o, e_d = np.zeros((n, 3)), np.zeros((n, 3))
            else:
                to = o_w[:, None, :] * inv[None, :, :3]  # (n, 3, 3): term j of row k
                td = d_w[:, None, :] * inv[None, :, :3]
                o = ((to[..., 0] + to[..., 1]) + to[..., 2]) + inv[None, :, 3]
                d = (td[..., 0] + td[..., 1]) + td[..., 2]
                e_o = 2.0 * (np.abs(to).sum(-1) + np.abs(inv[None, :, 3])).astype(np.float64)
                e_d = 2.0 * np.abs(td).sum(-1).astype(np.float64)
            in_x = surface[prims["xform"][surface] == xi]
            for kind in range(5):
                ids = in_x[prims["type"][in_x] == kind]
                if ids.size == 0:
                    continue
                cen, rad = _bounds(kind, prims["p"][ids].astype(np.float64))
                if (xi, kind) not in pairs:
                    pairs[(xi, kind)] = _pairs(o.astype(np.float64), d.astype(np.float64), cen, rad)
                ri, mi = pairs[(xi, kind)]
                P = prims["p"][ids].astype(ft)[mi]
                args = (P, o[ri], d[ri], e_o[ri], e_d[ri], tmin[ri], tmax[ri])
                if kind <= abi.PRIM_MOVING_SPHERE:
                    t, flag, unit = _spheres(kind, *args, rt[ri].astype(ft), gt[ri].astype(ft), ft)
                else:
                    t, flag, unit = _rects(kind, *args, ft)
                ok = np.isfinite(t)
                found.append((ri[ok], ids[mi][ok], t[ok].astype(np.float64), flag[ok], unit[ok].astype(np.float64)))
    ray, prim, t, flag, unit = (np.concatenate([f[i] for f in found]) if found else np.zeros(0, dt)
                                for i, dt in enumerate((np.int64, np.int64, np.float64, bool, np.float64)))
    order = np.lexsort((prim, t, ray))  # by ray, then t, ties to the lower primitive index
    ray, prim, t, flag, unit = ray[order], prim[order], t[order], flag[order], unit[order]
    first = np.nonzero(np.r_[True, ray[1:] != ray[:-1]])[0] if ray.size else np.zeros(0, np.int64)
    t1, p1, f1, u1 = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, bool), np.zeros(n)
    t2, p2, u2 = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n)
    t1[ray[first]], p1[ray[first]], f1[ray[first]], u1[ray[first]] = t[first], prim[first], flag[first], unit[first]
    second = first + 1
    second = second[(second < ray.size)]
    second = second[ray[second] == ray[second - 1]]
    t2[ray[second]], p2[ray[second]], u2[ray[second]] = t[second], prim[second], unit[second]
    with np.errstate(invalid="ignore"):
        close = np.isfinite(t2) & ((t2 - t1) < np.maximum(EPS * np.abs(t1), EPS_UNIT * (u1 + u2)))
    miss = p1 < 0
    # what an fp32 evaluation may answer on an ill-conditioned ray: any candidate up to and including the second that is not marginal
    clean_before = np.cumsum(~flag) - (~flag)
    clean_before = clean_before - np.repeat(clean_before[first], np.diff(np.r_[first, ray.size])) if ray.size else clean_before
    allowed = ray[clean_before < 2] * np.int64(len(prims) + 1) + prim[clean_before < 2]
    return {"t": np.where(miss, rays[:, 7].astype(np.float64), t1), "prim": p1.astype(np.int32), "t2": t2, "prim2": p2.astype(np.int32),
            "ill": f1 | close, "unit": np.where(miss, 0.0, u1), "allowed": allowed, "n_prims": len(prims), "_pairs": pairs}


def _spheres(kind, P, o, d, e_o, e_d, tmin, tmax, rt, gt, ft):
    """One candidate per (ray, sphere) pair (rows of the arguments): t (inf: none), marginal flag, error unit."""
    lenient = ft is np.float64  # the fp32 evaluation accepts what the formula accepts: no near misses, nothing marginal
    c, r = P[:, 0:3], P[:, 3]
    e_c = 0.0
    if kind == abi.PRIM_MOVING_SPHERE:
        c0, c1, t0, t1 = P[:, 0:3], P[:, 4:7], P[:, 7], P[:, 8]
        s = np.clip(rt, ft(0.0), ft(1.0))[:, None]
        mt = c0 + s * (c1 - c0)                     # the motion transform's translation at the ray time
        o_m = o - mt
        e_o = e_o + np.abs(o) + 2 * np.abs(mt) + np.abs(o_m)
        o = o_m
        g = np.where(t1 == t0, ft(0.0), (gt - t0) / np.where(t1 == t0, ft(1.0), t1 - t0))[:, None]
        c = c0 + g * (c1 - c0)                      # the centre at the gather time
        e_c = 2 * np.abs(c0) + 3 * np.abs(g * (c1 - c0))
    oc = o - c
    e_oc = e_o + e_c + np.abs(oc)
    dd, ocd, oc2 = d * d, oc * d, oc * oc
    a = (dd[:, 0] + dd[:, 1]) + dd[:, 2]
    b = (ocd[:, 0] + ocd[:, 1]) + ocd[:, 2]
    cc = ((oc2[:, 0] + oc2[:, 1]) + oc2[:, 2]) - r * r
    disc = b * b - a * cc
    e_a = 2 * (np.abs(d) * e_d).sum(-1) + 3 * a
    e_b = (np.abs(d) * e_oc + np.abs(oc) * e_d).sum(-1) + 3 * np.abs(ocd).sum(-1)
    e_cc = 2 * (np.abs(oc) * e_oc).sum(-1) + 3 * oc2.sum(-1) + r * r + np.abs(cc)
    e_disc = 2 * np.abs(b) * e_b + b * b + a * e_cc + np.abs(cc) * e_a + np.abs(a * cc) + np.abs(disc)
    grazing = ((np.abs(disc / a) < ft(EPS) * (r * r)) | (np.abs(disc) < EPS_UNIT * e_disc)) & lenient   # disc / a = r^2 - |perp|^2
    s_ = np.sqrt(np.maximum(disc, ft(0.0)))
    e_s = e_disc / (2 * s_) + s_
    T = np.full(b.shape, np.inf, dtype=ft)
    flag = np.zeros(b.shape, bool)
    unit = np.zeros(b.shape, dtype=np.float64)
    have = np.zeros(b.shape, bool)
    real = (disc >= 0) | grazing
    for sign in (-1.0, 1.0):
        num = -b + ft(sign) * s_
        t = num / a
        un = (e_b + e_s + np.abs(num)) / a + np.abs(t) * e_a / a + np.abs(t)
        un = np.where(np.isfinite(un), un, 0.0)
        cand, near = _range_state(t, un, tmin, tmax, True, lenient)
        take = cand & real & ~have
        T = np.where(take, t, T)
        flag = np.where(take, near | grazing, flag)
        unit = np.where(take, un, unit)
        have |= take
    return T, flag, unit


def _rects(kind, P, o, d, e_o, e_d, tmin, tmax, ft):
    """One candidate per (ray, rectangle) pair: t (inf: none), marginal flag, error unit."""
    lenient = ft is np.float64
    ik, ia, ib = RECT_AXES[kind]
    a0, a1, b0, b1, k = (P[:, i] for i in range(5))
    ok, dk = o[:, ik], d[:, ik]
    t = (k - ok) / dk
    a = o[:, ia] + t * d[:, ia]
    b = o[:, ib] + t * d[:, ib]
    unit = (e_o[:, ik] + np.abs(k - ok)) / np.abs(dk) + np.abs(t) * e_d[:, ik] / np.abs(dk) + np.abs(t)
    unit = np.where(np.isfinite(unit), unit, 0.0)
    ma, mb = (ft(EPS) * (a1 - a0), ft(EPS) * (b1 - b0)) if lenient else (ft(0.0), ft(0.0))
    inside = (a >= a0 - ma) & (a <= a1 + ma) & (b >= b0 - mb) & (b <= b1 + mb)   # widened: near misses stay candidates
    edge = (np.abs(a - a0) < ma) | (np.abs(a - a1) < ma) | (np.abs(b - b0) < mb) | (np.abs(b - b1) < mb)
    flat = (np.abs(dk) < ft(EPS) * np.sqrt((d * d).sum(-1))) & lenient
    cand, near = _range_state(t, unit, tmin, tmax, False, lenient)
    take = cand & inside
    return np.where(take, t, np.inf).astype(ft), (near | edge | flat) & take, unit


def closest_hit(blob, rays, ray_time=None, gather_time=None):
    """Closest hit of every ray (n, 8: origin, direction, tmin, tmax - rtw_debug_intersect's layout) among the primitives of
    kinds 0 to 4, in float64. Returns a dict of per-ray arrays: t (tmax on a miss), prim (-1 on a miss), t2 / prim2 (the
    runner-up; inf / -1 when there is none), ill (the conditioning mask of the module docstring: True = do not trust prim),
    unit (the error unit of t, see the module docstring; the tolerance is K * 2^-24 * unit), allowed (keys ray * (n_prims + 1) + prim
    of the candidates an ill-conditioned ray may end at: its best ones up to the second that is not marginal)."""
    return _closest(blob, rays, ray_time, gather_time, np.float64)


def closest_hit_fp32(blob, rays, ray_time=None, gather_time=None):
    """The same algebra evaluated in float32: only there to measure MEASURED_CONSTANT against closest_hit."""
    return _closest(blob, rays, ray_time, gather_time, np.float32)


def error_constant(blob, rays, ray_time=None, gather_time=None, ref=None):
    """max |t32 - t64| / (2^-24 * unit) over the well-conditioned rays that hit, and how many fp32 primitives differ there."""
    ref = closest_hit(blob, rays, ray_time, gather_time) if ref is None else ref
    f32 = _closest(blob, rays, ray_time, gather_time, np.float32, ref["_pairs"])
    good = ~ref["ill"] & (ref["prim"] >= 0)
    same = f32["prim"][good] == ref["prim"][good]
    err = np.abs(f32["t"][good].astype(np.float64) - ref["t"][good]) / (U * ref["unit"][good])
    return (float(err[same].max()) if same.any() else 0.0), int((~same).sum())


# ---------------------------------------------------------------- shading normal and texture coordinates
def _object_point(xf, point):
    inv = xf["inv"].reshape(3, 4).astype(np.float64)
    return point @ inv[:, :3].T + inv[:, 3]


def shading_normal(blob, prim, point):
    """World-space shading normal at world-space hit points `point` (n, 3) of primitive `prim`, float64."""
    prims, xforms = scene_tables(blob)
    pr = prims[prim]
    point = np.asarray(point, np.float64)
    inv = xforms[pr["xform"]]["inv"].reshape(3, 4).astype(np.float64)[:, :3]
    p = pr["p"].astype(np.float64)
    if pr["type"] == abi.PRIM_SPHERE:
        n_obj = (point - p[0:3]) / p[3]        # the WORLD-space point minus the OBJECT-space centre
        return n_obj @ inv                     # transposed world -> object matrix; not normalised (sphere.cu:63-67)
    if pr["type"] in RECT_AXES:
        n_obj = np.zeros(3)
        n_obj[RECT_AXES[int(pr["type"])][0]] = -1.0 if pr["flip"] else 1.0
        n = n_obj @ inv
        return np.broadcast_to(n / np.linalg.norm(n), point.shape).copy()
    raise ValueError("shading_normal: spheres and rectangles only")


def surface_uv(blob, prim, point):
    """Texture coordinates (u, v) at world-space hit points `point` (n, 3) of primitive `prim` (a sphere or a rectangle), float64."""
    prims, xforms = scene_tables(blob)
    pr = prims[prim]
    point = np.asarray(point, np.float64)
    p = pr["p"].astype(np.float64)
    if pr["type"] == abi.PRIM_SPHERE:
        n = shading_normal(blob, prim, point)  # get_sphere_uv takes the shading normal (sphere.cu:69), Q13 and all
        phi = np.arctan2(n[:, 2], n[:, 0])
        theta = np.arcsin(np.clip(n[:, 1], -1.0, 1.0))
        return 1.0 - (phi + np.pi) / (2.0 * np.pi), (theta + np.pi / 2.0) / np.pi
    if pr["type"] in RECT_AXES:
        _, ia, ib = RECT_AXES[int(pr["type"])]
        q = _object_point(xforms[pr["xform"]], point)
        return (q[:, ia] - p[0]) / (p[1] - p[0]), (q[:, ib] - p[2]) / (p[3] - p[2])
    raise ValueError("surface_uv: spheres and rectangles only")


def ramp_image(w, h):
    """Texture data of an RTW_TEX_IMAGE (width, height, then texels r | g << 8 | b << 16 | a << 24, row 0 first): red ramps with
    the column, round(255 (i + 0.5) / w), green with the row, round(255 (j + 0.5) / h). A bilinear fetch with texel centres at
    (i + 0.5) / w then returns red = u and green = v to within half an 8-bit step (between the outermost texel centres)."""
    red = np.rint(255.0 * (np.arange(w) + 0.5) / w).astype(np.uint32)
    green = np.rint(255.0 * (np.arange(h) + 0.5) / h).astype(np.uint32)
    texels = red[None, :] | (green[:, None] << 8) | np.uint32(255 << 24)
    return np.array([w, h], "<u4").tobytes() + texels.astype("<u4").tobytes()


def camera_rays(hdr, s, t):
    """Perspective camera at lens radius 0 (shaders/camera.cu:11-19): origin, direction = lower_left + s horizontal + t vertical
    - origin, float64, for arrays s, t of image-plane coordinates (pixel x's samples have s in [x / w, (x + 1) / w))."""
    cam = hdr.camera
    o = np.array(list(cam.origin), np.float64)
    ll, hz, vt = (np.array(list(v), np.float64) for v in (cam.lower_left, cam.horizontal, cam.vertical))
    d = ll + np.asarray(s)[..., None] * hz + np.asarray(t)[..., None] * vt - o
    return np.broadcast_to(o, d.shape).copy(), d


# ---------------------------------------------------------------- the scenes and rays of the geometry tests
def rigid_xform(axis, deg, translation):
    """rtw_xform of a rotation by deg about coordinate axis `axis` followed by a translation: m = T R, inv = (T R)^-1, rounded to fp32."""
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(4)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    m[:3, 3] = translation
    mi = np.linalg.inv(m)
    x = abi.Xform()
    for k in range(12):
        x.m[k] = float(np.float32(m[k // 4, k % 4]))
        x.inv[k] = float(np.float32(mi[k // 4, k % 4]))
    return x


def identity_xform():
    return rigid_xform(0, 0.0, (0.0, 0.0, 0.0))


SINGLE_PRIMS = {  # kind -> p[]; sizes of a few units, nothing centred on the origin or on an axis
    "sphere": (abi.PRIM_SPHERE, (3.0, -2.0, 5.0, 2.5)),
    "moving_sphere": (abi.PRIM_MOVING_SPHERE, (3.0, -2.0, 5.0, 2.0, 4.5, -1.0, 4.0, 0.25, 1.5)),
    "rect_x": (abi.PRIM_RECT_X, (-3.0, 4.0, 1.0, 6.0, 2.0)),
    "rect_y": (abi.PRIM_RECT_Y, (-3.0, 4.0, 1.0, 6.0, 2.0)),
    "rect_z": (abi.PRIM_RECT_Z, (-3.0, 4.0, 1.0, 6.0, 2.0)),
}
SINGLE_XFORMS = {"identity": None, "rot_x": (0, 25.0, (1.5, -4.0, 2.0)), "rot_y": (1, -40.0, (-3.0, 0.5, 6.0)), "rot_z": (2, 60.0, (2.0, 3.0, -5.0))}


def single_prim_scene(kind, xform):
    """One primitive alone (SINGLE_PRIMS[kind]) under SINGLE_XFORMS[xform]; one lambertian material, sky on."""
    ptype, params = SINGLE_PRIMS[kind]
    hdr = abi.SceneHeader()
    hdr.magic, hdr.version, hdr.sky_light = abi.RTW_SCENE_MAGIC, abi.RTW_SCENE_VERSION, 1
    xforms = [identity_xform()]
    pr = abi.Prim(type=ptype, material=0, xform=0, flip=0)
    for i, v in enumerate(params):
        pr.p[i] = v
    if SINGLE_XFORMS[xform] is not None:
        xforms.append(rigid_xform(*SINGLE_XFORMS[xform]))
        pr.xform = 1
    return abi.assemble_scene({"header": hdr, "prims": [pr], "xforms": xforms, "lights": [],
                               "materials": [abi.Material(type=abi.MAT_LAMBERTIAN, texture=0, fuzz_or_eta=0.0, bsdf_eval=0)],
                               "textures": [abi.Texture(type=abi.TEX_CONSTANT)]})


def _multi_scenes():
    import oracle  # scene builders only (pure Python): the oracle library is not loaded here
    w = h = 32
    out = {f"scene{s}": (lambda s=s: abi.build_scene(s, w, h)) for s in (0, 1, 2, 4)}
    out["cluttered_cornell"] = lambda: oracle.cluttered_cornell(w, h)
    out["random19"] = lambda: oracle.random_scene(19, w, h, n_prims=300)
    out["random16_motion"] = lambda: oracle.random_scene(16, w, h, n_prims=80, motion=True)
    return out


SCENES = {f"{k}-{x}": (lambda k=k, x=x: single_prim_scene(k, x)) for k in SINGLE_PRIMS for x in SINGLE_XFORMS}
SCENES.update(_multi_scenes())
N_RAYS = 50_000
RAY_SEED = 1


def bounding_spheres(blob):
    """World-space bounding spheres (centre (n, 3), radius (n,)) of the surface primitives, and their indices."""
    prims, xforms = scene_tables(blob)
    ids = np.nonzero(prims["type"] <= abi.PRIM_RECT_Z)[0]
    cen, rad = np.zeros((ids.size, 3)), np.zeros(ids.size)
    for n_, i in enumerate(ids):
        c, r = _bounds(int(prims["type"][i]), prims["p"][i:i + 1].astype(np.float64))
        m = xforms["m"][prims["xform"][i]].reshape(3, 4).astype(np.float64)
        cen[n_], rad[n_] = m[:, :3] @ c[0] + m[:, 3], r[0]
    return cen, rad, ids


def scene_rays(blob, seed, n=N_RAYS):
    """The ray mix of the traversal tests: origins inside and around the content, unnormalised directions of length 0.2 to 12
    (half of them aimed into the inner 60 % of a random primitive's bounding sphere), every seventh ray with a finite tmax, random ray and gather
    times. Returns (rays (n, 8) float32, ray_time, gather_time)."""
    rng = np.random.default_rng(seed)
    cen, rad, _ = bounding_spheres(blob)
    lo, hi = np.percentile(cen - rad[:, None], 5, axis=0), np.percentile(cen + rad[:, None], 95, axis=0)
    if len(rad) == 1:
        lo, hi = cen[0] - 4.0 * rad[0], cen[0] + 4.0 * rad[0]
    pad = 0.15 * float(np.max(hi - lo))
    o = rng.uniform(lo - pad, hi + pad, (n, 3))
    d = rng.normal(size=(n, 3))
    pick = rng.integers(0, len(rad), n // 2)
    inside = rng.normal(size=(n // 2, 3))
    inside *= (rng.uniform(0, 1, (n // 2, 1)) ** (1 / 3)) / np.linalg.norm(inside, axis=1, keepdims=True)
    d[: n // 2] = cen[pick] + 0.6 * rad[pick, None] * inside - o[: n // 2]
    d *= rng.uniform(0.2, 12.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 1e-6), np.full((n, 1), 1e27)], axis=1).astype(np.float32)
    scale = float(np.linalg.norm(hi - lo))
    rays[::7, 7] = rng.uniform(0.0005 * scale / 12.0, scale / 12.0, len(rays[::7]))  # finite tmax like shadow probes
    return rays, rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)


def check_against(name, ref, t, prim, kinds_needed=None):
    """The assertions of the geometry tests for one scene: (t, prim) of an fp32 implementation against closest_hit's `ref`.
    Returns the figures (excluded share, hit share, largest error in units) for the caller to print."""
    assert K > 0.0
    ill, good = ref["ill"], ~ref["ill"]
    excluded, hits = float(ill.mean()), float((ref["prim"] >= 0).mean())
    hit = good & (ref["prim"] >= 0)
    err = np.abs(t[hit].astype(np.float64) - ref["t"][hit]) / (U * ref["unit"][hit])
    worst = float(err.max()) if hit.any() else 0.0
    fig = f"{name}: excluded {100 * excluded:.2f} %, hits {100 * hits:.1f} %, largest |t - t64| = {worst:.2f} units (K = {K:g})"
    wrong = np.nonzero(good & (prim != ref["prim"]))[0]
    assert wrong.size == 0, f"{fig}; primitive differs on {wrong.size} well-conditioned rays, first {wrong[:5]}: got {prim[wrong[:5]]}, reference {ref['prim'][wrong[:5]]}"
    assert worst <= K, f"{fig}; ray {np.nonzero(hit)[0][int(err.argmax())]}"
    miss = good & (ref["prim"] < 0)
    assert np.array_equal(t[miss], ref["t"][miss].astype(np.float32)), f"{fig}; a miss does not return tmax"
    odd = ill & (prim != -1) & ~np.isin(np.arange(len(prim), dtype=np.int64) * (ref["n_prims"] + 1) + prim, ref["allowed"])
    assert not odd.any(), f"{fig}; {int(odd.sum())} ill-conditioned rays hit none of the best candidates, first {np.nonzero(odd)[0][:5]}"
    assert excluded <= 0.10 and hits >= 0.20, fig
    return fig


# ---------------------------------------------------------------- the texture-coordinate scene
TEX_W = TEX_H = 96
TEX_SIZE = 256  # texels per side of the ramp: half a texel (the clamp at the border) stays below half an 8-bit step


def texture_scene(w=TEX_W, h=TEX_H):
    """Six emitters showing one ramp_image texture, seen by the Cornell box's perspective camera (at (278, 278, -800), looking
    along +z, lens radius 0) without overlapping: a sphere, one rectangle of each axis, and a sphere and a z-rectangle under
    rigid transforms. The transformed sphere's transform keeps its centre in place (rotation about the centre), so that the
    reference's shading normal stays a unit vector: the true normal turned once more."""
    parts = dict(abi.parse_scene(abi.build_scene(0, w, h)))
    hdr = abi.SceneHeader.from_buffer_copy(bytes(parts["header"]))
    hdr.sky_light = 0
    hdr.camera.lens_radius = 0.0
    c_b = np.array([430.0, 200.0, 250.0])
    rot_b = rigid_xform(2, 25.0, (0.0, 0.0, 0.0))
    r3 = np.array(list(rot_b.m), np.float64).reshape(3, 4)[:, :3]
    xforms = [identity_xform(), rigid_xform(2, 25.0, c_b - r3 @ c_b), rigid_xform(1, 30.0, (230.0, 215.0, 300.0))]

    def prim(ptype, params, xf=0, flip=0):
        pr = abi.Prim(type=ptype, material=0, xform=xf, flip=flip)
        for i, v in enumerate(params):
            pr.p[i] = v
        return pr
    prims = [prim(abi.PRIM_SPHERE, (140.0, 420.0, 200.0, 95.0)),
             prim(abi.PRIM_RECT_X, (40.0, 270.0, 50.0, 450.0, 20.0)),
             prim(abi.PRIM_RECT_Y, (200.0, 430.0, 50.0, 450.0, 30.0)),
             prim(abi.PRIM_RECT_Z, (330.0, 540.0, 330.0, 540.0, 400.0), flip=1),
             prim(abi.PRIM_SPHERE, (c_b[0], c_b[1], c_b[2], 80.0), xf=1),
             prim(abi.PRIM_RECT_Z, (-85.0, 85.0, -75.0, 75.0, 0.0), xf=2, flip=1)]
    parts.update(header=hdr, prims=prims, xforms=xforms, lights=[], texdata=ramp_image(TEX_SIZE, TEX_SIZE),
                 materials=[abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=0, fuzz_or_eta=0.0, bsdf_eval=-1)],
                 textures=[abi.Texture(type=abi.TEX_IMAGE, data=0)])
    return abi.assemble_scene(parts)


def uv_expectation(blob, w=TEX_W, h=TEX_H):
    """What the red and green channels of an emitter picture of `blob` (ramp texture, perspective camera, one sample per pixel)
    may be, from float64 alone: the rays through the (w + 1) x (h + 1) pixel corners are intersected by closest_hit, the hit
    points go through surface_uv and shading_normal, and a pixel - whose jittered sample lies between its corners - gets
    [min, max] of its four corner values, widened by one 8-bit step. Returns a dict of (h, w) arrays: prim (the primitive all
    four corners hit, else -1), touched (h, w, n_prims: some corner hits that primitive), checked, lo / hi (h, w, 2: red, green).
    Not checked: pixels whose corners do not all hit one primitive, that straddle a sphere's seam (u jumps), that lie within 5
    degrees of a pole, or whose corners disagree on which face the shading normal shows; where all four show the back the
    emitter is dark (front-face rule: dot(n, d) < 0) and lo = hi = 0."""
    hdr = abi.SceneHeader.from_buffer_copy(blob[:C.sizeof(abi.SceneHeader)])
    prims, _ = scene_tables(blob)
    ys, xs = np.mgrid[0:h + 1, 0:w + 1]
    o, d = camera_rays(hdr, xs.ravel() / w, ys.ravel() / h)
    rays = np.concatenate([o, d, np.full((o.shape[0], 1), 1e-6), np.full((o.shape[0], 1), 1e27)], axis=1)
    hit = closest_hit(blob, rays.astype(np.float32))  # (the corner rays round to fp32 here; a pixel is 1e5 times coarser)
    point = o + hit["t"][:, None] * d
    u, v, front = np.zeros(len(o)), np.zeros(len(o)), np.zeros(len(o), bool)
    for i in range(len(prims)):
        m = hit["prim"] == i
        if m.any():
            u[m], v[m] = surface_uv(blob, i, point[m])
            front[m] = (shading_normal(blob, i, point[m]) * d[m]).sum(1) < 0.0
    shape = (h + 1, w + 1)

    def corners(a):
        a = a.reshape(shape)
        return np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]], axis=-1)
    cp, cu, cv, cf, ci = corners(hit["prim"]), corners(u), corners(v), corners(front), corners(hit["ill"])
    same = (cp == cp[..., :1]).all(-1) & (cp[..., 0] >= 0) & ~ci.any(-1)
    prim = np.where(same, cp[..., 0], -1)
    is_sphere = np.isin(prim, np.nonzero(prims["type"] == abi.PRIM_SPHERE)[0])
    seam = is_sphere & (cu.max(-1) - cu.min(-1) > 0.5)
    pole = is_sphere & ((cv.min(-1) < 5.0 / 180.0) | (cv.max(-1) > 1.0 - 5.0 / 180.0))
    mixed_face = cf.any(-1) & ~cf.all(-1)
    checked = same & ~seam & ~pole & ~mixed_face
    lit = cf.all(-1)[..., None]
    step = 1.0 / 255.0
    lo = np.where(lit, np.stack([cu.min(-1), cv.min(-1)], -1) - step, 0.0)
    hi = np.where(lit, np.stack([cu.max(-1), cv.max(-1)], -1) + step, 0.0)
    touched = np.stack([(cp == i).any(-1) for i in range(len(prims))], axis=-1)
    return {"prim": prim, "touched": touched, "checked": checked, "lo": lo, "hi": hi, "lit": lit[..., 0]}


def check_uv(exp, rgb, what):
    """Red and green of a picture (h, w, >= 2) of texture_scene against uv_expectation's `exp`."""
    n_prims = exp["touched"].shape[-1]
    for i in range(n_prims):
        mine = exp["touched"][..., i]
        kept = exp["checked"] & (exp["prim"] == i)
        assert kept.sum() >= 50 and kept.sum() >= 0.75 * mine.sum(), f"primitive {i}: {kept.sum()} of {mine.sum()} pixels checked"
        assert (kept & exp["lit"]).sum() >= 50, f"primitive {i}: {(kept & exp['lit']).sum()} lit pixels"
    c = exp["checked"]
    got = np.asarray(rgb, np.float64)[..., :2]
    bad = c[..., None] & ((got < exp["lo"]) | (got > exp["hi"]))
    where = np.argwhere(bad)
    assert not bad.any(), (f"{what}: {len(where)} channel values outside the reference's range, first (row, column, channel) "
                           f"{where[:4].tolist()}: got {got[bad][:4]}, allowed {exp['lo'][bad][:4]} .. {exp['hi'][bad][:4]}, "
                           f"primitives {exp['prim'][bad.any(-1)][:4]}")


if __name__ == "__main__":  # the measurement behind MEASURED_CONSTANT
    worst = 0.0
    for name_, make_ in SCENES.items():
        blob_ = make_()
        rays_, rt_, gt_ = scene_rays(blob_, RAY_SEED)
        ref_ = closest_hit(blob_, rays_, rt_, gt_)
        c_, differ_ = error_constant(blob_, rays_, rt_, gt_, ref_)
        worst = max(worst, c_)
        print(f"{name_:26s} excluded {100 * ref_['ill'].mean():5.2f} %  hits {100 * (ref_['prim'] >= 0).mean():5.1f} %  constant {c_:.4f}  fp32 primitive differs on {differ_}")
    print(f"MEASURED_CONSTANT = {worst:.4f}")
