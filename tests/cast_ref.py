"""A float64 reading of what rtw_cast returns beside t and prim - material, shading normal, front flag, texture coordinates - at
the point p = o + t d of a ray's hit, with the tolerances an fp32 implementation is held to. It builds on geometry_ref.py
(shading_normal, surface_uv: static spheres and rectangles) and adds the moving sphere; like that file it is written from
include/rtw.h and the reference's intersection programs (geometry/sphere.cu:63-69, movingSphere.cu:33-39 and :83-90,
shaders/aarect{x,y,z}.cu:25-34), not from the kernels. Shared by test_cast_cpu.py and test_gpu_cast.py.

What is modelled (geometry_ref.py's docstring has the static cases)
  Moving sphere   normal = ((P_world - C(g)) / r) taken to world space with the transposed world -> object matrix, not normalised;
                  C(g) = C0 + (g - t0) / (t1 - t0) (C1 - C0) is the centre at the GATHER time g (C0 when t0 = t1). The motion
                  transform of the ray time moves points, not normals, and P_world is the world ray at t: it does not enter.
                  u, v from that normal as for a sphere.
  Front flag      dot(normal, d) < 0 (closehit's front-face rule).
  Material        prims[prim].material.
  Miss            zeros (material -1).

Error units (first-order forward error of these formulae in fp32, in units of 2^-24, per component k; |.| per component):
  sphere normal   unit_obj_k = (|p_k| + 3 |p_k - c_k| + e_c_k) / r, with e_c = 2 |C0| + 3 |g (C1 - C0)| for a moving centre
                  (geometry_ref's e_c), else 0; under a transform unit_k = sum_j unit_obj_j |inv_jk| (carried through |inv|^T).
  rectangle normal identity transform: 0, the normal is exactly +-axis. Else 4: a row of inv normalised in fp32 (three squares, two
                  sums, a root, a division on components of at most 1).
  rectangle uv    (e_q + |q_a| + |q_a - a0|) / |a1 - a0|, q the object-space hit point; e_q is the error of the object-space ray
                  evaluated at t as geometry_ref states it: e_o'_a + |t| e_d'_a = 2 (sum_j |inv_aj o_j| + |inv_a3|) + 2 |t| sum_j |inv_aj d_j|,
                  zero for the identity (the reference's rectangle programs take the point from the object-space ray).
  sphere uv       the normal's units through the first derivatives, plus 1 for the function itself:
                  u: (|n_x| unit_z + |n_z| unit_x) / (2 pi (n_x^2 + n_z^2)) + 1;  v: unit_y / (pi sqrt(1 - n_y^2)) + 1, the root floored
                  at sqrt(2^-24 unit_y): beyond |n_y| = 1 asin is clamped and a step of size e moves it by sqrt(2 e), not e / 0.
                  u is compared modulo 1 (the seam at n_z = 0, n_x < 0 joins 0 and 1).
  Off the poles   sphere uv is only checked where n_x^2 + n_z^2 >= 1e-2 |n|^2 (`pole` below marks the others).
The tolerance of the tests is |x - x64| <= K_FACTOR * C * 2^-24 * unit with C the measured constant of its kind.

Measured constants. C is the largest |x32 - x64| / (2^-24 unit) between these formulae evaluated in numpy float32 and in float64,
both at the float64 reference's t rounded to fp32, over the well-conditioned hits of the seven scenes of test_gpu_cast.py
(CAST_SCENES, 20 000 rays each at geometry_ref.RAY_SEED), measured on the CPU by `python tests/cast_ref.py`:
  C_NORMAL = 0.969 (per scene 0.05 to 0.97), C_UV_RECT = 1.575 (0.36 to 1.57), C_UV_SPHERE = 1.130 (0.77 to 1.13)
(at fp32 the point is formed with one rounding, see evaluate(); rounded twice, the Cornell box's rectangle uv alone measures 152:
the units have no |t d_k| term, and beyond ~100 an error model lacks one). That single rounding is a choice, and not one rtw.h
makes: rtw.h says p = o + t d and no more. It is taken because every implementation here forms the point with a fused
multiply-add (the oracle and the kernels alike), so the tolerances below hold an implementation that fuses this one product; one
that rounds t d first would need the |t d_k| term added to every unit before it could be held to them.
test_cast_cpu.py re-measures them per scene and holds them to these values. K_FACTOR = 4 is geometry_ref's factor for
geometry_ref's reason: the kernels fuse multiply-adds and use another, equally valid, operation order. No GPU number stands
behind anything here.
"""
import numpy as np

import geometry_ref as G
from raytracing_weekend_amd import abi

U = G.U
K_FACTOR = G.K_FACTOR
C_NORMAL = 0.969
C_UV_RECT = 1.575
C_UV_SPHERE = 1.130
POLE = 1e-2
N_RAYS = 20_000
CAST_SCENES = ("sphere-rot_x", "moving_sphere-rot_y", "rect_y-rot_z", "scene0", "cluttered_cornell", "random19", "random16_motion")
_SPHERES = (abi.PRIM_SPHERE, abi.PRIM_MOVING_SPHERE)


def _is_identity(xf):
    return np.array_equal(xf["inv"].reshape(3, 4), np.eye(3, 4, dtype=np.float32))


def _centre(pr, g, ft):
    """Centre of a sphere (n, 3) and its error bound in units: static, or the moving sphere's at gather times g."""
    P = pr["p"].astype(ft)
    c = np.broadcast_to(P[0:3], (len(g), 3))
    if pr["type"] != abi.PRIM_MOVING_SPHERE or P[7] == P[8]:
        return c, np.zeros((len(g), 3))
    s = ((g.astype(ft) - P[7]) / (P[8] - P[7]))[:, None]
    step = s * (P[4:7] - P[0:3])
    return P[0:3] + step, (2.0 * np.abs(P[0:3]) + 3.0 * np.abs(step)).astype(np.float64)


def _sphere_uv(n, ft):
    pi = ft(np.pi)
    phi = np.arctan2(n[:, 2], n[:, 0])
    theta = np.arcsin(np.clip(n[:, 1], ft(-1.0), ft(1.0)))
    return np.stack([ft(1.0) - (phi + pi) / (ft(2.0) * pi), (theta + pi / ft(2.0)) / pi], axis=1)


def evaluate(blob, rays, t, prim, gather_time=None, ft=np.float64):
    """The formulae of the module docstring in precision ft, every kind of surface primitive in this one place: (normal (n, 3),
    uv (n, 2)) at p = o + t d of the rays whose prim is >= 0, zeros elsewhere. ft = float32 is only there to measure the constants."""
    prims, xforms = G.scene_tables(blob)
    rays = np.asarray(rays, np.float32)
    n = len(rays)
    gt = np.zeros(n, np.float32) if gather_time is None else np.asarray(gather_time, np.float32)
    # the point enters with ONE rounding (the units' |p_k| term): o + t d is formed in float64, where the product of two fp32 numbers
    # is exact, and then rounded to ft - a fused multiply-add. A point rounded twice would need a |t d_k| term in every unit.
    p = (rays[:, 0:3].astype(np.float64) + np.asarray(t, np.float32).astype(np.float64)[:, None] * rays[:, 3:6].astype(np.float64)).astype(ft)
    normal, uv = np.zeros((n, 3), ft), np.zeros((n, 2), ft)
    with np.errstate(all="ignore"):
        for i in np.unique(prim[prim >= 0]):
            m = prim == i
            pr = prims[i]
            P = pr["p"].astype(ft)
            ident = _is_identity(xforms[pr["xform"]])
            inv = xforms[pr["xform"]]["inv"].reshape(3, 4).astype(ft)
            if pr["type"] in _SPHERES:
                c, _ = _centre(pr, gt[m], ft)
                no = (p[m] - c) / P[3]
                nw = no if ident else (no[:, 0:1] * inv[0, :3] + no[:, 1:2] * inv[1, :3]) + no[:, 2:3] * inv[2, :3]
                normal[m], uv[m] = nw, _sphere_uv(nw, ft)
            else:
                ik, ia, ib = G.RECT_AXES[int(pr["type"])]
                row = inv[ik, :3] * ft(-1.0 if pr["flip"] else 1.0)
                normal[m] = row if ident else row / np.sqrt((row[0] * row[0] + row[1] * row[1]) + row[2] * row[2])
                q = p[m] if ident else ((p[m][:, 0:1] * inv[:, 0] + p[m][:, 1:2] * inv[:, 1]) + p[m][:, 2:3] * inv[:, 2]) + inv[:, 3]
                uv[m] = np.stack([(q[:, ia] - P[0]) / (P[1] - P[0]), (q[:, ib] - P[2]) / (P[3] - P[2])], axis=1)
    return normal, uv


def reference(blob, rays, t, prim, gather_time=None):
    """What rtw_cast's attribute outputs should be for hits (t, prim) of `rays`, in float64 at p = o + t d. A dict of per-ray
    arrays: material (n,), normal (n, 3), dot (n,: normal . d), uv (n, 2), the error units unit_n (n, 3) and unit_uv (n, 2), sphere
    (n,: the hit is a sphere), pole (n,: a sphere hit whose uv is not checked), exact_normal (n,: a rectangle under the identity).
    Static spheres and rectangles come from geometry_ref.shading_normal / surface_uv; the moving sphere is added here."""
    prims, xforms = G.scene_tables(blob)
    rays = np.asarray(rays, np.float32)
    n = len(rays)
    prim = np.asarray(prim)
    gt = np.zeros(n, np.float32) if gather_time is None else np.asarray(gather_time, np.float32)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    t64 = np.asarray(t, np.float32).astype(np.float64)
    p = o + t64[:, None] * d
    normal, uv = evaluate(blob, rays, t, prim, gt, np.float64)  # (the moving sphere's rows stay; the others are replaced below)
    unit_n, unit_uv = np.zeros((n, 3)), np.zeros((n, 2))
    material = np.full(n, -1, np.int32)
    sphere, pole, exact = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in np.unique(prim[prim >= 0]):
            m = prim == i
            pr = prims[i]
            P = pr["p"].astype(np.float64)
            material[m] = pr["material"]
            ident = _is_identity(xforms[pr["xform"]])
            ainv = np.abs(xforms[pr["xform"]]["inv"].reshape(3, 4).astype(np.float64))
            if pr["type"] != abi.PRIM_MOVING_SPHERE:
                normal[m] = G.shading_normal(blob, i, p[m])
                uv[m] = np.stack(G.surface_uv(blob, i, p[m]), axis=1)
            if pr["type"] in _SPHERES:
                c, e_c = _centre(pr, gt[m], np.float64)
                uo = (np.abs(p[m]) + 3.0 * np.abs(p[m] - c) + e_c) / abs(P[3])
                un = uo if ident else uo @ ainv[:, :3]
                nw = normal[m]
                flat2 = nw[:, 0] ** 2 + nw[:, 2] ** 2
                root = np.sqrt(np.maximum(1.0 - nw[:, 1] ** 2, U * un[:, 1]))
                unit_n[m] = un
                unit_uv[m] = np.stack([(np.abs(nw[:, 0]) * un[:, 2] + np.abs(nw[:, 2]) * un[:, 0]) / (2.0 * np.pi * flat2) + 1.0,
                                       un[:, 1] / (np.pi * root) + 1.0], axis=1)
                sphere[m] = True
                pole[m] = ~(flat2 >= POLE * (flat2 + nw[:, 1] ** 2))
            else:
                _, ia, ib = G.RECT_AXES[int(pr["type"])]
                unit_n[m] = 0.0 if ident else 4.0
                exact[m] = ident
                q = p[m] if ident else p[m] @ xforms[pr["xform"]]["inv"].reshape(3, 4).astype(np.float64)[:, :3].T + xforms[pr["xform"]]["inv"].reshape(3, 4).astype(np.float64)[:, 3]
                cols = []
                for a, lo, hi in ((ia, P[0], P[1]), (ib, P[2], P[3])):
                    e_q = 0.0 if ident else 2.0 * ((np.abs(o[m]) * ainv[a, :3]).sum(1) + ainv[a, 3]) + 2.0 * np.abs(t64[m]) * (np.abs(d[m]) * ainv[a, :3]).sum(1)
                    cols.append((e_q + np.abs(q[:, a]) + np.abs(q[:, a] - lo)) / abs(hi - lo))
                unit_uv[m] = np.stack(cols, axis=1)
    return {"material": material, "normal": normal, "dot": (normal * d).sum(1), "uv": uv, "unit_n": unit_n, "unit_uv": unit_uv,
            "sphere": sphere, "pole": pole, "exact_normal": exact}


def uv_difference(uv, ref):
    """|uv - uv64| per component; a sphere's u modulo 1 (the seam joins u = 0 and u = 1)."""
    diff = np.abs(np.asarray(uv, np.float64) - ref["uv"])
    diff[:, 0] = np.where(ref["sphere"], np.minimum(diff[:, 0], np.abs(1.0 - diff[:, 0])), diff[:, 0])
    return diff


def tolerances(ref):
    """(normal (n, 3), uv (n, 2)) absolute tolerances of the module docstring for reference()'s `ref`."""
    tol_uv = K_FACTOR * np.where(ref["sphere"], C_UV_SPHERE, C_UV_RECT)[:, None] * U * ref["unit_uv"]
    return K_FACTOR * C_NORMAL * U * ref["unit_n"], tol_uv


def front_margin(ref, rays):
    """The front flag is decided where |normal . d| exceeds this: the normal's tolerance against |d| per component, and the dot
    product's own three roundings."""
    d = np.abs(np.asarray(rays, np.float32)[:, 3:6].astype(np.float64))
    return (tolerances(ref)[0] * d).sum(1) + K_FACTOR * 3.0 * U * (np.abs(ref["normal"]) * d).sum(1)


def measure(blob, rays, ray_time, gather_time, hit=None):
    """The three constants of one scene: fp32 against float64 at the float64 reference's t (rounded to fp32) on the well-conditioned
    hits, sphere uv off the poles. Returns ((c_normal, c_uv_rect, c_uv_sphere), share of sphere hits left out at the poles)."""
    hit = G.closest_hit(blob, rays, ray_time, gather_time) if hit is None else hit
    good = ~hit["ill"] & (hit["prim"] >= 0)
    prim = np.where(good, hit["prim"], -1)
    t = hit["t"].astype(np.float32)
    ref = reference(blob, rays, t, prim, gather_time)
    n32, uv32 = evaluate(blob, rays, t, prim, gather_time, np.float32)
    with np.errstate(all="ignore"):
        rn = np.abs(n32.astype(np.float64) - ref["normal"]) / (U * ref["unit_n"])
        ruv = uv_difference(uv32, ref) / (U * ref["unit_uv"])
    rn = np.where(ref["unit_n"] > 0.0, rn, 0.0)[good]  # (unit 0: exact, asserted by the tests on its own)
    rect, sph = good & ~ref["sphere"], good & ref["sphere"] & ~ref["pole"]
    assert not (np.abs(n32.astype(np.float64) - ref["normal"])[good & ref["exact_normal"]] != 0.0).any()
    c = (float(rn.max()) if rn.size else 0.0, float(ruv[rect].max()) if rect.any() else 0.0, float(ruv[sph].max()) if sph.any() else 0.0)
    n_sph = int((good & ref["sphere"]).sum())
    return c, (float((good & ref["pole"]).sum()) / n_sph if n_sph else 0.0)


if __name__ == "__main__":  # the measurement behind the constants
    worst = [0.0, 0.0, 0.0]
    for name_ in CAST_SCENES:
        blob_ = G.SCENES[name_]()
        rays_, rt_, gt_ = G.scene_rays(blob_, G.RAY_SEED, N_RAYS)
        c_, poles_ = measure(blob_, rays_, rt_, gt_)
        worst = [max(a, b) for a, b in zip(worst, c_)]
        print(f"{name_:22s} normal {c_[0]:.4f}  rect uv {c_[1]:.4f}  sphere uv {c_[2]:.4f}  sphere hits at the poles {100 * poles_:.2f} %")
    print("C_NORMAL = %.4f  C_UV_RECT = %.4f  C_UV_SPHERE = %.4f" % tuple(worst))
