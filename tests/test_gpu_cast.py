"""GPU suite of the ray queries (include/rtw.h rtw_cast / rtw_cast_device): t and prim against the oracle's and
rtw_debug_intersect's bits and geometry_ref's float64 reading, the attributes against cast_ref's, the occlusion mode against the
closest-hit mode, batch shapes, the torch path, one batch beyond 2^29 rays, errors, groups and sessions."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import cast_ref as R
import geometry_ref as G
import gpu_common
import oracle
from gpu_common import UPLOADS_LDS as UPLOADS, check_stream_order, gpu, left_alone, same_dict as same  # noqa: F401
from gpu_common import sentinel_stats, to_numpy, words as bits
from raytracing_weekend_amd import abi
from raytracing_weekend_amd.torch_cast import cast_torch

pytestmark = pytest.mark.gpu

ALL = ("t", "prim", "material", "normal", "uv")


upload = functools.partial(gpu_common.upload, knobs=("RTW_BRUTE_MAX", "RTW_LDS_KB", "RTW_CAST_CHUNK"))


@functools.lru_cache(maxsize=None)
def case(name):
    """(blob, rays, ray times, gather times, float64 reference, oracle t, oracle prim) of one scene of test 1, computed once."""
    blob = G.SCENES[name]()
    rays, rt, gt = G.scene_rays(blob, G.RAY_SEED, R.N_RAYS)
    return (blob, rays, rt, gt, G.closest_hit(blob, rays, rt, gt)) + oracle.intersect(blob, rays, rt, gt)


# ---------------------------------------------------------------- 1. bits of t and prim, 4. attributes
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", R.CAST_SCENES)
def test_t_and_prim_carry_the_oracles_and_debug_intersects_bits(gpu, monkeypatch, name, how):
    blob, rays, rt, gt, ref, t_cpu, prim_cpu = case(name)
    upload(gpu, monkeypatch, blob, how)
    st = abi.Stats()
    got = gpu.cast(rays, rt, gt, stats=st)
    assert list(got) == list(ALL) and len(got["t"]) == R.N_RAYS
    assert np.array_equal(got["prim"], prim_cpu) and same(got["t"], t_cpu)
    t_dbg, prim_dbg = gpu.debug_intersect(rays, rt, gt)
    assert np.array_equal(got["prim"], prim_dbg) and same(got["t"], t_dbg)
    print(G.check_against(f"{name} ({how})", ref, got["t"], got["prim"]))
    assert (st.segments, st.shadow_rays, st.samples) == (R.N_RAYS, 0, 0) and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    # the t / prim-only instantiation returns the same bits
    assert same(gpu.cast(rays, rt, gt, want=("t", "prim")), {k: got[k] for k in ("t", "prim")})


@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", R.CAST_SCENES)
def test_attributes_match_the_float64_reading(gpu, monkeypatch, name, how):
    """Material exactly; the normal of a rectangle under the identity exactly; normal and uv within cast_ref's tolerances of the
    float64 values at p = o + t_gpu d on the well-conditioned hits; the front flag wherever the float64 dot product decides it;
    sphere uv off the poles, at most 10 % of a scene's sphere hits left out; zeros on a miss."""
    blob, rays, rt, gt, hit, _, _ = case(name)
    upload(gpu, monkeypatch, blob, how)
    got = gpu.cast(rays, rt, gt)
    prims, _ = G.scene_tables(blob)
    miss = got["prim"] < 0
    assert np.array_equal(got["material"][miss], np.full(miss.sum(), -1, np.int32)) and not bits(got["normal"][miss]).any() and not bits(got["uv"][miss]).any()
    assert np.array_equal(got["material"][~miss], prims["material"][got["prim"][~miss]])
    good = ~hit["ill"] & (hit["prim"] >= 0) & (got["prim"] == hit["prim"])
    assert good.sum() == (~hit["ill"] & (hit["prim"] >= 0)).sum() >= 0.2 * R.N_RAYS
    ref = R.reference(blob, rays, got["t"], np.where(good, got["prim"], -1), gt)
    tol_n, tol_uv = R.tolerances(ref)
    with np.errstate(all="ignore"):
        err_n = np.abs(got["normal"][:, :3].astype(np.float64) - ref["normal"])
        err_uv = R.uv_difference(got["uv"], ref)
        units_n = np.where(ref["unit_n"] > 0, err_n / (R.U * ref["unit_n"]), 0.0)[good]
        units_uv = err_uv / (R.U * ref["unit_uv"])
    rect, sph = good & ~ref["sphere"], good & ref["sphere"] & ~ref["pole"]
    n_sph = int((good & ref["sphere"]).sum())
    poles = float((good & ref["pole"]).sum()) / n_sph if n_sph else 0.0
    print(f"{name} ({how}): normal {units_n.max():.2f} units (tolerance {R.K_FACTOR * R.C_NORMAL:.2f}), rectangle uv "
          f"{units_uv[rect].max() if rect.any() else 0.0:.2f} ({R.K_FACTOR * R.C_UV_RECT:.2f}), sphere uv {units_uv[sph].max() if sph.any() else 0.0:.2f} "
          f"({R.K_FACTOR * R.C_UV_SPHERE:.2f}); {100 * poles:.2f} % of the sphere hits at the poles")
    exact = good & ref["exact_normal"]
    assert np.array_equal(got["normal"][exact, :3], ref["normal"][exact].astype(np.float32))  # exactly +-axis
    assert (err_n[good] <= tol_n[good]).all(), f"normal: ray {np.nonzero(good)[0][int((err_n[good] - tol_n[good]).max(1).argmax())]}"
    assert (err_uv[rect] <= tol_uv[rect]).all() and (err_uv[sph] <= tol_uv[sph]).all()
    assert poles <= 0.10
    decided = good & (np.abs(ref["dot"]) > R.front_margin(ref, rays))
    assert decided.sum() >= 0.9 * good.sum()
    assert np.array_equal(got["normal"][decided, 3], (ref["dot"][decided] < 0.0).astype(np.float32))
    assert np.isin(got["normal"][~miss, 3], (0.0, 1.0)).all()


def test_texture_scene_uv_agrees_with_surface_uv(gpu, monkeypatch):
    """G.texture_scene() through rays at the pixel centres: on the pixels uv_expectation marks as checked, uv lies in the
    expectation's range over the pixel and within cast_ref's tolerance of surface_uv at the hit point."""
    blob = G.texture_scene()
    exp = G.uv_expectation(blob)
    hdr = abi.SceneHeader.from_buffer_copy(blob[:C.sizeof(abi.SceneHeader)])
    ys, xs = np.mgrid[0:G.TEX_H, 0:G.TEX_W]
    o, d = G.camera_rays(hdr, (xs.ravel() + 0.5) / G.TEX_W, (ys.ravel() + 0.5) / G.TEX_H)
    rays = np.concatenate([o, d, np.full((len(o), 1), 1e-6), np.full((len(o), 1), 1e27)], axis=1).astype(np.float32)
    for how in ("as_uploaded", "forced_tree"):
        upload(gpu, monkeypatch, blob, how)
        got = gpu.cast(rays)
        c = exp["checked"].ravel()
        assert c.sum() > 1000 and np.array_equal(got["prim"][c], exp["prim"].ravel()[c])
        lo, hi = exp["lo"].reshape(-1, 2), exp["hi"].reshape(-1, 2)  # the range over the pixel's corners, widened by an 8-bit step
        lit = exp["lit"].ravel() & c
        uv = got["uv"].astype(np.float64)
        assert ((uv[lit] >= lo[lit]) & (uv[lit] <= hi[lit])).all(), how
        assert np.array_equal(got["normal"][c, 3], exp["lit"].ravel()[c].astype(np.float32))  # lit = the front face shows
        ref = R.reference(blob, rays, got["t"], np.where(c, got["prim"], -1))
        _, tol_uv = R.tolerances(ref)
        assert (R.uv_difference(got["uv"], ref)[c & ~ref["pole"]] <= tol_uv[c & ~ref["pole"]]).all(), how


# ---------------------------------------------------------------- 2. edge rays (test_gpu_geometry's recipe, rebuilt here)
def edge_rays(blob, seed, first_pass):
    """About 20 000 rays (n, 8) of the families random draws never produce, with their ray and gather times.
    first_pass(rays) -> t: hit distances of a first pass, for the family whose tmax is its own hit distance."""
    rng = np.random.default_rng(seed)
    prims, xforms = G.scene_tables(blob)
    cen, rad, _ = G.bounding_spheres(blob)
    lo, hi = (cen - rad[:, None]).min(0), (cen + rad[:, None]).max(0)
    f32 = np.float32

    def rand_o(n):
        return rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n, 3)).astype(f32)

    def rand_d(n):
        d = rng.normal(size=(n, 3))
        return (d * rng.uniform(0.2, 12.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)

    def to_world(xi, p):  # fp32, the way a hit point is made
        m = xforms["m"][xi].reshape(3, 4)
        if np.array_equal(m, np.eye(3, 4, dtype=f32)):
            return p.astype(f32)
        return (p.astype(f32) @ m[:, :3].T + m[:, 3]).astype(f32)

    def vec_world(xi, v):
        return (v.astype(f32) @ xforms["m"][xi].reshape(3, 4)[:, :3].T).astype(f32)
    rects = np.nonzero((prims["type"] >= abi.PRIM_RECT_X) & (prims["type"] <= abi.PRIM_RECT_Z))[0]
    spheres = np.nonzero(prims["type"] == abi.PRIM_SPHERE)[0]
    out = []

    def add(o, d, tmin=1e-6, tmax=1e27):
        n = len(o)
        r = np.empty((n, 8), f32)
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
        out.append(r)

    def rect_points(n, mode):
        """n points of random rectangles in object space, with the rectangle's index, transform and axes: mode 'in' anywhere
        inside, 'corner' a corner, 'edge' on an edge."""
        pi = rng.choice(rects, n)
        p = prims["p"][pi]
        fa, fb = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        if mode == "corner":
            fa, fb = np.rint(fa), np.rint(fb)
        elif mode == "edge":
            fa = np.rint(fa)
        pts = np.zeros((n, 3), f32)
        axes = np.array([G.RECT_AXES[int(t)] for t in prims["type"][pi]])
        rows = np.arange(n)
        pts[rows, axes[:, 0]] = p[:, 4]
        pts[rows, axes[:, 1]] = np.where(fa == 0, p[:, 0], np.where(fa == 1, p[:, 1], (p[:, 0] + fa * (p[:, 1] - p[:, 0])).astype(f32)))
        pts[rows, axes[:, 2]] = np.where(fb == 0, p[:, 2], np.where(fb == 1, p[:, 3], (p[:, 2] + fb * (p[:, 3] - p[:, 2])).astype(f32)))
        return pi, prims["xform"][pi], axes, pts

    def per_xform(xi, pts, fn):
        res = np.empty_like(pts)
        for x in np.unique(xi):
            res[xi == x] = fn(int(x), pts[xi == x])
        return res
    # 1. directions with one or two components exactly +0.0 / -0.0
    n = 3000
    d = rand_d(n)
    pat = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1]], bool)[np.arange(n) % 6]
    d[pat] = np.where(np.arange(n) % 2 == 0, f32(0.0), f32(-0.0))[:, None].repeat(3, 1)[pat]
    add(rand_o(n), d)
    # 2. origins exactly on a rectangle's plane / a transformed box's face (tmin 1e-6 and 0), random and axis-parallel directions
    n = 2400
    _, xi, axes, pts = rect_points(n, "in")
    d = rand_d(n)
    axis_d = np.zeros((n, 3), f32)
    axis_d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0, 3.0], n)
    d[::3] = per_xform(xi, axis_d, vec_world)[::3]
    add(per_xform(xi, pts, to_world), d, tmin=np.where(np.arange(n) % 2 == 0, 1e-6, 0.0))
    # 3. origins on a sphere's surface: the fp32 point c + r n
    if spheres.size:
        n = 1200
        si = rng.choice(spheres, n)
        nrm = rng.normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        p = prims["p"][si]
        pts = (p[:, 0:3] + p[:, 3:4] * nrm.astype(f32)).astype(f32)
        add(per_xform(prims["xform"][si], pts, to_world), rand_d(n), tmin=np.where(np.arange(n) % 2 == 0, 1e-6, 0.0))
    # 4. origins on coordinates taken from the primitives' bounds (the tree's split planes are among them)
    n = 3000
    ident = prims["xform"] == 0
    coords = []
    for ax in range(3):
        vals = [cen[:, ax] - rad, cen[:, ax] + rad]  # bounding spheres of everything, transformed primitives included
        for ty, (ik, ia, ib) in G.RECT_AXES.items():
            m = ident & (prims["type"] == ty)
            vals += [prims["p"][m, 4]] if ik == ax else []
            vals += [prims["p"][m, 0], prims["p"][m, 1]] if ia == ax else []
            vals += [prims["p"][m, 2], prims["p"][m, 3]] if ib == ax else []
        m = ident & (prims["type"] == abi.PRIM_SPHERE)
        vals += [prims["p"][m, ax] - prims["p"][m, 3], prims["p"][m, ax] + prims["p"][m, 3], prims["p"][m, ax]]
        coords.append(np.unique(np.concatenate(vals).astype(f32)))
    o = np.stack([rng.choice(coords[ax], n) for ax in range(3)], axis=1)
    rnd = rand_o(n)
    keep_random = rng.uniform(size=(n, 3)) < 0.4  # one or two coordinates stay off the planes
    o[keep_random] = rnd[keep_random]
    d = rand_d(n)
    axis_d = np.zeros((n, 3), f32)
    axis_d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    d[::2] = axis_d[::2]
    add(o, d)
    # 5. rays lying in a rectangle's plane (d_k = 0 in its object space), starting on the plane inside, outside and far away
    n = 1500
    _, xi, axes, pts = rect_points(n, "in")
    d_obj = rand_d(n)
    d_obj[np.arange(n), axes[:, 0]] = 0.0
    shift = (rng.choice([0.0, -1.5, 40.0], n)[:, None] * d_obj).astype(f32)
    add(per_xform(xi, (pts + shift).astype(f32), to_world), per_xform(xi, d_obj, vec_world))
    # 6. rays through rectangle corners and along edges
    n = 2400
    _, xi, axes, pts = rect_points(n, "corner")
    rows = np.arange(n)
    d_obj = np.zeros((n, 3), f32)                  # a third: along the normal, exactly through the corner
    d_obj[rows, axes[:, 0]] = rng.choice([-2.0, 1.0], n)
    o_obj = (pts - 5.0 * d_obj).astype(f32)
    k3 = rows % 3 == 1                             # a third: along an edge, starting before the corner
    d_obj[k3] = 0.0
    d_obj[rows[k3], axes[k3, 1]] = 1.0
    o_obj[k3] = (pts[k3] - 7.0 * d_obj[k3]).astype(f32)
    o_w, d_w = per_xform(xi, o_obj, to_world), per_xform(xi, d_obj, vec_world)
    k3 = rows % 3 == 2                             # a third: from anywhere, aimed at the corner
    o_w[k3] = rand_o(int(k3.sum()))
    d_w[k3] = (per_xform(xi, pts, to_world)[k3] - o_w[k3]).astype(f32)
    add(o_w, d_w)
    # 7. denormal components and components of 1e-30
    n = 2000
    o, d = rand_o(n), rand_d(n)
    tiny = np.array([1e-30, -1e-30, 1e-40, -1e-40, 1.4e-45], f32)
    col = rng.integers(0, 3, n)
    d[np.arange(n)[: n // 2], col[: n // 2]] = rng.choice(tiny, n // 2)
    o[np.arange(n)[n // 2:], col[n // 2:]] = rng.choice(tiny, n - n // 2)
    add(o, d)
    # 8. direction lengths of 1e-18 and 1e18
    n = 2000
    d = rand_d(n)
    d = (d * np.where(np.arange(n) % 2 == 0, f32(1e-18), f32(1e18))[:, None]).astype(f32)
    o = rand_o(n)
    o[: n // 2] = ((lo + hi) / 2).astype(f32)
    add(o, d)
    # 9. tmax equal to the hit distance of the same ray (and one ulp above it); tmin == tmax; tmin > tmax; tmax = inf
    n = 2000
    o, d = rand_o(n), rand_d(n)
    probe = np.concatenate([o, d, np.full((n, 1), 1e-6, f32), np.full((n, 1), 1e27, f32)], axis=1).astype(f32)
    t_hit = np.asarray(first_pass(probe), f32)
    add(o, d, tmax=np.where(np.arange(n) % 2 == 0, t_hit, np.nextafter(t_hit, f32(np.inf))))
    add(o[:600], d[:600], tmin=t_hit[:600], tmax=t_hit[:600])
    add(o[600:1000], d[600:1000], tmin=5.0, tmax=1.0)
    add(o[1000:], d[1000:], tmax=np.inf)
    # 10. NaN and inf components; the null direction
    n = 600
    o, d = rand_o(n), rand_d(n)
    bad = np.array([np.nan, np.inf, -np.inf], f32)
    col = rng.integers(0, 3, n)
    o[np.arange(n)[:200], col[:200]] = rng.choice(bad, 200)
    d[np.arange(n)[200:400], col[200:400]] = rng.choice(bad, 200)
    tmax = np.full(n, 1e27, f32)
    tmax[400:500] = np.nan
    d[500:] = 0.0  # the null direction: 0 / 0 everywhere
    add(o, d, tmax=tmax)
    rays = np.concatenate(out)
    return rays, rng.uniform(0, 1, len(rays)).astype(f32), rng.uniform(0, 1, len(rays)).astype(f32)


EDGE_SCENES = {
    "cornell": (lambda: abi.build_scene(0, 32, 32), ("as_uploaded", "forced_tree")),
    "random19": (lambda: oracle.random_scene(19, 32, 32, n_prims=300), ("forced_tree",)),
}
EDGE_CASES = [(n, h) for n, (_, hows) in EDGE_SCENES.items() for h in hows]


@functools.lru_cache(maxsize=None)
def edge_case(name):
    blob = EDGE_SCENES[name][0]()
    rays, rt, gt = edge_rays(blob, 77, lambda probe: oracle.intersect(blob, probe)[0])
    return (blob, rays, rt, gt) + oracle.intersect(blob, rays, rt, gt)


@pytest.mark.parametrize("name,how", EDGE_CASES)
def test_edge_rays_match_the_oracle_bit_for_bit(gpu, monkeypatch, name, how):
    """Zero components, origins on planes, denormals, NaN and inf, tmin >= tmax, tmax equal to the hit distance: the closest hits
    are the oracle's, and the call returning at all is the kernel terminating on every one of them."""
    blob, rays, rt, gt, t_cpu, prim_cpu = edge_case(name)
    assert 15_000 <= len(rays) <= 25_000
    finite = np.isfinite(rays[:, :6]).all(1)
    assert (prim_cpu[finite] >= 0).mean() > 0.2
    upload(gpu, monkeypatch, blob, how)
    got = gpu.cast(rays, rt, gt)
    wrong = np.nonzero((got["prim"] != prim_cpu) | (bits(got["t"]) != bits(t_cpu)))[0]
    assert wrong.size == 0, (f"{wrong.size} rays differ, first {wrong[:5]}: rays {rays[wrong[:5]]}, gpu {list(zip(got['t'][wrong[:5]], got['prim'][wrong[:5]]))}, "
                             f"oracle {list(zip(t_cpu[wrong[:5]], prim_cpu[wrong[:5]]))}")
    miss = got["prim"] < 0
    assert not bits(got["normal"][miss]).any() and not bits(got["uv"][miss]).any() and (got["material"][miss] == -1).all()


# ---------------------------------------------------------------- 3. occlusion queries
def check_any(gpu, blob, rays, rt, gt, what):
    prims, _ = G.scene_tables(blob)
    closest = gpu.cast(rays, rt, gt, want=("t", "prim"))
    any_ = gpu.cast(rays, rt, gt, mode="any")
    assert list(any_) == ["t", "prim"]
    assert np.array_equal(any_["prim"] >= 0, closest["prim"] >= 0), f"{what}: {(( any_['prim'] >= 0) != (closest['prim'] >= 0)).sum()} rays disagree"
    hit = any_["prim"] >= 0
    assert (any_["prim"][hit] < len(prims)).all() and (any_["prim"] >= -1).all()
    assert (prims["type"][any_["prim"][hit]] <= abi.PRIM_RECT_Z).all(), f"{what}: a volume primitive occludes"
    assert same(any_["t"], np.ascontiguousarray(rays[:, 7])), f"{what}: t is not tmax"
    assert same(gpu.cast(rays, rt, gt, mode="any"), any_)  # the same candidate from call to call
    st = abi.Stats()
    gpu.cast(rays, rt, gt, mode="any", want=("prim",), stats=st)
    assert (st.segments, st.shadow_rays, st.samples) == (0, len(rays), 0)
    return closest, hit


@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", R.CAST_SCENES)
def test_any_hit_exactly_where_closest_hits(gpu, monkeypatch, name, how):
    blob, rays, rt, gt, _, _, _ = case(name)
    upload(gpu, monkeypatch, blob, how)
    _, hit = check_any(gpu, blob, rays, rt, gt, f"{name} ({how})")
    assert 0.2 < hit.mean() < 1.0


@pytest.mark.parametrize("name,how", EDGE_CASES)
def test_any_hit_exactly_where_closest_hits_on_edge_rays(gpu, monkeypatch, name, how):
    blob, rays, rt, gt, _, _ = edge_case(name)
    upload(gpu, monkeypatch, blob, how)
    check_any(gpu, blob, rays, rt, gt, f"{name} ({how})")


@pytest.mark.parametrize("how", ["as_uploaded", "no_lds"])
def test_media_are_transparent_in_both_modes(gpu, monkeypatch, how):
    blob = oracle.random_scene(23, 32, 32, n_prims=60, volumes=True)
    prims, _ = G.scene_tables(blob)
    assert (prims["type"] >= abi.PRIM_VOLUME_BOX).sum() >= 2
    rays, rt, gt = G.scene_rays(blob, G.RAY_SEED, R.N_RAYS)
    upload(gpu, monkeypatch, blob, how)
    closest, _ = check_any(gpu, blob, rays, rt, gt, f"media ({how})")
    t_cpu, prim_cpu = oracle.intersect(blob, rays, rt, gt)  # (volumes skipped there too)
    assert np.array_equal(closest["prim"], prim_cpu) and same(closest["t"], t_cpu)
    hit = closest["prim"] >= 0
    assert hit.mean() > 0.2 and (prims["type"][closest["prim"][hit]] <= abi.PRIM_RECT_Z).all()


# ---------------------------------------------------------------- 5. shapes
SHAPE_SCENES = {"scene0": "scene0", "random19": "random19"}


@pytest.mark.parametrize("name", list(SHAPE_SCENES))
def test_a_prefix_of_the_batch_gives_a_prefix_of_the_results(gpu, monkeypatch, name):
    """Block and wave edges, threads that sit at the barrier with no ray, and the host variant's chunks."""
    blob, rays, rt, gt, _, _, _ = case(name)
    upload(gpu, monkeypatch, blob)
    full = gpu.cast(rays, rt, gt)
    full_any = gpu.cast(rays, rt, gt, mode="any")
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        assert same(gpu.cast(rays[:n], rt[:n], gt[:n]), {k: v[:n] for k, v in full.items()}), n
        assert same(gpu.cast(rays[:n], rt[:n], gt[:n], mode="any"), {k: v[:n] for k, v in full_any.items()}), n
    assert same(gpu.cast(rays[:300]), gpu.cast(rays[:300], np.zeros(300, np.float32), np.zeros(300, np.float32)))  # NULL times are zeros
    monkeypatch.setenv("RTW_CAST_CHUNK", "100")
    assert same(gpu.cast(rays[:257], rt[:257], gt[:257]), {k: v[:257] for k, v in full.items()})
    assert same(gpu.cast(rays[:257], rt[:257], gt[:257], mode="any"), {k: v[:257] for k, v in full_any.items()})
    monkeypatch.setenv("RTW_CAST_CHUNK", "7777")
    assert same(gpu.cast(rays, rt, gt), full)


def raw_hits(arrays):
    return abi.Hits(**{k: v.ctypes.data for k, v in arrays.items()})


def sentinels(n=16):
    return {k: np.full((n,) + shape, -7, dt) for k, (dt, shape) in abi.CAST_OUTPUTS.items()}


def test_no_rays_is_ok_and_writes_nothing(gpu, monkeypatch):
    upload(gpu, monkeypatch, case("scene0")[0])
    out, rays = sentinels(), np.zeros((16, 8), np.float32)
    st = abi.Stats()
    assert gpu.lib.rtw_cast(gpu.ctx, rays.ctypes.data, None, None, 0, 0, C.byref(raw_hits(out)), C.byref(st)) == 0
    assert gpu.lib.rtw_cast(gpu.ctx, None, None, None, 0, 1, None, None) == 0
    d_out = {k: torch.from_numpy(v).cuda() for k, v in out.items()}
    h = abi.Hits(**{k: v.data_ptr() for k, v in d_out.items()})
    assert gpu.lib.rtw_cast_device(gpu.ctx, torch.from_numpy(rays).cuda().data_ptr(), None, None, 0, 0, C.byref(h), None, C.byref(st)) == 0
    torch.cuda.synchronize()
    assert (st.segments, st.shadow_rays, st.samples, st.seconds) == (0, 0, 0, 0.0)
    assert same(out, sentinels()) and same({k: v.cpu().numpy() for k, v in d_out.items()}, sentinels())
    empty = gpu.cast(np.zeros((0, 8), np.float32))
    assert [v.shape for v in empty.values()] == [(0,), (0,), (0,), (0, 4), (0, 2)]
    assert [tuple(v.shape) for v in cast_torch(gpu, torch.zeros((0, 8), device="cuda:0")).values()] == [(0,), (0,), (0,), (0, 4), (0, 2)]


# ---------------------------------------------------------------- 6. the device path through torch
def test_cast_torch_equals_cast_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    blob, rays, rt, gt, _, _, _ = case("random16_motion")
    upload(gpu, monkeypatch, blob)
    want = {m: gpu.cast(rays, rt, gt, mode=m) for m in ("closest", "any")}
    d_rays, d_rt, d_gt = (torch.from_numpy(a).cuda() for a in (rays, rt, gt))
    for m in ("closest", "any"):
        st = abi.Stats()
        got = cast_torch(gpu, d_rays, d_rt, d_gt, mode=m, stats=st)
        assert all(v.is_cuda for v in got.values()) and same(to_numpy(got), want[m])
        assert st.seconds > 0.0 and (st.segments, st.shadow_rays) == ((R.N_RAYS, 0) if m == "closest" else (0, R.N_RAYS))
    # a subset: the others are not allocated, the requested ones unchanged
    sub = cast_torch(gpu, d_rays, d_rt, d_gt, want=("prim", "uv"))
    assert list(sub) == ["prim", "uv"] and same(to_numpy(sub), {k: want["closest"][k] for k in ("prim", "uv")})
    check_stream_order(lambda t: cast_torch(gpu, t, d_rt, d_gt), d_rays, lambda got: same(to_numpy(got), want["closest"]))


# ---------------------------------------------------------------- 7. one batch whose byte offsets pass 2^32 and 2^34
def test_ray_indices_and_offsets_are_64_bit(gpu, monkeypatch):
    """n = 2^29 + 257: the ray tensor is 17 GiB, a 32-bit byte offset wraps at ray 2^27 and a 32-bit element offset of the rays'
    floats at ray 2^29. Every 2^20-ray tile of the outputs must equal the first."""
    free, _ = torch.cuda.mem_get_info(0)
    if free < 32 << 30:
        pytest.skip(f"needs 32 GiB of free device memory for a 17 GiB ray tensor and its outputs, {free >> 30} GiB are free")
    blob, rays, _, _, _, _, _ = case("scene0")
    upload(gpu, monkeypatch, blob)
    tile, n = 1 << 20, (1 << 29) + 257
    block = torch.from_numpy(np.resize(rays, (tile, 8))).cuda()
    first = cast_torch(gpu, block, want=("t", "prim"))
    want = gpu.cast(rays, want=("t", "prim"))
    assert same({k: v[: len(rays)].cpu().numpy() for k, v in first.items()}, want) and (want["prim"] >= 0).mean() > 0.2
    big = block.repeat(n // tile + 1, 1)[:n]
    assert big.is_contiguous() and big.shape == (n, 8)
    got = cast_torch(gpu, big, want=("t", "prim"))
    assert list(got) == ["t", "prim"]
    ok = torch.ones((), dtype=torch.bool, device="cuda:0")
    for k in ("t", "prim"):
        a, f = got[k].view(torch.int32), first[k].view(torch.int32)
        for i in range(n // tile):
            ok &= (a[i * tile:(i + 1) * tile] == f).all()  # on the device, tile by tile; one read-back at the end
        ok &= (a[(n // tile) * tile:] == f[:257]).all()
    assert bool(ok.item())


# ---------------------------------------------------------------- 8. errors, groups, sessions
def test_every_refusal_leaves_the_context_usable(gpu, monkeypatch):
    blob, rays, rt, gt, _, _, _ = case("cluttered_cornell")
    rays, rt, gt = rays[:1000], rt[:1000], gt[:1000]
    lib = gpu.lib
    fresh = abi.Renderer(0)
    out = sentinels(1000)
    h_all, h_none, h_tp = raw_hits(out), abi.Hits(), raw_hits({k: out[k] for k in ("t", "prim")})
    d_rays = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(8, np.float32)])).cuda()
    d_out = {k: torch.zeros(v.size + 8, dtype=torch.float32 if v.dtype == np.float32 else torch.int32, device="cuda:0") for k, v in out.items()}
    dp = {k: v.data_ptr() for k, v in d_out.items()}
    try:
        assert lib.rtw_cast(fresh.ctx, rays.ctypes.data, None, None, 1000, 0, C.byref(h_all), None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_cast_device(fresh.ctx, d_rays.data_ptr(), None, None, 1000, 0, C.byref(abi.Hits(**dp)), None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()
    upload(gpu, monkeypatch, blob)
    want = gpu.cast(rays, rt, gt)
    want_any = gpu.cast(rays, rt, gt, mode="any")

    def still_fine():
        assert same(gpu.cast(rays, rt, gt), want) and same(gpu.cast(rays, rt, gt, mode="any"), want_any)
    R_ = rays.ctypes.data
    host_refusals = [
        (None, 1000, 0, C.byref(h_all)),          # no rays
        (R_, 1000, 0, None),                      # no rtw_hits
        (R_, 1000, 0, C.byref(h_none)),           # every output NULL
        (R_, 1000, 2, C.byref(h_all)), (R_, 1000, -1, C.byref(h_all)),
        (R_, 1 << 31, 0, C.byref(h_all)),         # n > 2^31 - 1 (refused before anything is read)
        (R_, 1000, 1, C.byref(h_all)),            # RTW_CAST_ANY with material, normal and uv
    ] + [(R_, 1000, 1, C.byref(raw_hits({"t": out["t"], k: out[k]}))) for k in ("material", "normal", "uv")]
    for r_, n, mode, h in host_refusals:
        assert lib.rtw_cast(gpu.ctx, r_, None, None, n, mode, h, None) == -1, (n, mode)
        assert lib.rtw_last_error(gpu.ctx)
        still_fine()
    D_ = d_rays.data_ptr()
    dev_refusals = [
        (None, 1000, 0, abi.Hits(**dp)), (D_, 1000, 0, None), (D_, 1000, 0, abi.Hits()), (D_, 1000, 3, abi.Hits(**dp)),
        (D_, 1 << 31, 0, abi.Hits(**dp)), (D_, 1000, 1, abi.Hits(**dp)),
        (D_ + 4, 1000, 0, abi.Hits(**dp)), (D_ + 8, 1000, 0, abi.Hits(t=dp["t"])),                 # rays off 16 bytes
        (D_, 1000, 0, abi.Hits(normal=dp["normal"] + 4)), (D_, 1000, 0, abi.Hits(normal=dp["normal"] + 8)),
        (D_, 1000, 0, abi.Hits(uv=dp["uv"] + 4)),
    ]
    for r_, n, mode, h in dev_refusals:
        st = sentinel_stats()
        assert lib.rtw_cast_device(gpu.ctx, r_, None, None, n, mode, None if h is None else C.byref(h), None, C.byref(st)) == -1, (n, mode)
        assert left_alone(st)  # a refused call leaves *stats alone
        still_fine()
    assert lib.rtw_cast_device(gpu.ctx, D_, None, None, 1000, 0, C.byref(abi.Hits(uv=dp["uv"] + 8, t=dp["t"] + 4)), None, None) == 0  # aligned enough
    assert same(out, sentinels(1000))  # no refused call wrote anything
    assert lib.rtw_cast(gpu.ctx, R_, None, None, 1000, 1, C.byref(h_tp), None) == 0
    with pytest.raises(ValueError):
        gpu.cast(rays[:, :6])
    with pytest.raises(ValueError):
        gpu.cast(rays, rt[:10])


def test_a_group_casts_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    blob, rays, rt, gt, _, _, _ = case("cluttered_cornell")
    upload(gpu, monkeypatch, blob)
    want = gpu.cast(rays, rt, gt)
    group = abi.Renderer([0, 0])
    try:
        assert group.lib.rtw_cast(group.ctx, rays.ctypes.data, None, None, 10, 0, C.byref(raw_hits(sentinels(10))), None) == -3
        group.upload_scene(blob)
        assert same(group.cast(rays, rt, gt), want)
        assert same(group.cast(rays, rt, gt, mode="any"), gpu.cast(rays, rt, gt, mode="any"))
        d = [torch.from_numpy(a).cuda() for a in (rays, rt, gt)]
        assert same(to_numpy(cast_torch(group, *d)), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    blob, rays, rt, gt, _, _, _ = case("scene0")
    upload(gpu, monkeypatch, blob)
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    want = gpu.cast(rays, rt, gt)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        assert same(gpu.cast(rays, rt, gt), want)
        assert same(to_numpy(cast_torch(gpu, *(torch.from_numpy(a).cuda() for a in (rays, rt, gt)))), want)
        monkeypatch.setenv("RTW_CAST_CHUNK", "4096")
        assert same(gpu.cast(rays, rt, gt, mode="any"), gpu.cast(rays, rt, gt, mode="any"))
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    assert same(gpu.cast(rays, rt, gt), want)
