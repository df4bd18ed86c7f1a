"""CPU suite of the ray queries (include/rtw.h rtw_cast / rtw_cast_device): the additive ABI, the Python surface's argument
handling, and cast_ref.py - the float64 reading of a hit's attributes and the constants its tolerances rest on."""
import ast
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cast_ref as R
import geometry_ref as G
from raytracing_weekend_amd import abi


# ---------------------------------------------------------------- ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_DIR, "include", "rtw.h")).read(), flags=re.S)


def test_header_declares_both_entry_points_and_the_struct():
    text = " ".join(header().split())
    assert ("int rtw_cast(rtw_ctx* ctx, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode, "
            "const rtw_hits* out, rtw_stats* stats);") in text
    assert ("int rtw_cast_device(rtw_ctx* ctx, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode, "
            "const rtw_hits* out, void* hip_stream, rtw_stats* stats);") in text
    assert "enum { RTW_CAST_CLOSEST = 0, RTW_CAST_ANY = 1 };" in text
    fields = re.search(r"typedef struct rtw_hits \{(.*?)\} rtw_hits;", text).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == ["t", "prim", "material", "normal", "uv"]
    assert "#define RTW_ABI_VERSION 5" in text  # additive: the version and the older structs stay


def test_symbols_are_listed_and_exported():
    assert "rtw_cast" in abi.HIP_SYMBOLS and "rtw_cast_device" in abi.HIP_SYMBOLS
    lib = abi.load_hip()
    assert hasattr(lib, "rtw_cast") and hasattr(lib, "rtw_cast_device")


def test_hits_mirrors_rtw_hits():
    assert C.sizeof(abi.Hits) == 40
    assert [f for f, _ in abi.Hits._fields_] == ["t", "prim", "material", "normal", "uv"] == list(abi.CAST_OUTPUTS)
    assert abi.CAST_MODES == {"closest": 0, "any": 1}
    assert C.sizeof(abi.Stats) == 184 and C.sizeof(abi.Params) == 48  # rtw_stats does not grow


def test_null_context_is_an_error_not_a_crash():
    lib = abi.load_hip()
    rays = np.zeros((4, 8), np.float32)
    t = np.zeros(4, np.float32)
    h = abi.Hits(t=t.ctypes.data)
    for n in (0, 4):
        assert lib.rtw_cast(None, rays.ctypes.data, None, None, n, 0, C.byref(h), None) < 0
        assert lib.rtw_cast_device(None, rays.ctypes.data, None, None, n, 0, C.byref(h), None, None) < 0
    assert lib.rtw_cast(None, None, None, None, 0, 7, None, None) < 0


def test_the_chunk_knob_is_listed_with_the_others():
    plan = open(os.path.join(abi.PKG_DIR, "csrc", "rtw_plan.h")).read()
    assert re.search(r"//\s+RTW_CAST_CHUNK\s", plan) and 'geti("RTW_CAST_CHUNK"' in plan


def test_the_kernel_is_a_unit_of_the_build_with_the_common_flags():
    entry = open(os.path.join(abi.REPO_DIR, "__graft_entry__.py")).read()
    assert '("rtw_cast.hip", "rtw_cast.o", [])' in entry and '"rtw_cast.hip"' not in entry.split("UNIT_FLAGS = ")[1].split("\n")[0]
    hip = open(os.path.join(abi.PKG_DIR, "csrc", "rtw_hip.hip")).read()
    assert '#include "rtw_cast.hip"' not in hip  # (a translation unit of its own, in no other)


# ---------------------------------------------------------------- the Python surface
def test_cast_outputs_follow_the_mode():
    f = abi.Renderer.cast_outputs
    assert f("closest", ("uv", "t")) == ["t", "uv"]                       # rtw_hits' order
    assert f("closest", abi.CAST_OUTPUTS) == ["t", "prim", "material", "normal", "uv"]
    assert f("any", ("t", "prim", "material", "normal", "uv")) == ["t", "prim"]   # the default `want` under "any"
    for mode, want in (("nearest", ("t",)), ("closest", ()), ("closest", ("depth",)), ("any", ("normal",))):
        with pytest.raises(ValueError):
            f(mode, want)


def test_torch_is_imported_inside_the_function_only():
    for name in ("abi.py", "torch_cast.py"):
        tree = ast.parse(open(os.path.join(abi.PKG_DIR, name)).read())
        top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
        assert "torch" not in names, name
    from raytracing_weekend_amd import torch_cast
    assert callable(torch_cast.cast_torch)


# ---------------------------------------------------------------- cast_ref: the reference and its constants
@functools.lru_cache(maxsize=None)
def case(name):
    blob = G.SCENES[name]()
    rays, rt, gt = G.scene_rays(blob, G.RAY_SEED, R.N_RAYS)
    hit = G.closest_hit(blob, rays, rt, gt)
    return blob, rays, rt, gt, hit, R.measure(blob, rays, rt, gt, hit)


def test_the_tolerances_are_four_times_the_measured_constants():
    assert R.K_FACTOR == 4.0 == G.K_FACTOR and R.U == 2.0 ** -24 and R.POLE == 1e-2 and R.N_RAYS == 20_000
    for c in (R.C_NORMAL, R.C_UV_RECT, R.C_UV_SPHERE):
        assert 0.0 < c < 100.0  # beyond ~100 the error model lacks a term
    ref = {"sphere": np.array([True, False]), "unit_n": np.ones((2, 3)), "unit_uv": np.ones((2, 2))}
    tol_n, tol_uv = R.tolerances(ref)
    assert np.allclose(tol_n, 4.0 * R.C_NORMAL * 2.0 ** -24, rtol=1e-15)
    assert np.allclose(tol_uv[0], 4.0 * R.C_UV_SPHERE * 2.0 ** -24, rtol=1e-15) and np.allclose(tol_uv[1], 4.0 * R.C_UV_RECT * 2.0 ** -24, rtol=1e-15)


@pytest.mark.parametrize("name", R.CAST_SCENES)
def test_constants_re_measured(name):
    blob, rays, rt, gt, hit, (c, poles) = case(name)
    print(f"{name}: normal {c[0]:.4f}, rectangle uv {c[1]:.4f}, sphere uv {c[2]:.4f} units; {100 * poles:.2f} % of the sphere hits at the poles")
    assert c[0] <= R.C_NORMAL + 5e-4 and c[1] <= R.C_UV_RECT + 5e-4 and c[2] <= R.C_UV_SPHERE + 5e-4
    assert poles <= 0.10
    good = ~hit["ill"] & (hit["prim"] >= 0)
    assert good.mean() >= 0.20


def test_the_written_constants_are_the_largest_of_the_scenes():
    worst = np.max([case(name)[5][0] for name in R.CAST_SCENES], axis=0)
    for got, written in zip(worst, (R.C_NORMAL, R.C_UV_RECT, R.C_UV_SPHERE)):
        assert written - 1e-3 <= got <= written + 5e-4, (worst, written)


def test_single_sphere_scenes_lose_few_hits_to_the_poles():
    """The issue's figures: 0.3 %, 5.6 %, 0 % and 0 % of the well-conditioned sphere hits (SURVEY Q13's off-centre normal is why
    sphere-rot_x is the largest)."""
    shares = []
    for x in ("identity", "rot_x", "rot_y", "rot_z"):
        blob = G.SCENES[f"sphere-{x}"]()
        rays, rt, gt = G.scene_rays(blob, G.RAY_SEED, R.N_RAYS)
        shares.append(R.measure(blob, rays, rt, gt)[1])
    print(shares)
    assert max(shares) <= 0.10 and int(np.argmax(shares)) == 1 and abs(shares[1] - 0.056) < 0.002


@pytest.mark.parametrize("name", ["sphere-rot_x", "rect_y-rot_z", "scene0", "random19"])
def test_evaluate_at_float64_is_geometry_refs_reading(name):
    """evaluate() restates shading_normal and surface_uv (it exists to run them at fp32): at float64 the two must agree."""
    blob, rays, rt, gt, hit, _ = case(name)
    prim = np.where(hit["ill"], -1, hit["prim"])
    ref = R.reference(blob, rays, hit["t"].astype(np.float32), prim, gt)
    n64, uv64 = R.evaluate(blob, rays, hit["t"].astype(np.float32), prim, gt, np.float64)
    hits = prim >= 0
    assert hits.sum() > 2000
    assert np.abs(n64 - ref["normal"])[hits].max() <= 1e-12 * max(1.0, np.abs(ref["normal"][hits]).max())
    assert R.uv_difference(uv64, ref)[hits & ~ref["pole"]].max() <= 1e-10
    assert np.array_equal(ref["material"][~hits], np.full((~hits).sum(), -1)) and not ref["normal"][~hits].any() and not ref["uv"][~hits].any()
    prims, _ = G.scene_tables(blob)
    assert np.array_equal(ref["material"][hits], prims["material"][prim[hits]])


def test_moving_sphere_normal_takes_the_centre_at_the_gather_time():
    """(P - C(g)) / r: with the ray time in the gather time's place nearly every normal leaves its tolerance, and the centre does
    move between the keys (t0 = 0.25, t1 = 1.5 of geometry_ref.SINGLE_PRIMS)."""
    blob, rays, rt, gt, hit, _ = case("moving_sphere-rot_y")
    prim = np.where(hit["ill"], -1, hit["prim"])
    t = hit["t"].astype(np.float32)
    ref = R.reference(blob, rays, t, prim, gt)
    swapped = R.reference(blob, rays, t, prim, rt)
    hits = prim >= 0
    tol_n, _ = R.tolerances(ref)
    off = (np.abs(swapped["normal"] - ref["normal"]) > tol_n).any(1)
    assert hits.sum() > 2000 and off[hits].mean() > 0.99
    # by hand for one hit: C(g) = C0 + (g - 0.25) / 1.25 (C1 - C0), the normal through the transposed inverse
    i = int(np.nonzero(hits)[0][0])
    prims, xforms = G.scene_tables(blob)
    P = prims[0]["p"].astype(np.float64)
    c = P[0:3] + (float(gt[i]) - P[7]) / (P[8] - P[7]) * (P[4:7] - P[0:3])
    p = rays[i, 0:3].astype(np.float64) + float(t[i]) * rays[i, 3:6].astype(np.float64)
    want = ((p - c) / P[3]) @ xforms[prims[0]["xform"]]["inv"].reshape(3, 4).astype(np.float64)[:, :3]
    assert np.allclose(ref["normal"][i], want, rtol=1e-13, atol=1e-13)


def test_front_margin_leaves_exact_rectangles_decided():
    blob, rays, rt, gt, hit, _ = case("scene0")
    prim = np.where(hit["ill"], -1, hit["prim"])
    ref = R.reference(blob, rays, hit["t"].astype(np.float32), prim, gt)
    ex = ref["exact_normal"]
    assert ex.sum() > 2000 and set(np.abs(ref["normal"][ex]).sum(1).tolist()) == {1.0}
    assert (np.abs(ref["dot"][ex]) > R.front_margin(ref, rays)[ex]).mean() > 0.999
