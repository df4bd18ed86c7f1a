"""CPU suite: the oracle's closest hits and texture coordinates against geometry_ref.py, a float64 second reading of the
reference's intersection and texture programs. What the bit-parity tests cannot see - an axis swapped, a transform applied the
wrong way round, the two times of a moving sphere exchanged, a mirrored image - in the oracle and the kernels alike shows here."""
import functools

import numpy as np
import pytest

import geometry_ref as G
import oracle
from raytracing_weekend_amd import abi


@functools.lru_cache(maxsize=None)
def case(name):
    """(blob, rays, ray times, gather times, float64 reference) of one scene, computed once."""
    blob = G.SCENES[name]()
    rays, rt, gt = G.scene_rays(blob, G.RAY_SEED)
    return blob, rays, rt, gt, G.closest_hit(blob, rays, rt, gt)


def test_the_tolerance_is_four_times_the_measured_constant():
    assert G.K == 4.0 * G.MEASURED_CONSTANT and 0.0 < G.MEASURED_CONSTANT < 100.0  # beyond ~100 the error model lacks a term
    assert G.EPS == 1e-3 and G.EPS_UNIT * 2.0 ** 24 > G.K  # the unit margin of the conditioning covers the tolerance


@pytest.mark.parametrize("name", list(G.SCENES))
def test_oracle_closest_hit_matches_float64_reference(name):
    blob, rays, rt, gt, ref = case(name)
    t, prim = oracle.intersect(blob, rays, rt, gt)
    fig = G.check_against(name, ref, t, prim)
    # the conditions of the check itself: every primitive kind of the scene wins somewhere, and the reference at fp32 stays
    # within the constant the tolerance was derived from (and picks the same primitive on every well-conditioned ray)
    prims, _ = G.scene_tables(blob)
    won = set(prims["type"][ref["prim"][~ref["ill"] & (ref["prim"] >= 0)]].tolist())
    assert won == set(prims["type"][prims["type"] <= abi.PRIM_RECT_Z].tolist()), fig
    constant, differ = G.error_constant(blob, rays, rt, gt, ref)
    print(f"{fig}; reference at fp32: {constant:.3f} units")
    assert differ == 0 and constant <= G.MEASURED_CONSTANT + 5e-4, (fig, constant, differ)


# ---------------------------------------------------------------- texture coordinates
@functools.lru_cache(maxsize=None)
def uv_case():
    blob = G.texture_scene()
    return blob, G.uv_expectation(blob)


def test_ramp_image_is_what_rtw_h_says():
    words = np.frombuffer(G.ramp_image(8, 4), "<u4")
    assert words[0] == 8 and words[1] == 4 and len(words) == 2 + 32
    tex = words[2:].reshape(4, 8)
    assert [int(v) & 255 for v in tex[0]] == [16, 48, 80, 112, 143, 175, 207, 239]       # red: the column
    assert [int(v) >> 8 & 255 for v in tex[:, 0]] == [32, 96, 159, 223]                  # green: the row, row 0 first
    assert np.all(tex >> 24 == 255) and np.all((tex >> 16) & 255 == 0)


@pytest.mark.parametrize("rng", [abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG])
def test_oracle_texture_coordinates_match_float64_reference(rng):
    """Emitters, depth 1, one sample: the oracle's picture IS texture(u, v) at the first hit. Red must be the reference's u and
    green its v: sphere u = 1 - (phi + pi) / 2 pi and v from asin(n.y), rectangle u, v along its a and b axes, image row 0 at
    v = 0, texel centres at (i + 0.5) / width - each within the range over the pixel plus one 8-bit step."""
    blob, exp = uv_case()
    img, _ = oracle.render(blob, abi.make_params(G.TEX_W, G.TEX_H, 1, 1, rng_kind=rng), threads=4)
    G.check_uv(exp, img, "oracle picture")
    dark = exp["checked"] & ~exp["lit"]
    print(f"checked {exp['checked'].sum()} pixels, {dark.sum()} of them on faces the shading normal turns away (SURVEY Q13)")
