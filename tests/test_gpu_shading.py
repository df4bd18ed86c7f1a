"""The kernels' materials, media and textures against tests/shading_ref.py (a float64 reading of the reference's programs that shares
nothing with the oracle or the kernels), then against the oracle's bits of the same keys, so that a failure says which side moved.
Two entries: rtw_radiance on the cases' rays (uploaded as is, with the tree forced, with the tree outside LDS) and rtw_render of
radiance_ref.ray_blob - every pixel the same ray on its own key - through k_path and through the wavefront kernels."""
import numpy as np
import pytest

import law_common as C
import radiance_ref as R
import shading_ref as S
from gpu_common import UPLOADS_LDS as UPLOADS, check_both, gpu, probe_is_pi_times_radiance, radiance_observed, render_observed  # noqa: F401
from gpu_common import upload_lds as upload
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- entry 1: rtw_radiance, one sample per ray, keys by key_offset
# (the second of the generator's independent samples as uploaded only, and only where the samples depend on the draws)
@pytest.mark.parametrize("name,how,rng,est,seed,base", C.runs(S, hows=list(UPLOADS), draws=slice(0, 1)) + C.runs(S, hows=["as_uploaded"], draws=slice(1, 2)))
def test_radiance_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base):
    """The float64 reference first, the oracle's bits second."""
    check_both(S, name, radiance_observed(gpu, monkeypatch, S.case(name), how, rng, est, seed, base), (rng, est, seed, base), S.COUNTS)


# ---------------------------------------------------------------- entry 2: rtw_render of the ray's own blob
RENDERED = [n for n in S.CASES if S.case(n).m <= 32]  # one upload per ray: the textures go as their 32-point subsets (texture32-*)
assert {n.split("-")[0] for n in S.CASES} - {n.split("-")[0] for n in RENDERED} == {"texture"}


@pytest.mark.parametrize("path", ["1", "0"])  # k_path (the default) / the wavefront kernels
@pytest.mark.parametrize("name,how,rng,est,seed,base", C.runs(S, RENDERED, ["as_uploaded"], slice(0, 1)))
def test_render_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base, path):
    check_both(S, name, render_observed(gpu, monkeypatch, S.case(name), path, rng, est, seed, base), (rng, est, seed, base), S.COUNTS)


# ---------------------------------------------------------------- rtw_probe: the lobe the library draws itself
@pytest.mark.parametrize("est", [S.REF, S.CORR])
@pytest.mark.parametrize("rng", S.RNGS)
@pytest.mark.parametrize("normal,kind", [((0.0, 2.0, 0.0), "normal"), ((0.0, -0.5, 0.0), "flipped"), ((3.0, 0.0, 0.0), "tangent"), ((0.0, 0.0, -1.0), "tangent")])
def test_probe_directions_follow_the_cosine_lobe(gpu, monkeypatch, normal, kind, rng, est):
    """Irradiance probes of one sample each under the sky: a probe's red is pi times the sky's red along its direction, so the
    direction's y is read as from a scatter event. The lobe is the cosine lobe whichever estimator is chosen (include/rtw.h):
    y / |n| has the CDF c^2 about a normal along +-y, the semicircle law about a normal along x or z. And each probe is, bit for
    bit, pi times rtw_radiance along that direction on the same key."""
    upload(gpu, monkeypatch, S.probe_scene(), "as_uploaded")
    probes = np.tile(np.array([0.25, 1.0, -0.5, *normal, 1e-3, 1e27], np.float32), (S.N_STAT, 1))
    out = gpu.probe(probes, 1, 1, rng_kind=rng, estimator=est, key_offset=0)
    red = out[:, 0].astype(np.float64) / float(C.PI32)
    uy = S.decode_uy(red)
    lost = S.lost_count(red)
    if kind == "tangent":
        ks = S.ks_sqrt_n(uy, lambda y: S.lambert_tangent_cdf(y, False))
    else:
        ks = S.ks_sqrt_n(uy if kind == "normal" else -uy, lambda c: S.lambert_normal_cdf(c, False))
    print(f"probe about {normal}: lost {lost}, KS sqrt(n) = {ks:.2f} (limit {S.KS_LIMIT})")
    assert lost == 0 and ks <= S.KS_LIMIT
    probe_is_pi_times_radiance(gpu, probes, out, rng, est)


# ---------------------------------------------------------------- RTW_MAT_NORMAL: black in the beauty, its colour in the albedo guide
@pytest.mark.parametrize("axis,flip", [(0, 0), (1, 0), (1, 1), (2, 1)])
def test_normal_material_colour_is_half_n_plus_half(gpu, monkeypatch, axis, flip):
    """normalMaterial.cu:30: 0.5 (n + 1) for the shading normal of a rectangle, +-axis by its flip flag, at depth 1 - where the
    library shows it: the albedo guide (include/rtw.h rtw_render_guides). The values are exact in float32."""
    n = np.zeros(3)
    n[axis] = -1.0 if flip else 1.0
    d = -np.array([0.5, 0.25, 0.125]) - 0.75 * np.eye(3)[axis]  # towards the plane from its positive side, oblique
    blob = S.surface_scene(abi.MAT_NORMAL, axis=axis, flip=flip, xformed=axis == 1 and flip == 1)
    hit = np.array([1.0, 0.5, -3.0]) if axis == 1 and flip == 1 else np.zeros(3)
    c = S.Case(blob, hit - d, d, 16)
    upload(gpu, monkeypatch, R.ray_blob(c.blob, c.o[0], c.ll[0]), "as_uploaded")
    g = gpu.render_guides(abi.make_params(4, 4, 1, 1), which=("albedo", "normal"))
    assert np.array_equal(g["normal"][..., :3], np.broadcast_to(n.astype(np.float32), (4, 4, 3)))
    assert np.array_equal(g["albedo"], np.broadcast_to(np.append(0.5 * n + 0.5, 1.0).astype(np.float32), (4, 4, 4)))
