"""The kernels' materials, media and textures against tests/shading_ref.py (a float64 reading of the reference's programs that shares
nothing with the oracle or the kernels), then against the oracle's bits of the same keys, so that a failure says which side moved.
Two entries: rtw_radiance on the cases' rays (uploaded as is, with the tree forced, with the tree outside LDS) and rtw_render of
radiance_ref.ray_blob - every pixel the same ray on its own key - through k_path and through the wavefront kernels."""
import functools

import numpy as np
import pytest

import probe_ref
import radiance_ref as R
import shading_ref as S
import gpu_common
from gpu_common import UPLOADS_LDS as UPLOADS, gpu, same_bits  # noqa: F401
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu


upload = functools.partial(gpu_common.upload, knobs=gpu_common.UPLOAD_KNOBS)


def runs(names, hows, draws):
    """draws: which of the generator's independent samples (shading_ref.DRAWS: a second seed for Philox, other keys for TEA+LCG)."""
    out = []
    for name in names:
        for est in S.case(name).estimators:
            out += [pytest.param(name, how, rng, est, seed, base, id=f"{name}-{how}-rng{rng}-est{est}-seed{seed:x}-key{base}")
                    for how in hows for rng in S.RNGS for seed, base in S.DRAWS[rng][draws]]
    return out


def drawn(names):
    """The cases whose samples depend on draws: only they are worth a second draw."""
    return [n for n in names if n.split("-")[0] not in ("emitter", "texture", "texture32")]


def both(name, got, rng, est, seed, base):
    """The float64 reference first, the oracle's bits second."""
    print(S.check(name, got, est))
    want = S.oracle_samples(name, rng, est, seed, base)
    assert same_bits(got, want), f"{name}: {int((got != want).any(-1).sum())} samples differ from the oracle's"


# ---------------------------------------------------------------- entry 1: rtw_radiance, one sample per ray, keys by key_offset
@pytest.mark.parametrize("name,how,rng,est,seed,base", runs(list(S.CASES), list(UPLOADS), slice(0, 1)) + runs(drawn(S.CASES), ["as_uploaded"], slice(1, 2)))
def test_radiance_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base):
    c = S.case(name)
    upload(gpu, monkeypatch, c.blob, how)
    out = gpu.radiance(c.rays(est), 1, c.depth, seed=seed, rng_kind=rng, estimator=est, key_offset=base)
    assert np.array_equal(out[:, 3], np.ones(len(out), np.float32))
    both(name, out[:, :3].reshape(c.m, c.keys_per_ray, 3), rng, est, seed, base)


# ---------------------------------------------------------------- entry 2: rtw_render of the ray's own blob
RENDERED = [n for n in S.CASES if S.case(n).m <= 32]  # one upload per ray: the textures go as their 32-point subsets (texture32-*)
assert {n.split("-")[0] for n in S.CASES} - {n.split("-")[0] for n in RENDERED} == {"texture"}


@pytest.mark.parametrize("path", ["1", "0"])  # k_path (the default) / the wavefront kernels
@pytest.mark.parametrize("name,how,rng,est,seed,base", runs(RENDERED, ["as_uploaded"], slice(0, 1)))
def test_render_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base, path):
    for k in ("RTW_BRUTE_MAX", "RTW_LDS_KB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTW_PATH", path)
    c = S.case(name)
    got = np.empty((c.m, c.keys_per_ray, 3), np.float32)
    for j in range(c.m):
        gpu.upload_scene(R.ray_blob(c.blob, c.o[j], c.ll[j]))
        img, _ = gpu.render(S.render_params(c, j, rng, est, seed, base))
        got[j] = img[..., :3].reshape(c.keys_per_ray, 3)
    both(name, got, rng, est, seed, base)


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
    red = out[:, 0].astype(np.float64) / float(np.float32(3.14159265))
    uy = S.decode_uy(red)
    lost = S.lost_count(red)
    if kind == "tangent":
        ks = S.ks_sqrt_n(uy, lambda y: S.lambert_tangent_cdf(y, False))
    else:
        ks = S.ks_sqrt_n(uy if kind == "normal" else -uy, lambda c: S.lambert_normal_cdf(c, False))
    print(f"probe about {normal}: lost {lost}, KS sqrt(n) = {ks:.2f} (limit {S.KS_LIMIT})")
    assert lost == 0 and ks <= S.KS_LIMIT
    first = probes[:1024]  # the keys count from 0, so the first probes are the first rays
    rays = probe_ref.rays_of(first, probe_ref.directions(first, 1, rng_kind=rng), 0)
    rad = gpu.radiance(rays, 1, 1, rng_kind=rng, estimator=est, key_offset=0)
    assert same_bits(out[:1024, :3], rad[:, :3] * np.float32(3.14159265))


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
