"""The kernels' direct lighting against tests/lighting_ref.py (a float64 reading of the reference's closest-hit, pdf and material
programs that shares nothing with the oracle or the kernels), then against the oracle's bits and probe count of the same keys, so
that a failure says which side moved. Three entries: rtw_radiance on the case's ray (uploaded as is, with the tree forced, with
the tree outside LDS), rtw_render of radiance_ref.ray_blob through k_path and through the wavefront kernels - the shadow probe is
inline, deferred and queued respectively - and rtw_probe's irradiance at the receiver point."""
import functools

import numpy as np
import pytest

import lighting_ref as L
import probe_ref
import radiance_ref as R
import shading_ref as S
import gpu_common
from gpu_common import UPLOADS_LDS as UPLOADS, gpu, same_bits  # noqa: F401
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu

PI32 = np.float32(3.14159265)


upload = functools.partial(gpu_common.upload, knobs=gpu_common.UPLOAD_KNOBS)


def runs(hows, draws):
    """draws: which of the generator's independent samples (shading_ref.DRAWS); a case without draws has only the first."""
    out = []
    for name in L.CASES:
        for est in L.case(name).estimators:
            out += [pytest.param(name, how, rng, est, seed, base, id=f"{name}-{how}-rng{rng}-est{est}-seed{seed:x}-key{base}")
                    for how in hows for rng in L.RNGS for seed, base in L.DRAWS[rng][draws] if draws.start == 0 or L.drawn(name)]
    return out


def both(name, got, shadow_rays, rng, est, seed, base):
    """The float64 reference first, the oracle's bits and probe count second."""
    print(L.check(name, got, est, shadow_rays=shadow_rays))
    want, want_shadow = L.oracle_samples(name, rng, est, seed, base)
    assert same_bits(got, want), f"{name}: {int((got != want).any(-1).sum())} samples differ from the oracle's"
    assert shadow_rays == want_shadow, f"{name}: {shadow_rays} shadow rays, the oracle traces {want_shadow}"


# ---------------------------------------------------------------- entry 1: rtw_radiance, one sample per ray, keys by key_offset
@pytest.mark.parametrize("name,how,rng,est,seed,base", runs(list(UPLOADS), slice(0, 1)) + runs(["as_uploaded"], slice(1, 2)))
def test_radiance_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base):
    c = L.case(name)
    upload(gpu, monkeypatch, c.blob, how)
    st = abi.Stats()
    out = gpu.radiance(c.rays(est), 1, c.depth, seed=seed, rng_kind=rng, estimator=est, key_offset=base, stats=st)
    assert np.array_equal(out[:, 3], np.ones(len(out), np.float32))
    both(name, out[:, :3].reshape(1, c.keys_per_ray, 3), int(st.shadow_rays), rng, est, seed, base)


# ---------------------------------------------------------------- entry 2: rtw_render of the ray's own blob
@pytest.mark.parametrize("path", ["1", "0"])  # k_path (the default) / the wavefront kernels
@pytest.mark.parametrize("name,how,rng,est,seed,base", runs(["as_uploaded"], slice(0, 1)))
def test_render_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base, path):
    for k in ("RTW_BRUTE_MAX", "RTW_LDS_KB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTW_PATH", path)
    c = L.case(name)
    gpu.upload_scene(R.ray_blob(c.blob, c.o[0], c.ll[0]))
    img, st = gpu.render(S.render_params(c, 0, rng, est, seed, base))
    both(name, img[..., :3].reshape(1, c.keys_per_ray, 3), int(st.shadow_rays), rng, est, seed, base)


# ---------------------------------------------------------------- entry 3: rtw_probe, the irradiance at the receiver point
@pytest.mark.parametrize("est", [L.CORR, L.NO_NEE])
@pytest.mark.parametrize("rng", L.RNGS)
@pytest.mark.parametrize("name", ["two_emitters_one_unlisted-d2", "occluded-d2", "own_emitter-d2"])
def test_probe_irradiance_is_pi_times_the_emitters_form_factors(gpu, monkeypatch, name, rng, est):
    """Irradiance probes of one sample and one segment each at the receiver point: a probe is pi * Le of the emitter its
    cosine-distributed direction meets - listed or not, no light sample came before - so the hit count per channel is binomial with
    p = the visible form factor, and the mean irradiance is pi * sum Le_c F_c. And each probe is, bit for bit, pi times
    rtw_radiance along that direction on the same key."""
    c = L.case(name)
    upload(gpu, monkeypatch, c.blob, "as_uploaded")
    probes = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1e-3, 1e27], np.float32), (L.N_RARE, 1))
    out = gpu.probe(probes, 1, 1, rng_kind=rng, estimator=est, key_offset=0)
    print(L.check_irradiance(name, out[:, :3], PI32))
    first = probes[:1024]  # the keys count from 0, so the first probes are the first rays
    rays = probe_ref.rays_of(first, probe_ref.directions(first, 1, rng_kind=rng), 0)
    rad = gpu.radiance(rays, 1, 1, rng_kind=rng, estimator=est, key_offset=0)
    assert same_bits(out[:1024, :3], rad[:, :3] * PI32)
