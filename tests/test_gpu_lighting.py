"""The kernels' direct lighting against tests/lighting_ref.py (a float64 reading of the reference's closest-hit, pdf and material
programs that shares nothing with the oracle or the kernels), then against the oracle's bits and probe count of the same keys, so
that a failure says which side moved. Three entries: rtw_radiance on the case's ray (uploaded as is, with the tree forced, with
the tree outside LDS), rtw_render of radiance_ref.ray_blob through k_path and through the wavefront kernels - the shadow probe is
inline, deferred and queued respectively - and rtw_probe's irradiance at the receiver point."""
import numpy as np
import pytest

import law_common as C
import lighting_ref as L
from gpu_common import UPLOADS_LDS as UPLOADS, check_both, gpu, probe_is_pi_times_radiance, radiance_observed, render_observed  # noqa: F401
from gpu_common import upload_lds as upload

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- entry 1: rtw_radiance, one sample per ray, keys by key_offset
# (the second of the generator's independent samples as uploaded only; a case without draws has only the first)
@pytest.mark.parametrize("name,how,rng,est,seed,base", C.runs(L, hows=list(UPLOADS), draws=slice(0, 1)) + C.runs(L, hows=["as_uploaded"], draws=slice(1, 2)))
def test_radiance_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base):
    """The float64 reference first, the oracle's bits and probe count second."""
    check_both(L, name, radiance_observed(gpu, monkeypatch, L.case(name), how, rng, est, seed, base), (rng, est, seed, base), L.COUNTS)


# ---------------------------------------------------------------- entry 2: rtw_render of the ray's own blob
@pytest.mark.parametrize("path", ["1", "0"])  # k_path (the default) / the wavefront kernels
@pytest.mark.parametrize("name,how,rng,est,seed,base", C.runs(L, hows=["as_uploaded"], draws=slice(0, 1)))
def test_render_matches_float64_reference_and_oracle(gpu, monkeypatch, name, how, rng, est, seed, base, path):
    check_both(L, name, render_observed(gpu, monkeypatch, L.case(name), path, rng, est, seed, base), (rng, est, seed, base), L.COUNTS)


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
    print(L.check_irradiance(name, out[:, :3], C.PI32))
    probe_is_pi_times_radiance(gpu, probes, out, rng, est)
