"""GPU suite: the kernels against the reference's own device programs run on the CPU (tests/ref_programs.py; fixtures only, never
the reference tree). The level B frames through rtw_render on both pipelines and both uploads, level A's rays through rtw_cast, and
one level B frame's keys through rtw_radiance along the camera rays the reference's own camera callable produced."""
import functools

import numpy as np
import pytest

import geometry_ref as G
import ref_programs as RP
from gpu_common import UPLOADS, gpu, upload_lds  # noqa: F401  (gpu is a fixture)
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu


def _params(fx):
    w, h, depth = (int(v) for v in fx["meta"])
    return abi.make_params(w, h, 1, depth, rng_kind=abi.RTW_RNG_TEA_LCG, estimator=abi.RTW_EST_REFERENCE)


@pytest.mark.parametrize("name", list(RP.LEVEL_B))
def test_render_matches_the_reference_programs(gpu, monkeypatch, name):
    """Sample 0 of every pixel, TEA+LCG, the reference's estimator, by k_path (RTW_PATH=1) and by the wavefront kernels (0), as
    uploaded and with the tree forced: within TOLERANCE of the reference's frame on all but CAP of the samples, counts alike.
    (The four runs of a case share one test: they share its fixture, and the suite stays short.)"""
    fx = RP.fixture("b", name)
    for how in UPLOADS:
        for path in ("1", "0"):
            upload_lds(gpu, monkeypatch, fx["blob"], how)
            monkeypatch.setenv("RTW_PATH", path)
            img, st = gpu.render(_params(fx))
            assert np.all(img[..., 3] == 1.0), (how, path)
            print(RP.check_frame(name, fx, RP.display(img), st.segments, st.shadow_rays, what=f"rtw_render, RTW_PATH={path}, {how}"))


def test_render_check_rejects_reversed_rows(gpu, monkeypatch):
    """Negative control on the GPU's own frame: with its rows reversed it is rejected."""
    fx = RP.fixture("b", "cornell")
    upload_lds(gpu, monkeypatch, fx["blob"])
    img, _ = gpu.render(_params(fx))
    RP.check_frame("cornell", fx, RP.display(img))
    with pytest.raises(AssertionError):
        RP.check_frame("cornell", fx, RP.display(img)[::-1])


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    fx = RP.fixture("a", name)
    return fx, G.closest_hit(fx["blob"], fx["rays"], fx["ray_time"], fx["gather_time"])


@pytest.mark.parametrize("name", list(RP.LEVEL_A))
def test_cast_matches_the_reference_programs(gpu, monkeypatch, name):
    """Level A's rays through rtw_cast, as uploaded and with the tree forced: geometry_ref's check (its unit, K, mask and cap), and
    the primitive the reference's intersection programs commit on every well-conditioned ray."""
    fx, ref = geometry_case(name)
    good = ~ref["ill"]
    for how in UPLOADS:
        upload_lds(gpu, monkeypatch, fx["blob"], how)
        out = gpu.cast(fx["rays"], fx["ray_time"], fx["gather_time"], want=("t", "prim"))
        print(G.check_against(f"{name} (rtw_cast, {how})", ref, out["t"], out["prim"]))
        assert np.array_equal(out["prim"][good], fx["prim_plain"][good]), how


@pytest.mark.parametrize("name", ["cornell", "random21"])
def test_radiance_along_the_reference_camera_rays(gpu, monkeypatch, name):
    """The keys of a level B frame (perspective camera) through rtw_radiance along the rays the reference's camera callable gave
    for them: the reference's frame again."""
    fx = RP.fixture("b", name)
    upload_lds(gpu, monkeypatch, fx["blob"])
    w, h, depth = (int(v) for v in fx["meta"])
    n = w * h
    rays = np.concatenate([fx["camera_origin"], fx["camera_direction"], np.full((n, 1), 1e-6, np.float32), np.full((n, 1), 1e27, np.float32)], axis=1)
    st = abi.Stats()
    out = gpu.radiance(np.ascontiguousarray(rays, np.float32), 1, depth, rng_kind=abi.RTW_RNG_TEA_LCG, estimator=abi.RTW_EST_REFERENCE, key_offset=0, stats=st)
    print(RP.check_frame(name, fx, RP.display(out.reshape(h, w, 4)), st.segments, st.shadow_rays, what="rtw_radiance"))
