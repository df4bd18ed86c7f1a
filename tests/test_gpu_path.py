"""The kernels' path loop - the depth limit, the throughput, Russian roulette, the NaN scrub - against tests/path_ref.py (a float64
reading of the reference's raygen.cu:28-87 that shares nothing with the oracle or the kernels), then against the oracle's bits and
counts of the same keys, so that a failure says which side moved. Entries: rtw_radiance on the cases' rays (uploaded as is, with the
tree forced, with the tree outside LDS); rtw_render of radiance_ref.ray_blob - every pixel the same ray on its own key - through
k_path and through the wavefront kernels; whole frames from a camera inside the shell through rtw_render (both pipelines) and
rtw_views; rtw_probe and rtw_probe_sh in the shell."""
import numpy as np
import pytest

import law_common as C
import path_ref as P
import radiance_ref as R
import shading_ref as S
from gpu_common import UPLOADS_LDS as UPLOADS, check_both, gpu, radiance_observed, render_observed  # noqa: F401
from gpu_common import upload_lds as upload
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- entry 1: rtw_radiance, one sample per ray, keys by key_offset
# (the second of the generator's independent samples as uploaded only)
@pytest.mark.parametrize("name,how,rng,est,seed,base", C.runs(P, hows=list(UPLOADS), draws=slice(0, 1)) + C.runs(P, hows=["as_uploaded"], draws=slice(1, 2)))
def test_radiance_meets_the_law_and_the_oracle(gpu, monkeypatch, name, how, rng, est, seed, base):
    """The float64 law first, the oracle's bits and counts second."""
    check_both(P, name, radiance_observed(gpu, monkeypatch, P.case(name), how, rng, est, seed, base), (rng, est, seed, base), P.COUNTS)


# ---------------------------------------------------------------- entry 2: rtw_render of the ray's own blob, one upload per ray
@pytest.mark.parametrize("path", ["1", "0"])  # k_path (the default) / the wavefront kernels
@pytest.mark.parametrize("name,how,rng,est,seed,base", C.runs(P, hows=["as_uploaded"], draws=slice(0, 1)))
def test_render_meets_the_law_and_the_oracle(gpu, monkeypatch, name, how, rng, est, seed, base, path):
    check_both(P, name, render_observed(gpu, monkeypatch, P.case(name), path, rng, est, seed, base), (rng, est, seed, base), P.COUNTS)


def test_dark_light_render_runs_the_one_light_route(gpu, monkeypatch):
    """One listed rectangle light, the reference estimator, Philox, no textures: the scene rtw_hip.hip hands to k_path's one-light
    instantiation. The call reports success, k_path did the work and probes were traced."""
    for k in ("RTW_BRUTE_MAX", "RTW_LDS_KB", "RTW_PATH"):
        monkeypatch.delenv(k, raising=False)
    c = P.case("shell_dark_light-d50")
    gpu.upload_scene(R.ray_blob(c.blob, c.o[0], c.ll[0]))  # a refusal (a black light, say) raises here
    img, st = gpu.render(S.render_params(c, 0, abi.RTW_RNG_PHILOX, P.REF, P.SEEDS[0]))
    assert st.kernel_launches[abi.Stats.KERNELS.index("k_path")] > 0 and st.shadow_rays > 0 and np.isfinite(img).all()


# ---------------------------------------------------------------- the NaN scrub's pixel
@pytest.mark.parametrize("est", [P.REF, P.CORR])
@pytest.mark.parametrize("rng", P.RNGS)
def test_nan_scrub_pixel_is_inf_inf_0_1(gpu, monkeypatch, rng, est):
    """64 samples per ray, the lamp +inf behind a wall without blue: (inf, inf, 0, 1) from rtw_radiance and from both pipelines of
    rtw_render - inf * 0 = NaN is scrubbed per channel, and the sums carry inf."""
    c = P.case("shell_nan_scrub-d50")
    want = np.array([np.inf, np.inf, 0.0, 1.0], np.float32)
    upload(gpu, monkeypatch, c.blob, "as_uploaded")
    out = gpu.radiance(np.repeat(R.make_rays(c.o, c.ll, est), 64, 0), 64, 50, rng_kind=rng, estimator=est)
    assert np.array_equal(out, np.broadcast_to(want, out.shape)), out[(out != want).any(1)][:4]
    gpu.upload_scene(R.ray_blob(c.blob, c.o[0], c.ll[0]))
    for path in ("1", "0"):
        monkeypatch.setenv("RTW_PATH", path)
        img, _ = gpu.render(abi.make_params(8, 8, 64, 50, rng_kind=rng, estimator=est))
        assert np.array_equal(img, np.broadcast_to(want, img.shape)), (path, img[(img != want).any(-1)][:4])


# ---------------------------------------------------------------- whole frames: regeneration, many samples per lane, block and unit sums
def check_frames(got, segments, shadow_rays, which, rng, est, depth):
    want, want_segments, want_shadow = P.oracle_frames(rng, est, depth)
    for i, w in enumerate(which):
        print(f"view {w}, estimator {est}, max_depth {depth}: " + P.check_frame(got[i], w, est, depth))
    for i, w in enumerate(which):
        differ = int((got[i].view(np.uint32) != want[w].view(np.uint32)).any(-1).sum())
        print(f"view {w}: {differ} pixels differ from the oracle's")
        assert differ == 0
    assert (segments, shadow_rays) == (sum(want_segments[w] for w in which), sum(want_shadow[w] for w in which))


@pytest.mark.parametrize("depth", [4, 50])
@pytest.mark.parametrize("est", [P.REF, P.CORR])
@pytest.mark.parametrize("rng", P.RNGS)
@pytest.mark.parametrize("path", ["1", "0"])
def test_rendered_frame_meets_the_law_and_the_oracle(gpu, monkeypatch, path, rng, est, depth):
    for k in ("RTW_BRUTE_MAX", "RTW_LDS_KB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTW_PATH", path)
    view = P.frame_views()[0]
    gpu.upload_scene(P.frame_blob(view))
    img, st = gpu.render(abi.make_params(P.FRAME_SIDE, P.FRAME_SIDE, P.FRAME_SPP, depth, seed=view.seed, rng_kind=rng, estimator=est))
    check_frames(img[None], int(st.segments), int(st.shadow_rays), (0,), rng, est, depth)


@pytest.mark.parametrize("depth", [4, 50])
@pytest.mark.parametrize("est", [P.REF, P.CORR])
@pytest.mark.parametrize("rng", P.RNGS)
def test_views_meet_the_law_and_the_oracle(gpu, monkeypatch, rng, est, depth):
    """One perspective and one environment view in one call."""
    upload(gpu, monkeypatch, P.shell_blob(), "as_uploaded")
    st = abi.Stats()
    frames = gpu.views(list(P.frame_views()), P.FRAME_SIDE, P.FRAME_SIDE, P.FRAME_SPP, depth, rng_kind=rng, estimator=est, stats=st)
    check_frames(frames, int(st.segments), int(st.shadow_rays), (0, 1), rng, est, depth)


# ---------------------------------------------------------------- the query family: rtw_probe at a wall point, rtw_probe_sh at a free point
@pytest.mark.parametrize("depth", [1, 4, 50])
@pytest.mark.parametrize("est", [P.REF, P.CORR])
@pytest.mark.parametrize("rng", P.RNGS)
def test_probes_meet_the_law(gpu, monkeypatch, rng, est, depth):
    upload(gpu, monkeypatch, P.shell_blob(), "as_uploaded")
    probes = np.tile(np.array(P.WALL_PROBE, np.float32), (P.QUERY_N, 1))
    out = gpu.probe(probes, P.QUERY_SPP, depth, rng_kind=rng, estimator=est)
    print(f"estimator {est}, max_depth {depth}: " + P.check_irradiance(out, est, depth))
    points = np.tile(np.array(P.FREE_POINT, np.float32), (P.QUERY_N, 1))
    sh = gpu.probe_sh(points, P.QUERY_SPP, depth, rng_kind=rng, estimator=est)
    print(f"estimator {est}, max_depth {depth}: " + P.check_sh(sh, est, depth))
