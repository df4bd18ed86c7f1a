"""CPU suite: the reference's own device programs, run on the CPU (oracle/ref_programs_wrap.cpp), as a referee. Where the live
libraries exist the committed fixtures equal them bit for bit; everything else reads the fixtures. Level A holds geometry_ref.py, the
float64 second reading, to the text; level B holds the oracle to the text (tests/ref_programs.py says how, and why at depth 1)."""
import functools

import numpy as np
import pytest

import geometry_ref as G
import law_common
import oracle
import ref_programs as RP
from raytracing_weekend_amd import abi

live = pytest.mark.skipif(not RP.have_live(), reason="oracle/_ref/libref_programs*.so are built only where the reference tree is")


def test_the_tolerance_is_four_times_the_measured_constant():
    assert RP.TOLERANCE == 4.0 * RP.MEASURED_CONSTANT_SAMPLE and RP.K_FACTOR == law_common.K_FACTOR == 4.0
    assert RP.CAP == 0.01 and RP.BUILDS_CAP == 0.0025 and RP.TOLERANCE < RP.DECISION
    assert set(RP.SHARES) == set(RP.LEVEL_B) and RP.DEPTH == 1


# ---------------------------------------------------------------- the fixtures are the live libraries' output
@live
@pytest.mark.parametrize("name", list(RP.LEVEL_B))
def test_level_b_fixture_equals_the_live_libraries(name):
    fx = RP.fixture("b", name)
    w, h, depth = (int(v) for v in fx["meta"])
    for build in RP.BUILDS:
        frame, counts = RP.launch(build, fx["blob"], w, h, depth)
        assert np.array_equal(frame[..., :3].view(np.uint32), fx[f"frame_{build}"].view(np.uint32)) and np.all(frame[..., 3] == 1.0), build
        assert np.array_equal(counts, fx[f"counts_{build}"]), build
    o, d = RP.camera_rays("plain", fx["blob"], w, h)
    assert np.array_equal(o.view(np.uint32), fx["camera_origin"].view(np.uint32)) and np.array_equal(d.view(np.uint32), fx["camera_direction"].view(np.uint32))
    assert fx["blob"] == RP.LEVEL_B[name](), "the case's scene is no longer the fixture's"


@live
@pytest.mark.parametrize("name", list(RP.LEVEL_A))
def test_level_a_fixture_equals_the_live_libraries(name):
    fx = RP.fixture("a", name)
    rays, rt, gt = RP.level_a_rays(fx["blob"])
    assert np.array_equal(rays, fx["rays"]) and np.array_equal(rt, fx["ray_time"]) and np.array_equal(gt, fx["gather_time"])
    for build in RP.BUILDS:
        for k, v in RP.intersect(build, fx["blob"], rays, rt, gt).items():
            assert np.array_equal(np.ascontiguousarray(v).view(np.uint32), fx[f"{k}_{build}"].view(np.uint32)), (build, k)


# ---------------------------------------------------------------- the reference against itself
def test_measured_constant_and_the_builds_agreement():
    """MEASURED_CONSTANT_SAMPLE re-measured from both builds' frames, and the condition on the cases: the builds disagree on at
    most 0.25 % of a case's samples."""
    constant = 0.0
    for name in RP.LEVEL_B:
        differ, c = RP.builds_disagree(RP.fixture("b", name))
        constant = max(constant, c)
        print(f"{name}: constant {c:.4e}, the builds disagree on {100 * differ.mean():.3f} % of the samples")
        assert differ.mean() <= RP.BUILDS_CAP, name
        rel = RP.relative(RP.fixture("b", name)["frame_plain"], RP.fixture("b", name)["frame_fma"]).max(-1)
        assert not ((rel > RP.TOLERANCE) & (rel <= RP.DECISION)).any(), f"{name}: a sample between the two modes"
        assert abs(differ.mean() - RP.SHARES[name][0]) < 1e-6, (name, differ.mean())
    law_common.measured_band(constant, RP.MEASURED_CONSTANT_SAMPLE, "MEASURED_CONSTANT_SAMPLE")


# ---------------------------------------------------------------- level A: geometry_ref against the text
@functools.lru_cache(maxsize=None)
def geometry_case(name):
    fx = RP.fixture("a", name)
    return fx, G.closest_hit(fx["blob"], fx["rays"], fx["ray_time"], fx["gather_time"])


@pytest.mark.parametrize("build", list(RP.BUILDS))
@pytest.mark.parametrize("name", list(RP.LEVEL_A))
def test_float64_closest_hit_matches_the_reference_programs(name, build):
    """geometry_ref.closest_hit on 2 000 of its own rays against what the reference's intersection programs report under closest-hit
    commit: its error unit, its K, its conditioning mask, its cap (check_against) - nothing new."""
    fx, ref = geometry_case(name)
    print(G.check_against(f"{name} ({build})", ref, fx[f"t_{build}"], fx[f"prim_{build}"]))
    hit = fx[f"prim_{build}"] >= 0
    assert np.all(fx[f"reported_{build}"][~hit] == 0) and np.all(fx[f"reported_{build}"][hit] >= 1)
    # the oracle picks the text's primitive on every well-conditioned ray
    t, prim = oracle.intersect(fx["blob"], fx["rays"], fx["ray_time"], fx["gather_time"])
    good = ~ref["ill"]
    assert np.array_equal(prim[good], fx[f"prim_{build}"][good])


def test_level_a_rejects_a_motion_transform_left_out():
    """Negative control: a float64 reading without the matrix-motion transform (ray time 0 for every ray) is rejected by the
    reference's hits of the moving-sphere scene. (Exchanging the two times would not show: with the keys at 0 and 1 the sphere's
    place depends on their sum.)"""
    fx = RP.fixture("a", "random16_motion")
    wrong = G.closest_hit(fx["blob"], fx["rays"], np.zeros_like(fx["ray_time"]), fx["gather_time"])
    with pytest.raises(AssertionError) as e:
        G.check_against("random16_motion, no motion transform", wrong, fx["t_plain"], fx["prim_plain"])
    print(str(e.value)[:300])


CAMERAS = {"cornell": ("b", "cornell", ""), "environment": ("b", "cornell_environment", ""), "orthographic": ("b", "cornell_orthographic", ""),
           "lens": ("a", "camera_lens", "_plain"), "lens_fma": ("a", "camera_lens", "_fma")}


@pytest.mark.parametrize("which", list(CAMERAS))
def test_float64_camera_rays_match_the_reference_callables(which):
    """camera_ref's rays for all three camera kinds, and the perspective camera with a lens, against the reference's camera
    callables on raygen.cu's own (s, t, seed)."""
    level, name, suffix = CAMERAS[which]
    fx = RP.fixture(level, name)
    print(RP.check_camera(which, fx["blob"], fx["camera_origin" + suffix], fx["camera_direction" + suffix]))


@live
def test_camera_lens_fixture_equals_the_live_libraries():
    fx = RP.fixture("a", "camera_lens")
    assert fx["blob"] == RP.lens_blob()
    for build in RP.BUILDS:
        o, d = RP.camera_rays(build, fx["blob"], RP.SIDE, RP.SIDE)
        assert np.array_equal(o.view(np.uint32), fx[f"camera_origin_{build}"].view(np.uint32)), build
        assert np.array_equal(d.view(np.uint32), fx[f"camera_direction_{build}"].view(np.uint32)), build


@pytest.mark.parametrize("which, wrong", [("lens", "lens_sin_cos_swapped"), ("environment", "plus_cos"), ("orthographic", "ortho_origin_once"),
                                          ("cornell", "swap_jitter")])
def test_camera_check_rejects_a_wrong_reading(which, wrong):
    """Negative controls: camera_ref's own wrong readings are rejected by the reference's rays."""
    level, name, suffix = CAMERAS[which]
    fx = RP.fixture(level, name)
    with pytest.raises(AssertionError) as e:
        RP.check_camera(which, fx["blob"], fx["camera_origin" + suffix], fx["camera_direction" + suffix], **{wrong: True})
    print(f"{wrong}: rejected, {str(e.value)[:200]}")


@pytest.mark.parametrize("build", list(RP.BUILDS))
@pytest.mark.parametrize("name", RP.TEXTURES)
def test_float64_textures_match_the_reference_callables(name, build):
    """shading_ref's noise and checker values at its own 2 000 points per case against the reference's texture callables: that
    file's unit, its per-case constant, its mask (|sin| < SIN_EPS) and its cap (TextureCase.check)."""
    import shading_ref
    fx = RP.fixture("a", "textures")
    c = shading_ref.case("texture-" + name)
    assert np.array_equal(c.points, fx[f"{name}_points"])
    print(f"{name} ({build}): " + c.check(fx[f"{name}_{build}"][:, None, :], law_common.REF))


def test_texture_check_rejects_the_other_checker_phase():
    """Negative control: a reading with sin(10 y) in place of sin(10 - y) is rejected by the reference's checker values."""
    import shading_ref
    fx = RP.fixture("a", "textures")
    c = shading_ref.case("texture-checker_constants")
    with pytest.raises(AssertionError):
        c.check(fx["checker_constants_plain"][:, None, :], law_common.REF, checker_py="10y")


@live
def test_texture_fixture_equals_the_live_libraries():
    import shading_ref
    fx = RP.fixture("a", "textures")
    for name in RP.TEXTURES:
        c = shading_ref.case("texture-" + name)
        for build in RP.BUILDS:
            assert np.array_equal(RP.texture_values(build, c.blob, 0, c.points).view(np.uint32), fx[f"{name}_{build}"].view(np.uint32)), (name, build)


LAWS = [(m, n) for m, names in RP.LAW_CASES.items() for n in names]


@pytest.mark.parametrize("build", list(RP.BUILDS))
@pytest.mark.parametrize("module, name", LAWS)
def test_float64_law_matches_the_reference_programs(module, name, build):
    """shading_ref's mirror / glass directions on its INCIDENCES and lighting_ref's depth-1 light sample (which light, where on the
    pdf rectangle, pdf, heuristic weight, the numLights factor, the probe) against samples that the reference's own closest-hit
    program, material, pdf and miss callables produced for the case's rays: the law file's own check, its unit, K, mask and cap."""
    m, ob = RP.law_module(module), RP.law_fixture(module, name, build)
    print(m.check(name, ob.samples, law_common.REF, **law_common.counts_of(m, ob)))
    # and the oracle's counts are the text's (its samples are held to the same law by test_shading_cpu / test_lighting_cpu)
    want = law_common.oracle_samples(m.case(name), abi.RTW_RNG_TEA_LCG, law_common.REF, law_common.SEEDS[0], 0)
    assert (ob.segments, ob.shadow_rays) == (want.segments, want.shadow_rays)


@live
@pytest.mark.parametrize("module, name", LAWS)
def test_law_fixture_equals_the_live_libraries(module, name):
    for build in RP.BUILDS:
        ob, fx = RP.law_samples(build, module, name), RP.law_fixture(module, name, build)
        assert np.array_equal(ob.samples.view(np.uint32), fx.samples.view(np.uint32)) and ob[1:] == fx[1:], build


@pytest.mark.parametrize("module, name, wrong", [
    ("shading_ref", "direction-glass_above", {"schlick_exponent": 4}), ("shading_ref", "direction-glass_below", {"invert_back_eta": True}),
    ("lighting_ref", "three_lights-d1", {"n_lights_factor": False}), ("lighting_ref", "three_lights-d1", {"own_rectangle": True}),
    ("lighting_ref", "nonwhite_pair-d1", {"heuristic": False}), ("lighting_ref", "nonwhite_pair-d1", {"area_factor": 1.02}),
    ("lighting_ref", "probe_far_end-d1", {"eps": 1e-3}), ("lighting_ref", "point00-d1", {"value_factor": 1.02})])
def test_law_check_rejects_a_wrong_reading(module, name, wrong):
    """Negative controls: the law files' own wrong models are rejected by the reference's samples (the right one passes on them)."""
    law_common.rejected(RP.law_module(module), name, law_common.REF, observed=RP.law_fixture(module, name, "plain"), **wrong)


# ---------------------------------------------------------------- level B: the oracle against the text
@functools.lru_cache(maxsize=None)
def oracle_case(name, sample=0):
    fx = RP.fixture("b", name)
    frame, st = RP.oracle_frame(fx["blob"], int(fx["meta"][2]), sample)
    frame.setflags(write=False)
    return fx, frame, st


@pytest.mark.parametrize("name", list(RP.LEVEL_B))
def test_oracle_frame_matches_the_reference_programs(name):
    fx, frame, st = oracle_case(name)
    fig = RP.check_frame(name, fx, frame, st.segments, st.shadow_rays)
    print(fig)
    outside = float((RP.relative(frame, fx["frame_plain"]).max(-1) > RP.TOLERANCE).mean())
    assert abs(outside - RP.SHARES[name][1]) < 1e-6, (name, outside)  # the recorded share is the measured one
    # the single-path entry point gives the frame's samples
    lib = oracle.load()
    p = abi.make_params(RP.SIDE, RP.SIDE, 1, int(fx["meta"][2]), rng_kind=abi.RTW_RNG_TEA_LCG, estimator=abi.RTW_EST_REFERENCE)
    rgb = np.zeros(3, np.float32)
    for x, y in ((0, 0), (17, 40), (63, 63)):
        assert lib.rtwo_trace_pixel(fx["blob"], len(fx["blob"]), p, x, y, 0, rgb.ctypes.data) == 0
        assert np.array_equal(RP.display(rgb), frame[y, x])


def test_level_b_rejects_another_sample_and_reversed_rows():
    """Negative controls: the oracle's sample 1 in place of sample 0, and the fixture's frame with its rows reversed."""
    fx, frame, st = oracle_case("cornell")
    RP.check_frame("cornell", fx, frame, st.segments, st.shadow_rays)
    _, other, st1 = oracle_case("cornell", 1)
    for what, got in (("sample 1", other), ("rows reversed", frame[::-1])):
        with pytest.raises(AssertionError) as e:
            RP.check_frame("cornell", fx, got, what=what)
        print(str(e.value).split("\n")[0])
