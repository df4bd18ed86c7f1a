"""The CPU oracle's direct lighting against tests/lighting_ref.py, a float64 reading of the reference's closest-hit, pdf and
material programs that shares nothing with the oracle: the light sample alone (max_depth = 1, the reference and the corrected
estimator), emitter hits after it (max_depth = 2, the three corrected estimators), point lights held to a float64 value. Thresholds
come from lighting_ref and shading_ref alone: 4 x the measured fp32-against-float64 constant for deterministic values, Kolmogorov
and binomial limits at alpha = 1e-4 for the laws."""
import functools

import numpy as np
import pytest

import law_common as C
import lighting_ref as L

REF, CORR, NO_NEE, MIX = L.REF, L.CORR, L.NO_NEE, L.MIX


@pytest.mark.parametrize("name,rng,est,seed,base", C.runs(L))
def test_oracle_matches_float64_reference(name, rng, est, seed, base):
    samples, shadow_rays = L.oracle_samples(name, rng, est, seed, base)
    print(L.check(name, samples, est, shadow_rays=shadow_rays))


@pytest.mark.parametrize("rng", L.RNGS)
@pytest.mark.parametrize("name", ["two_emitters_one_unlisted-d2", "occluded-d2", "own_emitter-d2"])
def test_oracle_irradiance_is_pi_times_the_emitters_form_factors(name, rng):
    """rtw_probe's irradiance at the receiver point as the oracle gives it: the probes' own directions (probe_ref.directions), one
    segment each, pi times the radiance - pi * Le of the emitter met, listed or not, since no light sample came before."""
    import probe_ref
    import radiance_ref as R
    c = L.case(name)
    probes = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1e-3, 1e27], np.float32), (L.N_RARE, 1))
    rays = probe_ref.rays_of(probes, probe_ref.directions(probes, 1, rng_kind=rng), 0)
    pix, _, _ = R.expect(c.blob, rays[:, :3], (rays[:, :3] + rays[:, 3:6]).astype(np.float32), 1, 1, rng_kind=rng, estimator=CORR)
    print(L.check_irradiance(name, pix[:, :3] * C.PI32))


def test_the_cases_are_what_their_names_say():
    """The geometry the laws rely on: the skewed light straddles the horizon and keeps 0.29 of the draws, the occluder's shadow
    lies inside the light above, the unlisted emitter is not a listed one, the medium's transmittance has power both ways."""
    c = L.case("three_lights-d1")
    heights = c.lights[2].polygon()[:, 1]
    assert heights.min() < 0 < heights.max()
    assert abs(c.sample_law(CORR).tables[2].share - 0.2917) < 2e-4
    assert [t.share for t in c.sample_law(CORR).tables[:2]] == [pytest.approx(1 / 3), pytest.approx(1 / 3)]
    assert c.pdf_rect[2] != c.lights[0].position[1] and c.pdf_rect[1] != (-1.0, 1.0, -0.5, 1.0)
    o = L.case("occluded-d2")
    hits = o.hit_law(False)
    assert hits.listed == [False, True, True, False, False] and hits.emitters == [1, 2, 3]
    open_ = L.case("two_emitters_one_unlisted-d2").hit_law(False)
    assert hits.visible[1] < open_.visible[1] and hits.visible[2] == open_.visible[2] and hits.visible[3] == open_.visible[3]
    assert len(L.shadows_on(1, 2.0, L.E_ABOVE.polygon(), [L.OCCLUDER])) == 1
    own = L.case("own_emitter-d1")
    moved, listed = L.moved_lights(own.lights, own.rects)
    assert listed == [False, True] and moved[0].position[1] == pytest.approx(200.9) and own.lights[0].position[1] == 200.0
    assert 0.05 < L.case("through_medium-d1").transmittance() < 0.95
    assert abs(L.case("through_medium-d1").transmittance() - np.exp(-1.0)) < 1e-6
    assert len(L.POINT_LIGHTS) == 12
    for name, thin in (("probe_far_end-d1", L.THIN_FAR), ("probe_near_end-d1", L.THIN_NEAR)):
        c = L.case(name)
        corners = L.L_ABOVE.polygon()
        gaps = [np.linalg.norm(p) * (1 - thin.k / p[1]) if thin is L.THIN_FAR else np.linalg.norm(p) * thin.k / p[1] for p in corners]
        assert L.PROBE_EPS * 4 < min(gaps) and max(gaps) * 1.5 < L.CORRECTED_EPS  # between the two intervals, with room for fp32
        assert c.sample_law(REF).tables[0].share == pytest.approx(0.5) and c.sample_law(CORR).tables[0].share == 1.0
    at = -L.case("probe_near_end-d1").d[0] * L.THIN_NEAR.k  # where the camera ray crosses the near rectangle's plane: beside it
    assert at[1] == L.THIN_NEAR.k and not L.THIN_NEAR.ext[0] <= at[0] <= L.THIN_NEAR.ext[1]


# ---------------------------------------------------------------- the constant and the grids
def test_measured_constant_holds():
    got = L.measure_constant()
    print(got)
    C.measured_band(got, L.MEASURED_CONSTANT_LIGHT, "MEASURED_CONSTANT_LIGHT")


def test_grids_agree_with_the_closed_forms_and_with_themselves():
    """The means against Lambert's formula, everything against the grid at half resolution, relative. 1e-5 is a four-hundredth of
    the standard error of a mean over 65536 samples whose standard deviation equals their mean, the sharpest mean asserted here."""
    extremes = 0.0
    for what, err in L.quadrature_errors().items():
        print(f"{what}: {err:.2e}")
        assert err < 1e-5, what
        if what.endswith("extremes"):
            extremes = max(extremes, err)
    C.measured_band(extremes, L.MEASURED_GRID_RANGE, "MEASURED_GRID_RANGE")


# ---------------------------------------------------------------- negative controls: the laws reject wrong models
rejected = functools.partial(C.rejected, L)


@pytest.mark.parametrize("est", [REF, CORR])
def test_control_no_n_lights_factor_is_rejected(est):
    rejected("three_lights-d1", est, n_lights_factor=False)


@pytest.mark.parametrize("name,est", [("three_lights-d1", REF), ("three_lights-d1", CORR), ("occluded-d1", CORR), ("own_emitter-d1", CORR)])
def test_control_area_2_percent_off_is_rejected(name, est):
    rejected(name, est, area_factor=1.02)


@pytest.mark.parametrize("est", [REF, CORR])
def test_control_point_light_2_percent_off_is_rejected(est):
    rejected("point00-d1", est, value_factor=1.02)
    rejected("point06-d1", est, value_factor=1.0 + 4 * L.K_FACTOR * L.MEASURED_CONSTANT_LIGHT * L.U)  # four times the bound


def test_control_unclipped_horizon_is_rejected():
    rejected("three_lights-d1", CORR, clip_horizon=False)


@pytest.mark.parametrize("name", ["three_lights-d1", "nonwhite_pair-d1", "own_emitter-d1"])
def test_control_omitted_heuristic_weight_is_rejected(name):
    rejected(name, REF, heuristic=False)


def test_control_the_lights_own_rectangle_under_the_reference_estimator_is_rejected():
    rejected("three_lights-d1", REF, own_rectangle=True)


@pytest.mark.parametrize("name", ["probe_far_end-d1", "probe_near_end-d1"])
def test_control_the_other_estimators_probe_interval_is_rejected(name):
    """A thin rectangle 4.9e-4 from an end of the probe shadows under the reference estimator (5e-5) and not under the corrected one
    (1e-3): either law with the other's interval is off by half the samples."""
    rejected(name, CORR, eps=L.PROBE_EPS)
    rejected(name, REF, eps=L.CORRECTED_EPS)


def test_control_one_sided_light_density_is_rejected():
    rejected("mixture_behind-d2", MIX, two_sided=False)


def test_control_the_definitions_plane_under_the_corrected_estimator_is_rejected():
    """own_emitter: the definition lies 0.9 below the rectangle it describes; the corrected estimator samples the
    rectangle's plane, and a law that samples the definition's is 0.9 % off at a distance of 200."""
    rejected("own_emitter-d1", CORR, unmoved=True)


@pytest.mark.parametrize("name", ["two_emitters_one_unlisted-d2", "occluded-d2"])
def test_control_light_density_without_one_over_n_lights_is_rejected(name):
    rejected(name, MIX, one_over_n_lights=False)


@pytest.mark.parametrize("name", ["two_emitters_one_unlisted-d2", "occluded-d2", "own_emitter-d2", "nonwhite_pair-d2"])
def test_control_listed_emitter_counted_after_a_light_sample_is_rejected(name):
    rejected(name, CORR, count_listed_hits=True)
