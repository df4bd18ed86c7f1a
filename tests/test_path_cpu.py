"""The CPU oracle's path loop - the depth limit, the throughput, Russian roulette, the NaN scrub - against tests/path_ref.py, a
float64 reading of the reference's raygen.cu:28-87 that shares nothing with the oracle: the shell (a stochastic path length with a
closed-form law for every sample), the corridor (a deterministic one, plain and textured), whole frames from a camera inside the
shell, irradiance and light probes there. Then the negative controls - the same checkers must reject the loops one could have
written instead -, the measured fp32 constants, and the input conditions the GPU tests rely on. Thresholds come from path_ref and
shading_ref alone."""
import functools
import math

import numpy as np
import pytest

import law_common as C
import path_ref as P
import radiance_ref as R
from raytracing_weekend_amd import abi

REF, CORR, NO_NEE, MIX = P.REF, P.CORR, P.NO_NEE, P.MIX


@pytest.mark.parametrize("name,rng,est,seed,base", C.runs(P))
def test_oracle_meets_the_law(name, rng, est, seed, base):
    samples, segments, shadow_rays = P.oracle_samples(name, rng, est, seed, base)
    print(P.check(name, samples, est, segments=segments, shadow_rays=shadow_rays))


# ---------------------------------------------------------------- the laws themselves
def test_lamp_probabilities_follow_from_the_lobes():
    assert P.lamp_probability(False) == pytest.approx(1 / 4, abs=1e-15) and P.lamp_probability(True) == pytest.approx(1 / 13, abs=1e-15)
    # the lobes' definitions, by quadrature over r2: sin^2 = r2 (cosine), tan^2 = 4 r2 / (1 - r2) (sampling.cuh:55-57)
    r2 = (np.arange(1 << 20) + 0.5) / (1 << 20)
    a2 = (P.LAMP_R / P.WALL_R) ** 2
    assert abs(np.mean(r2 < a2) - 1 / 4) < 2e-6
    sin2 = 4 * r2 / (4 * r2 + (1 - r2))
    assert abs(np.mean(sin2 < a2) - 1 / 13) < 2e-6


@pytest.mark.parametrize("est", [REF, CORR, NO_NEE, MIX])
def test_shell_law_has_the_closed_forms(est):
    """rho q / (1 - rho (1 - q)) at max_depth 50 up to what the depth cuts off, the red channel's values 0.8, 0.64 and 1, the
    lit share q sum ((1 - q)^(s-2) prod p_d), and the black wall's segment count 1 + 1 + (1 - q): the third hit ends the path."""
    q = P.lamp_probability(est == REF)
    law = P.shell_law(est, 50)
    print(f"estimator {est}: q = {q:.6f}, mean {law.m1}, lit share {law.alive:.6f}, segments {law.seg_mean:.6f} +- {math.sqrt(law.seg_var):.4f}")
    rho = np.array(P.RHO, np.float32).astype(np.float64)
    cut = float((rho.max() * (1 - q)) ** 48)  # what max_depth = 50 cuts off: 1e-6 under the reference lobe, 2e-11 under the cosine lobe
    assert np.allclose(law.m1, rho * q / (1 - rho * (1 - q)), rtol=0, atol=cut)
    assert np.allclose(law.m1, P.SHELL_MEANS_AT_50[est == REF], rtol=0, atol=cut + 1e-7)  # (0.8 is not a float32)
    red = np.unique(np.round(law.values[:, 0], 12))
    assert np.allclose(red, [0.64, 0.8, 1.0], atol=1e-7)
    s = law.s.astype(np.float64)
    pd = np.where(s >= 4, rho.max() ** 3 * rho.max() ** np.maximum(s - 4, 0), 1.0)
    assert np.allclose(law.probs, q * (1 - q) ** (s - 2) * pd, rtol=1e-12)
    assert np.allclose(law.values, rho[None, :] ** (s[:, None] - 1) / pd[:, None], rtol=1e-12)
    for depth in (3, 4, 50):
        black = P.case(f"shell_black_wall-d{depth}").laws(est)[0]
        assert black.seg_mean == pytest.approx(1 + 1 + (1 - q), abs=1e-12) and not black.lit
    assert P.case("shell_black_wall-d2").laws(est)[0].seg_mean == 2.0
    assert P.shell_law(est, 1).seg_mean == 1.0 and not P.shell_law(est, 1).lit
    assert [o.s for o in P.shell_law(est, 3).lit] == [2, 3]


def test_corridor_law_has_the_closed_forms():
    a = np.array(P.MIRROR, np.float32).astype(np.float64)
    for k in P.CORRIDOR_KS:
        law = P.case(f"corridor-k{k}-d50").laws(CORR)[0]
        alive = 1.0 if k < 3 else a.max() ** 3 * a.max() ** (k - 3)
        print(f"k = {k}: alive share {law.alive:.6f}, blue {law.values[0, 2]:.8f}, segments {law.seg_mean:.4f}")
        assert law.alive == pytest.approx(alive, rel=1e-12) and list(law.s) == [k + 1]
        assert law.values[0, 2] == pytest.approx(a[2] ** k / alive, rel=1e-12)       # the sky's blue is 1: the throughput itself
        uy = (-1) ** k / math.sqrt(2.0)
        assert law.values[0, 0] == pytest.approx((1 - 0.25 * (uy + 1)) * a[0] ** k / alive, rel=1e-12)
        assert not P.case(f"corridor-k{k}-d{k}").laws(CORR)[0].lit
    assert P.case("corridor-k2-d2").laws(REF)[0].seg_var == 0.0 and P.case("corridor-k2-d2").laws(REF)[0].seg_mean == 2.0


def test_chi2_survival_function_meets_the_tables():
    """The textbook 0.9999 quantiles: 15.137 (1 degree of freedom), 23.513 (4), 35.564 (10), 52.386 (20)."""
    for k, x in ((1, 15.137), (4, 23.513), (10, 35.564), (20, 52.386)):
        assert P.chi2_sf(x, k) == pytest.approx(1e-4, rel=2e-3), (k, P.chi2_sf(x, k))
    assert P.chi2_sf(0.0, 3) == pytest.approx(1.0) and P.chi2_sf(2.0, 2) == pytest.approx(math.exp(-1.0))


# ---------------------------------------------------------------- the constants and the input conditions
def test_measured_constants_hold():
    got = P.measure_constants()
    print(got)
    for k, v in got.items():
        C.measured_band(v, getattr(P, "MEASURED_CONSTANT_" + k), f"MEASURED_CONSTANT_{k}")


def test_input_conditions_hold():
    """What must be true before a GPU result means anything: the shell's rays meet the wall first; every bounce of the corridor lies
    a quarter unit inside the mirrors and no checker sign change is near; every texture channel is checked; the whole textured walk
    at float32 stays inside a quarter of its tolerance; at most 10 % of a frame's pixels are left out."""
    for name in P.CASES:
        c = P.case(name)
        if isinstance(c, P.ShellCase):
            assert c.first_hit_is_the_wall(), name
        else:
            margin, good = c.well_conditioned()
            assert margin >= 0.25 and good == 1.0, (name, margin, good)
            assert all(law.checked.all() for law in c.laws(REF)), name
            if c.textured:
                err = c.full_walk_error()
                print(f"{name}: the float32 walk uses {err:.3f} of the tolerance")
                assert err <= 0.25, (name, err)
    ks = [k for k in P.case("corridor_image-d50").ks]
    assert len(ks) == 32 and set(ks) == set(range(3, 9))
    assert len({(round(float(o[2]), 6), round(float(d[2]), 6)) for o, d in zip(P.case("corridor_image-d50").o, P.case("corridor_image-d50").d)}) >= 24
    vals = np.concatenate([P.case("corridor_checker-d50").vertices(j, CORR)[2] for j in range(32)])
    assert len(np.unique(vals, axis=0)) == 2  # both children of the checker are met
    for which in (0, 1):
        cls = P.classify(which)
        print(f"view {which}: {int((cls == 0).sum())} wall pixels, {int((cls == 1).sum())} lamp pixels, {float((cls < 0).mean()):.4f} left out")
        assert (cls < 0).mean() <= P.MAX_LEFT_OUT and (cls == 1).sum() >= 256 and (cls == 0).sum() >= 2048


def test_scene_preparation_accepts_the_scenes(tmp_path):
    """Everything rtw_upload_scene does before its first HIP call (csrc/rtw_scene.h through tests/native/scene_check.cpp) accepts the
    scenes - the wall's negative radius, the dark light with its emission of 0, the lamp of +inf, the textured mirrors - with the lists
    and with the tree forced, and its invariants hold for them."""
    import os
    import subprocess
    exe = str(tmp_path / "scene_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(abi.REPO_DIR, "tests", "native", "scene_check.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTW_")}
    for name in ("shell-r0-d50", "shell_dark_light-d50", "shell_black_wall-d4", "shell_nan_scrub-d50", "corridor-k12-d50", "corridor_checker-d50", "corridor_image-d50"):
        f = tmp_path / (name + ".blob")
        f.write_bytes(P.case(name).blob)
        for knobs in ({}, {"RTW_BRUTE_MAX": "0"}):
            out = subprocess.run([exe, "check", str(f)], capture_output=True, text=True, env=dict(env, **knobs))
            print(name, knobs, out.stdout.strip(), out.stderr[-500:])
            assert out.returncode == 0, (name, knobs, out.stderr[-2000:])


# ---------------------------------------------------------------- negative controls: the checkers reject the other loops
rejected = functools.partial(C.rejected, P)


RHO_MAX = float(np.float32(max(P.RHO)))
A_MAX = float(np.float32(max(P.MIRROR)))
LOOPS = {
    "roulette_from_depth_1": dict(rr_from=1),
    "roulette_from_depth_3": dict(rr_from=3),
    "p_is_the_mean_of_T": dict(p_rule="mean"),
    "p_before_the_throughput_update": dict(p_before_update=True),
    "survival_without_rescale": dict(rescale=False),
}


@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("name", ["shell-r0-d50", "shell-r0-d5", "corridor-k4-d50", "corridor-k7-d50", "corridor_image-d50"])
def test_control_another_roulette_is_rejected(name, loop, est):
    rejected(name, est, **LOOPS[loop])


@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("name,shift", [("shell-r0-d4", 1), ("shell-r0-d4", -1), ("shell-r0-d2", 1), ("shell-r0-d2", -1), ("corridor-k3-d3", 1),
                                        ("corridor-k3-d4", -1), ("corridor-k7-d7", 1), ("corridor-k7-d8", -1), ("corridor_checker-d6", 1), ("corridor_checker-d6", -1)])
def test_control_another_depth_cut_is_rejected(name, shift, est):
    rejected(name, est, depth_shift=shift)


@pytest.mark.parametrize("name", ["shell-r0-d50", "shell-r0-d2", "shell-r2-d4", "shell_dark_light-d50"])
def test_control_the_other_lobe_is_rejected(name):
    rejected(name, REF, lobe="cosine")
    rejected(name, CORR, lobe="reference")


@pytest.mark.parametrize("est", [REF, CORR])
def test_control_p_2_squared_is_rejected(est):
    rejected("shell-r0-d50", est, p_override=lambda d, T: RHO_MAX ** 2 if d == 2 else None)
    rejected("corridor-k4-d50", est, p_override=lambda d, T: A_MAX ** 2 if d == 2 else None)


@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("name", ["corridor_checker-d50", "corridor_image-d50", "corridor_image-d6"])
def test_control_p_from_the_constant_albedo_is_rejected(name, est):
    rejected(name, est, constant_p=True)


@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("name", ["shell-r0-d50", "corridor-k7-d50", "corridor_image-d50"])
def test_control_the_oracle_without_roulette_is_rejected(name, est):
    """The other way round: a renderer that is wrong, under the right law. rtwo_set_debug(1) switches the oracle's roulette off (the
    hook of test_oracle_physics.py: the draws are consumed, nobody dies, nothing is rescaled)."""
    import oracle
    lib = oracle.load()
    lib.rtwo_set_debug(1)
    try:
        got = C.observe(oracle.render, P.case(name), abi.RTW_RNG_PHILOX, est, P.SEEDS[0], 0)
    finally:
        lib.rtwo_set_debug(0)
    with pytest.raises(AssertionError) as e:
        P.check(name, got.samples, est, segments=got.segments)
    print(f"{name}, estimator {est}: rejected, {str(e.value)[:300]}")


# ---------------------------------------------------------------- the NaN scrub's pixel, whole frames, the query family
@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("rng", P.RNGS)
def test_oracle_nan_scrub_pixel_is_inf_inf_0_1(rng, est):
    """64 samples of a ray in the shell whose lamp is +inf behind a wall without blue: (inf, inf, 0, 1) - some sample of the 64 meets
    the lamp (all fail with probability (1 - 0.28)^64 < 1e-9), and inf * 0 = NaN is scrubbed per channel, not per sample."""
    c = P.case("shell_nan_scrub-d50")
    pix, _, _ = R.expect(c.blob, np.repeat(c.o, 4, 0), np.repeat(c.ll, 4, 0), 64, 50, rng_kind=rng, estimator=est)
    assert np.array_equal(pix, np.broadcast_to(np.array([np.inf, np.inf, 0.0, 1.0], np.float32), (4, 4))), pix


@pytest.mark.parametrize("depth", [4, 50])
@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("rng", P.RNGS)
def test_oracle_frames_meet_the_law(rng, est, depth):
    frames, _, shadow = P.oracle_frames(rng, est, depth)
    for which in (0, 1):
        print(f"view {which}, estimator {est}, max_depth {depth}: " + P.check_frame(frames[which], which, est, depth))
    assert shadow == [0, 0]


@pytest.mark.parametrize("depth", [1, 4, 50])
@pytest.mark.parametrize("est", [REF, CORR])
@pytest.mark.parametrize("rng", P.RNGS)
def test_oracle_probes_meet_the_law(rng, est, depth):
    irradiance, sh = P.oracle_queries(rng, est, depth)
    print(f"estimator {est}, max_depth {depth}: " + P.check_irradiance(irradiance, est, depth))
    print(f"estimator {est}, max_depth {depth}: " + P.check_sh(sh, est, depth))


def test_control_probes_with_the_other_depth_convention_are_rejected():
    """Were the probe's own ray not counted among the max_depth segments, the laws of max_depth + 1 would hold: they do not."""
    irradiance, sh = P.oracle_queries(abi.RTW_RNG_PHILOX, CORR, 1)
    for check, out in ((P.check_irradiance, irradiance), (P.check_sh, sh)):
        check(out, CORR, 1)
        with pytest.raises(AssertionError):
            check(out, CORR, 2)
