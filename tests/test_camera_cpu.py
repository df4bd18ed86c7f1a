"""The CPU oracle's camera rays and the camera builders against tests/camera_ref.py, a float64 reading of the reference's camera,
raygen and sampling programs that shares nothing with the oracle: its generators (numpy integer arithmetic) against the known
answers, oracle.render against the law for every case, generator, draw, frame and sample offset, one mean of 144 samples per camera
kind, negative controls (the law with one thing changed must fail on the oracle's samples), and bake's, the host description's and
view_ref's cameras against the float64 ioCamera law. Thresholds come from camera_ref alone: 4 x the measured fp32-against-float64
constants, exact equality on well-conditioned samples, at most 2 % left out."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import camera_ref as L
import view_ref as V
from law_common import measured_band
from raytracing_weekend_amd import abi, bake

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "rng_kat.json")))
PHILOX, TEA_LCG = L.PHILOX, L.TEA_LCG


# ---------------------------------------------------------------- the generators
def test_tea_matches_the_reference_builds_vectors():
    for n, key in ((64, "tea64"), (16, "tea16"), (4, "tea4")):
        a, b, want = (np.array(col, np.uint64) for col in zip(*KAT[key]))
        assert np.array_equal(L.tea(n, a, b), want), key
    px, smp, want = (np.array(col, np.uint64) for col in zip(*KAT["tea64_frame"]))
    assert np.array_equal(L.tea(64, px, smp), want)
    # SURVEY.md section 8c (captured from the reference header)
    assert [int(L.tea(64, a, 0)) for a in (0, 1, 1919, 1920 * 1079 + 1919)] == [0x437C1053, 0x4E7B0C67, 0x30EA8DA9, 0x6809BAFA]
    assert int(L.tea(16, 0, 0)) == 0x741C187D and int(L.tea(4, 7, 3)) == 0x81A8A401


def test_lcg_is_the_published_recurrence():
    # OptiX SDK cuda/random.h: prev = 1664525 * prev + 1013904223; (prev & 0xFFFFFF) / 2^24
    state = 0x437C1053
    st = np.array([state, 0xFFFFFFFF, 0], np.uint64)
    py = [state, 0xFFFFFFFF, 0]
    for _ in range(100):
        py = [(1664525 * p + 1013904223) & 0xFFFFFFFF for p in py]
        st, u = L.lcg(st)
        assert [int(x) for x in st] == py
        assert [float(x) for x in u] == [(p & 0xFFFFFF) / 16777216.0 for p in py]
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and (u < 1.0).all()


def test_philox_random123_known_answers():
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, want in cases:
        assert tuple(int(w) for w in L.philox4x32_10(ctr, key)) == want
    # elementwise over arrays: the three cases at once
    ctr = [np.array([c[0][i] for c in cases], np.uint64) for i in range(4)]
    key = [np.array([c[1][i] for c in cases], np.uint64) for i in range(2)]
    got = L.philox4x32_10(ctr, key)
    assert [[int(got[i][j]) for i in range(4)] for j in range(3)] == [list(c[2]) for c in cases]
    assert float(L.u24(0xFFFFFFFF)) == (2 ** 24 - 1) / 2 ** 24 and float(L.u24(0xFF)) == 0.0


def test_the_draws_are_what_the_law_says():
    key, smp = np.arange(5, dtype=np.uint64) + 1000, np.uint64(3)
    p, e = (L.draws(key, smp, 7, TEA_LCG, k) for k in (L.PERSP, L.ENV))
    st = L.tea(64, key, smp)
    seq = []
    for _ in range(5):
        st, u = L.lcg(st)
        seq.append(u)
    assert all(np.array_equal(p[n], seq[i]) for i, n in enumerate(("r0", "r1", "r2", "r3", "r4")))
    assert all(np.array_equal(e[n], seq[i]) for i, n in enumerate(("r0", "r1", "r4"))) and not e["r2"].any() and not e["r3"].any()
    assert p["rt"] is p["r4"] and e["rt"] is e["r4"]  # the first ray time is the gather draw's LCG output
    assert np.array_equal(L.draws(key, smp, 8, TEA_LCG, L.PERSP)["r0"], p["r0"])  # no seed
    a, b = (L.draws(key, smp, 7, PHILOX, k) for k in (L.PERSP, L.ORTHO))
    assert all(np.array_equal(a[n], b[n]) for n in a)  # positional: the same for every camera kind
    w = L.philox4x32_10((key, smp, 0, 0), (7, 0))
    low = [int(x) & 255 for x in (w[0][0], w[1][0], w[2][0])]
    assert float(a["r4"][0]) == ((low[0] << 16) | (low[1] << 8) | low[2]) / 2 ** 24
    assert float(a["rt"][0]) == (int(L.philox4x32_10((key, smp, 0, 2), (7, 0))[0][0]) >> 8) / 2 ** 24
    assert not np.array_equal(L.draws(key, smp, 8, PHILOX, L.PERSP)["r0"], a["r0"])


def test_self_checks_and_the_cases_are_what_their_names_say():
    print(L.self_checks())
    assert abi.parse_scene(L.case("wall24-pinhole").blob)["header"].n_prims == 24
    assert abi.parse_scene(L.case("wall300-lens").blob)["header"].n_prims == 300
    assert L.case("wall24-lens").cam[21] == np.float32(0.6) and L.case("wall24-pinhole").cam[21] == 0.0
    assert L.case("sky-perspective-v").cam[21] == 0.5 and L.case("sky-pinhole-v").cam[21] == 0.0
    assert np.array_equal(L.case("sky-perspective-u").cam[:12], L.case("sky-pinhole-u").cam[:12])  # the same camera without the lens
    hot = [n for n in L.CASES if L.lens_free_reference_camera(n)]
    assert hot == ["sky-pinhole-v", "sky-pinhole-w", "sky-pinhole-u", "wall24-pinhole", "wall300-pinhole"]
    for name in L.CASES:
        c = L.case(name)
        if c.kind != "wall":
            assert (c.cam[22], c.cam[23]) == L.SHUTTER and abi.parse_scene(c.blob)["header"].sky_light == 1
    keys = L.FRAMES["corner"].keys()
    assert int(keys.max()) == 7680 * 4320 - 1 and int(keys.max()) > 2 ** 24  # x and the key are beyond float32's integers only for the key
    assert int(L.FRAMES["shifted"].keys().min()) >= L.S.KEY_SHIFT > int(L.FRAMES["shifted"].keys().min()) - 24
    assert [int(r) for r in L.FRAMES["stride"].rows()] == [5, 7, 9, 11]


# ---------------------------------------------------------------- the oracle against the law
def all_runs():
    return [pytest.param(name, rng, draw, id=f"{name}-rng{rng}-draw{draw}") for name in L.CASES for rng in L.RNGS for draw in range(2)]


def oracle_render(name, rng):
    return lambda frame, sample, seed: L.oracle_frame(name, frame, sample, seed, rng)


@pytest.mark.parametrize("name,rng,draw", all_runs())
def test_oracle_matches_float64_reference(name, rng, draw):
    print(L.check_run(name, rng, draw, oracle_render(name, rng)))


@pytest.mark.parametrize("rng,seed", [(PHILOX, L.SEEDS[0]), (PHILOX, L.SEEDS[1]), (TEA_LCG, L.SEEDS[0])])
@pytest.mark.parametrize("name", L.MEAN_CASES)
def test_oracle_mean_of_144_samples(name, rng, seed):
    print(L.check_mean(name, seed, rng, L.oracle_frame(name, L.FULL, 0, seed, rng, L.MEAN_SPP)))


# ---------------------------------------------------------------- negative controls: the law with one thing changed must fail
def rejected(name, rng, frames=None, **wrong):
    """The right law passes on the oracle's samples of the generator's first draw; the law with `wrong` does not."""
    L.check_run(name, rng, 0, oracle_render(name, rng), frames=frames)
    with pytest.raises(AssertionError) as e:
        L.check_run(name, rng, 0, oracle_render(name, rng), frames=frames, **wrong)
    print(f"{name}, generator {rng}, with {wrong}: rejected, {str(e.value)[:200]}")


BOTH = pytest.mark.parametrize("rng", L.RNGS)


@BOTH
@pytest.mark.parametrize("name", ["sky-perspective-v", "sky-environment-u", "wall300-pinhole", "wall24-orthographic"])
def test_control_jitter_x_and_y_swapped_is_rejected(name, rng):
    rejected(name, rng, swap_jitter=True)


@BOTH
@pytest.mark.parametrize("name", ["sky-perspective-v", "sky-environment-v", "wall300-pinhole", "wall300-orthographic"])
def test_control_rows_counted_from_the_top_is_rejected(name, rng):
    rejected(name, rng, rows_from_top=True)


@BOTH
@pytest.mark.parametrize("name", ["sky-environment-v", "wall300-pinhole"])
def test_control_shard_local_rows_is_rejected(name, rng):
    """Only a shard that does not begin at row 0 can tell: the full frame is left out of this control by design."""
    rejected(name, rng, frames=("stride", "shard"), shard_local_rows=True)


def test_control_lens_draws_taken_by_the_environment_camera_is_rejected():
    """TEA+LCG only: two more draws move the gather draw and with it the ray time. The jitter comes first and does not move, so only
    the shutter cases can tell; under Philox the draws are positional and the control is the law, by design."""
    rejected("shutter-environment", TEA_LCG, lens_draws_for_all=True)
    rejected("shutter-orthographic", TEA_LCG, lens_draws_for_all=True)
    L.check_run("shutter-environment", PHILOX, 0, oracle_render("shutter-environment", PHILOX), lens_draws_for_all=True)


@BOTH
@pytest.mark.parametrize("name", ["sky-perspective-v", "sky-perspective-u", "wall300-lens"])
def test_control_lens_sine_and_cosine_swapped_is_rejected(name, rng):
    rejected(name, rng, lens_sin_cos_swapped=True)


@BOTH
def test_control_plus_cosine_in_the_environment_camera_is_rejected(rng):
    rejected("sky-environment-v", rng, plus_cos=True)
    rejected("wall300-environment", rng, plus_cos=True)


@BOTH
@pytest.mark.parametrize("name", ["wall24-orthographic", "wall300-orthographic", "shutter-orthographic"])
def test_control_orthographic_origin_entering_once_is_rejected(name, rng):
    rejected(name, rng, ortho_origin_once=True)


@pytest.mark.parametrize("name", ["shutter-perspective", "shutter-environment", "shutter-orthographic"])
def test_control_ray_and_gather_time_swapped_is_rejected(name):
    """Philox only. Under TEA+LCG both times come from one LCG output, so the swap is the law - by design: what can fail there is
    the law that gives the ray time a draw of its own (the next test)."""
    rejected(name, PHILOX, times_swapped=True)
    L.check_run(name, TEA_LCG, 0, oracle_render(name, TEA_LCG), times_swapped=True)


@pytest.mark.parametrize("name", ["shutter-perspective", "shutter-environment", "shutter-orthographic"])
def test_control_tea_lcg_ray_time_with_a_draw_of_its_own_is_rejected(name):
    rejected(name, TEA_LCG, ray_time_own_draw=True)


@BOTH
@pytest.mark.parametrize("name", ["shutter-perspective", "shutter-environment", "shutter-orthographic"])
def test_control_ray_time_spread_over_the_shutter_is_rejected(name, rng):
    rejected(name, rng, ray_time_over_shutter=True)


@BOTH
@pytest.mark.parametrize("name", ["shutter-perspective", "shutter-environment", "shutter-orthographic"])
def test_control_gather_time_raw_is_rejected(name, rng):
    rejected(name, rng, gather_raw=True)


@BOTH
@pytest.mark.parametrize("name", ["sky-pinhole-v", "sky-pinhole-u", "sky-environment-v"])
def test_control_mean_with_one_ray_handed_out_a_sample_late_is_rejected(name, rng):
    """One sample of 144 replaced by another moves a mean by about 1 / 144 of the jitter's reach: far beyond the tolerance."""
    img = L.oracle_frame(name, L.FULL, 0, L.SEEDS[0], rng, L.MEAN_SPP)
    L.check_mean(name, L.SEEDS[0], rng, img)
    with pytest.raises(AssertionError) as e:
        L.check_mean(name, L.SEEDS[0], rng, img, one_sample_late=True)
    print(f"{name}, generator {rng}: rejected, {str(e.value)[:200]}")


# ---------------------------------------------------------------- the constants
def test_measured_constants_hold_and_the_law_alone_stays_inside_the_cap():
    dirs, depth, left = L.measure_constants()
    build = L.measure_builder_constant()
    print(dirs, depth, build, {k: round(100 * v, 2) for k, v in left.items()})
    for kind, got in dirs.items():
        measured_band(got, L.MEASURED_CONSTANT_DIR[kind], f"MEASURED_CONSTANT_DIR[{kind!r}]")
    measured_band(depth, L.MEASURED_CONSTANT_DEPTH, "MEASURED_CONSTANT_DEPTH")
    measured_band(build, L.MEASURED_CONSTANT_BUILD, "MEASURED_CONSTANT_BUILD")
    assert max(left.values()) <= L.MAX_LEFT_OUT, left
    assert abs(L.sum_units(L.MEAN_SPP) - 14.3264) < 1e-4


# ---------------------------------------------------------------- the builders against the float64 ioCamera law
K_BUILD = L.K_FACTOR * L.MEASURED_CONSTANT_BUILD


def cam24(view_or_array):
    if isinstance(view_or_array, abi.View):
        return np.frombuffer(bytes(view_or_array.camera), np.float32).copy()
    return np.asarray(view_or_array, np.float32)


def held(got, law, what, at_size=0.0):
    err = L.builder_error(cam24(got), law, at_size)
    print(f"{what}: off by {err:.3f} units (K = {K_BUILD:.3f})")
    assert err <= K_BUILD, what


def test_look_at_is_the_perspective_builder():
    for name in ("look_at", "look_at_cornell"):
        fn, args = L.BUILDER_INPUTS[name]
        held(bake.look_at(*args), fn(*args), name)


def test_cube_views_are_six_perspective_builders():
    pos = (3.0, -2.0, 5.0)
    for v, (d, up) in zip(bake.cube_views(pos), bake.CUBE_FACES):
        held(v, L.io_perspective(pos, tuple(p + q for p, q in zip(pos, d)), up, 90.0, 1.0), f"cube face {d}")
        assert v.camera_type == L.PERSP


def test_view_refs_cameras_are_the_environment_and_orthographic_builders():
    fn, args = L.BUILDER_INPUTS["environment"]
    held(V.environment_camera(*args), fn(*args), "environment")
    fn, args = L.BUILDER_INPUTS["orthographic"]
    held(V.orthographic_camera(*args), fn(*args), "orthographic")


@pytest.mark.parametrize("kind", [L.PERSP, L.ENV, L.ORTHO])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_the_host_descriptions_header_cameras(k, kind):
    h = abi.parse_scene(abi.build_scene(100 * kind + k, 200, 100))["header"]
    assert h.camera_type == kind
    held(np.frombuffer(bytes(h.camera), np.float32), L.scene_camera(k, kind), f"scene {100 * kind + k}", L.at_size(k, kind))
