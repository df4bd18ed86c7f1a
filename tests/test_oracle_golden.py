"""CPU suite: the oracle against the committed golden fixtures, closed-form intersections and the
size-independent properties the path offers (tile independence, sample-range additivity)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from raytracing_weekend_amd import abi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(f[:-4] for f in os.listdir(GOLD) if f.endswith(".npz"))


def load_case(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    scene, w, h, spp, depth, rng, seed = (int(v) for v in z["meta"])
    p = abi.make_params(w, h, spp, depth, seed=seed, rng_kind=rng)
    return z["blob"].tobytes(), p, z["rgb"], tuple(int(v) for v in z["stats"])


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_golden_bit_for_bit(name):
    blob, p, rgb, stats = load_case(name)
    img, st = oracle.render(blob, p, threads=8)
    assert np.array_equal(img[..., :3], rgb)
    assert (st.samples, st.segments, st.shadow_rays) == stats
    assert np.all(img[..., 3] == 1.0) and np.isfinite(img).all()


def test_whole_frame_hashes_are_the_oracle_s():
    """tests/golden/metric_frames.json (whole BASELINE frames at their sample counts, hashed: what the GPU suite compares its
    renders with) was written by this oracle: its smallest entry, BASELINE config 1, is re-rendered here and hashed the same
    way; the large ones take a 64-thread host minutes each (tests/golden/make_metric_frame_hashes.py)."""
    import hashlib
    import json
    g = json.load(open(os.path.join(GOLD, "metric_frames.json")))
    assert {"c1", "c2", "c4", "headline"} <= set(g)
    for name, e in g.items():  # every entry was compared band by band with the GPU image when it was made
        assert e["gpu_mismatching_pixels"] == 0 and e["gpu_counts_equal"] and e["gpu_sha256"] == e["sha256"], name
        assert e["samples"] == e["width"] * e["height"] * e["spp"]
    # ... and the entries named after bench.py's configurations are those workloads (same scene, frame, samples, depth, seed)
    import importlib.util
    spec = importlib.util.spec_from_file_location("rtw_bench", os.path.join(abi.REPO_DIR, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name in ("headline", "c2", "c4"):
        c, e = bench.CONFIGS[name], g[name]
        assert (c["scene"], c["w"], c["h"], c["spp"], bench.DEPTH, bench.SEED) == (e["scene"], e["width"], e["height"], e["spp"], e["max_depth"], e["seed"])
    e = g["c1"]
    img, st = oracle.render(abi.build_scene(e["scene"], e["width"], e["height"]),
                            abi.make_params(e["width"], e["height"], e["spp"], e["max_depth"], seed=e["seed"]), threads=8)
    assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == e["sha256"]
    assert (st.samples, st.segments, st.shadow_rays) == (e["samples"], e["segments"], e["shadow_rays"])


def test_thread_count_does_not_change_the_image():
    blob, p, rgb, _ = load_case("cornell_200x200_16spp_d4_philox")
    p.row0, p.row1 = 90, 110
    a, _ = oracle.render(blob, p, threads=1)
    b, _ = oracle.render(blob, p, threads=5)
    assert np.array_equal(a, b) and np.array_equal(a[..., :3], rgb[90:110])


@pytest.mark.parametrize("rng", [0, 1])
def test_row_tiles_are_independent_of_the_partition(rng):
    blob = abi.build_scene(0, 64, 48)
    full, _ = oracle.render(blob, abi.make_params(64, 48, 4, 6, rng_kind=rng), threads=4)
    parts = []
    for r0, r1 in ((0, 7), (7, 7), (7, 30), (30, 48)):  # includes an empty tile
        img, st = oracle.render(blob, abi.make_params(64, 48, 4, 6, rng_kind=rng, row0=r0, row1=r1), threads=2)
        assert st.samples == (r1 - r0) * 64 * 4
        parts.append(img)
    assert np.array_equal(np.concatenate(parts, axis=0), full)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_interleaved_row_shards_reassemble_the_frame(world):
    blob = abi.build_scene(0, 40, 27)
    full, st_full = oracle.render(blob, abi.make_params(40, 27, 3, 5), threads=4)
    out = np.empty_like(full)
    seg = 0
    for g in range(world):
        p = abi.make_params(40, 27, 3, 5, row0=g, row1=27, row_stride=world)
        img, st = oracle.render(blob, p, threads=2)
        assert img.shape[0] == abi.local_rows(p) == len(range(g, 27, world))
        out[g::world] = img
        seg += st.segments
    assert np.array_equal(out, full) and seg == st_full.segments


def test_sample_offset_selects_the_same_streams():
    blob = abi.build_scene(0, 32, 32)
    whole, _ = oracle.render(blob, abi.make_params(32, 32, 8, 5), threads=4)
    a, _ = oracle.render(blob, abi.make_params(32, 32, 4, 5, sample_offset=0), threads=4)
    b, _ = oracle.render(blob, abi.make_params(32, 32, 4, 5, sample_offset=4), threads=4)
    assert np.allclose((a.astype(np.float64) + b) / 2, whole, rtol=0, atol=2e-6 * max(1.0, float(whole.max())))
    assert not np.array_equal(a, b)


def test_seed_changes_philox_but_reference_generator_ignores_it():
    blob = abi.build_scene(0, 32, 32)
    a, _ = oracle.render(blob, abi.make_params(32, 32, 2, 4, seed=1), threads=2)
    b, _ = oracle.render(blob, abi.make_params(32, 32, 2, 4, seed=2), threads=2)
    assert not np.array_equal(a, b)
    c, _ = oracle.render(blob, abi.make_params(32, 32, 2, 4, seed=1, rng_kind=1), threads=2)
    d, _ = oracle.render(blob, abi.make_params(32, 32, 2, 4, seed=2, rng_kind=1), threads=2)
    assert np.array_equal(c, d)  # tea<64>(pixel, sample): raygen.cu:129 has no user seed


def test_max_depth_zero_and_one():
    blob = abi.build_scene(0, 16, 16)
    img0, st0 = oracle.render(blob, abi.make_params(16, 16, 2, 0))
    assert st0.segments == 0 and np.all(img0[..., :3] == 0)
    img1, st1 = oracle.render(blob, abi.make_params(16, 16, 2, 1))
    assert st1.segments == st1.samples == 16 * 16 * 2


def test_invalid_inputs_are_rejected():
    lib = oracle.load()
    blob = abi.build_scene(0, 16, 16)
    out = np.zeros((16, 16, 4), np.float32)
    st = abi.Stats()
    bad = abi.make_params(16, 16, 1, 1, row0=5, row1=3)
    assert lib.rtwo_render(blob, len(blob), C.byref(bad), out.ctypes.data, C.byref(st), 1) == -1
    ok = abi.make_params(16, 16, 1, 1)
    assert lib.rtwo_render(blob[:40], 40, C.byref(ok), out.ctypes.data, C.byref(st), 1) == -2
    corrupt = bytearray(blob)
    corrupt[0] ^= 0xFF
    assert lib.rtwo_render(bytes(corrupt), len(corrupt), C.byref(ok), out.ctypes.data, C.byref(st), 1) == -2


# ---------------------------------------------------------------- closed-form intersections
def one_prim_scene(prim):
    """A blob with a single primitive, identity transform, one lambertian material."""
    hdr = abi.SceneHeader()
    hdr.magic, hdr.version = abi.RTW_SCENE_MAGIC, abi.RTW_SCENE_VERSION
    hdr.n_prims = hdr.n_xforms = hdr.n_materials = hdr.n_textures = 1
    sizes = [C.sizeof(abi.SceneHeader), 64, 96, 16, 32]
    offs = [0]
    for s_ in sizes:
        offs.append((offs[-1] + s_ + 15) // 16 * 16)
    hdr.off_prims, hdr.off_xforms, hdr.off_materials, hdr.off_textures, hdr.off_lights = offs[1], offs[2], offs[3], offs[4], offs[5]
    hdr.total_bytes = offs[5]
    hdr.sky_light = 1
    xf = abi.Xform()
    for i in (0, 5, 10):
        xf.m[i] = xf.inv[i] = 1.0
    mat = abi.Material(type=abi.MAT_LAMBERTIAN, texture=0, fuzz_or_eta=0.0, bsdf_eval=0)
    tex = abi.Texture(type=1)
    buf = bytearray(offs[5])
    for off, obj in ((0, hdr), (offs[1], prim), (offs[2], xf), (offs[3], mat), (offs[4], tex)):
        buf[off:off + C.sizeof(obj)] = bytes(obj)
    return bytes(buf)


def test_sphere_roots_closed_form():
    pr = abi.Prim(type=abi.PRIM_SPHERE)
    pr.p[0], pr.p[1], pr.p[2], pr.p[3] = 0.0, 0.0, 5.0, 2.0
    blob = one_prim_scene(pr)
    rays = np.array([[0, 0, 0, 0, 0, 1, 1e-6, 1e27],      # hits at t=3
                     [0, 0, 0, 0, 0, 2, 1e-6, 1e27],      # unnormalised direction: t=1.5 (sphere.cu:52-60)
                     [0, 0, 5, 0, 0, 1, 1e-6, 1e27],      # from the centre: far root t=2
                     [0, 3, 0, 0, 0, 1, 1e-6, 1e27],      # misses
                     [0, 0, 0, 0, 0, 1, 1e-6, 2.5],       # tmax before the sphere
                     [0, 0, 0, 0, 0, -1, 1e-6, 1e27]],    # behind
                    dtype=np.float32)
    t, prim = oracle.intersect(blob, rays)
    assert list(prim) == [0, 0, 0, -1, -1, -1]
    assert t[0] == 3.0 and t[1] == 1.5 and t[2] == 2.0 and t[4] == np.float32(2.5)


def test_rect_bounds_are_inclusive_and_tmin_applies():
    pr = abi.Prim(type=abi.PRIM_RECT_Y)
    for i, v in enumerate((0.0, 10.0, 0.0, 10.0, 4.0)):
        pr.p[i] = v
    blob = one_prim_scene(pr)
    rays = np.array([[5, 0, 5, 0, 1, 0, 1e-6, 1e27],      # centre, t=4
                     [10, 0, 10, 0, 2, 0, 1e-6, 1e27],    # corner exactly on a1,b1: inclusive (aarecty.cu:19-20), t=2
                     [10.001, 0, 5, 0, 1, 0, 1e-6, 1e27],  # just outside
                     [5, 4, 5, 0, 1, 0, 1e-6, 1e27],      # origin on the plane: t=0 < tmin
                     [5, 0, 5, 1, 0, 0, 1e-6, 1e27]],     # parallel
                    dtype=np.float32)
    t, prim = oracle.intersect(blob, rays)
    assert list(prim) == [0, 0, -1, -1, -1]
    assert t[0] == 4.0 and t[1] == 2.0


def test_schlick_reflection_share_of_the_oracle():
    """dielectricMaterial.cu:20-26: the share of samples the oracle reflects at glass of eta 1.5, read through the sky
    (tests/shading_ref.py), against r0 + (1 - r0) (1 - cos)^5 with r0 = ((1 - 1.5) / (1 + 1.5))^2 = 0.04 - at one incidence with
    16384 samples, and pooled over the incidences of either face (binomial limit at alpha = 1e-4)."""
    import shading_ref as S
    assert np.isclose(S.dielectric(np.array([[0.0, -1.0, 0.0]]), (0.0, 1.0, 0.0), 1.5)["p"][0], 0.04)
    for name in ("direction-glass_share", "direction-glass_above", "direction-glass_below"):
        for rng in S.RNGS:
            print(S.check(name, S.oracle_samples(name, rng, S.REF, S.SEEDS[0]), S.REF))


# ---------------------------------------------------------------- texture callables
def test_spec_sin_atan2_asin_accuracy():
    """The Cephes restatements the textures use stay within a few ulp of libm over the ranges the scenes produce."""
    lib = oracle.load()
    for f in ("rtwo_sinf", "rtwo_asinf"):
        getattr(lib, f).restype = C.c_float
        getattr(lib, f).argtypes = [C.c_float]
    lib.rtwo_atan2f.restype = C.c_float
    lib.rtwo_atan2f.argtypes = [C.c_float, C.c_float]
    rs = np.random.RandomState(0)
    xs = np.concatenate([rs.uniform(-6000, 6000, 4000), rs.uniform(-8, 8, 4000), [0.0, np.pi, -np.pi / 2]]).astype(np.float32)
    assert max(abs(lib.rtwo_sinf(float(x)) - np.sin(np.float64(x))) for x in xs) < 2e-7
    xs = np.concatenate([rs.uniform(-1, 1, 4000), [1.0, -1.0, 0.0, 0.5, 1.0000001, -1.5]]).astype(np.float32)
    assert max(abs(lib.rtwo_asinf(float(x)) - np.arcsin(np.clip(np.float64(x), -1, 1))) for x in xs) < 4e-7
    ys, xs = rs.uniform(-5, 5, 4000).astype(np.float32), rs.uniform(-5, 5, 4000).astype(np.float32)
    assert max(abs(lib.rtwo_atan2f(float(y), float(x)) - np.arctan2(np.float64(y), np.float64(x))) for x, y in zip(xs, ys)) < 6e-7
    assert lib.rtwo_atan2f(0.0, -1.0) == np.float32(np.pi) and lib.rtwo_atan2f(1.0, 0.0) == np.float32(np.pi / 2) and lib.rtwo_atan2f(0.0, 0.0) == 0.0


def test_textured_scene_on_the_oracle():
    """Checker / noise / image textures: finite image, textures visibly in effect, broken texture tables rejected."""
    w, h = 48, 40
    blob = oracle.textured_cornell(w, h)
    p = abi.make_params(w, h, 3, 10)
    img, st = oracle.render(blob, p, threads=4)
    assert np.isfinite(img).all() and st.segments > 0
    plain, _ = oracle.render(abi.build_scene(0, w, h), p, threads=4)
    assert not np.array_equal(img, plain)
    lib = oracle.load()
    out = np.zeros((h, w, 4), np.float32)
    st2 = abi.Stats()
    parts = dict(abi.parse_scene(blob))
    texs = list(parts["textures"])
    noise = [i for i, t in enumerate(texs) if t.type == abi.TEX_NOISE][0]
    bad = abi.Texture.from_buffer_copy(bytes(texs[noise]))
    bad.data = len(parts["texdata"]) // 4 - 10  # tables would run past the section
    texs[noise] = bad
    parts["textures"] = texs
    broken = abi.assemble_scene(parts)
    assert lib.rtwo_render(broken, len(broken), C.byref(p), out.ctypes.data, C.byref(st2), 1) == -2
    texs[noise] = abi.Texture(type=9)
    broken = abi.assemble_scene(parts)
    assert lib.rtwo_render(broken, len(broken), C.byref(p), out.ctypes.data, C.byref(st2), 1) == -2


def test_corrupted_scenes_are_rejected_by_the_oracle():
    lib = oracle.load()
    p = abi.make_params(24, 16, 1, 2)
    out = np.zeros((16, 24, 4), np.float32)
    st = abi.Stats()
    ok = oracle.textured_cornell(24, 16)
    assert lib.rtwo_render(ok, len(ok), C.byref(p), out.ctypes.data, C.byref(st), 1) == 0
    for name, blob in oracle.corrupted_scenes():
        assert lib.rtwo_render(blob, len(blob), C.byref(p), out.ctypes.data, C.byref(st), 1) == -2, name


def test_corrected_estimators_on_the_oracle():
    """SURVEY 8f rank 2 on the CPU: the modes differ from the reference mode and from each other at low sample counts,
    agree in the mean at moderate ones, bad estimator ids are refused, and the default (0) is the fixture mode."""
    w, h = 24, 24
    blob = abi.build_scene(0, w, h)
    imgs = {}
    for est, spp in ((0, 256), (1, 256), (2, 4096)):
        img, st = oracle.render(blob, abi.make_params(w, h, spp, 50, estimator=est), threads=8)
        assert np.isfinite(img).all()
        assert (st.shadow_rays > 0) == (est != 2)
        imgs[est] = img[..., :3].astype(np.float64)
    m = {k: v.mean() for k, v in imgs.items()}
    assert abs(m[1] - m[2]) / m[2] < 0.03, m          # two estimators, one integrand
    assert abs(m[0] - m[2]) / m[2] > 0.05, m          # the reference's quirks are visible in the mean
    lib = oracle.load()
    out = np.zeros((h, w, 4), np.float32)
    st = abi.Stats()
    for bad in (-1, 4):
        p = abi.make_params(w, h, 1, 2, estimator=bad)
        assert lib.rtwo_render(blob, len(blob), C.byref(p), out.ctypes.data, C.byref(st), 1) == -1


def test_denoise_stand_in_on_the_oracle():
    """The a-trous filter (rtw_denoise / rtwo_denoise): constants pass through, noise shrinks, edges survive."""
    rs = np.random.RandomState(3)
    flat = np.full((20, 24, 4), 0.25, np.float32)
    assert np.array_equal(oracle.denoise(flat, 3, 0.5), flat)
    clean = np.zeros((48, 64, 4), np.float32)
    clean[:, :32, :3] = 0.2
    clean[:, 32:, :3] = 0.9
    clean[..., 3] = 1.0
    noisy = clean.copy()
    noisy[..., :3] += rs.normal(0, 0.05, (48, 64, 3)).astype(np.float32)
    den = oracle.denoise(noisy, 5, 0.3)
    err = lambda a: float(np.sqrt(np.mean((a[..., :3] - clean[..., :3]) ** 2)))
    assert err(den) < 0.35 * err(noisy)
    assert abs(den[24, 28, 0] - 0.2) < 0.03 and abs(den[24, 36, 0] - 0.9) < 0.03   # the edge is kept
    assert np.array_equal(den[..., 3], noisy[..., 3])
    import ctypes as C2
    lib = oracle.load()
    lib.rtwo_denoise.restype = C2.c_int
    lib.rtwo_denoise.argtypes = [C2.c_void_p, C2.c_void_p, C2.c_int, C2.c_int, C2.c_int, C2.c_float]
    out = np.empty_like(noisy)
    assert lib.rtwo_denoise(noisy.ctypes.data, out.ctypes.data, 64, 48, 0, 0.3) == -1
    assert lib.rtwo_denoise(noisy.ctypes.data, out.ctypes.data, 64, 48, 3, 0.0) == -1
    assert lib.rtwo_denoise(noisy.ctypes.data, noisy.ctypes.data, 64, 48, 3, 0.3) == -1
