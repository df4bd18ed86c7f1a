"""The reference's own device programs as a referee: what tests/test_ref_programs_cpu.py and tests/test_gpu_ref_programs.py share.
oracle/ref_programs_wrap.cpp compiles the reference's .cu files, unmodified, behind stand-in headers and a host emulation of the OptiX
device API; `make -C oracle ref` builds it twice, oracle/_ref/libref_programs.so (no contraction) and libref_programs_fma.so
(contraction on). tests/golden/make_ref_programs.py records what both builds compute in tests/golden/ref_programs/*.npz; the tests read
those fixtures - in a directory of their own, since every .npz directly under tests/golden is a golden render to the parity
tests - (and the live libraries only to hold the fixtures to them), never the reference tree. A plain module on the
law_common / gpu_common scaffolds.

Level A, one program at a time: the intersection programs on geometry_ref's own rays, held to geometry_ref.closest_hit with that
file's error unit, K, conditioning mask and cap (geometry_ref.check_against), and the camera callables on raygen.cu's own (s, t, seed)
against camera_ref.camera_rays (check_camera), and the noise and checker callables at the points of shading_ref's texture cases with
that file's own check (TextureCase.check), and shading_ref's mirror / glass directions and lighting_ref's depth-1 light samples through
launches of those files' own cases as one-ray cameras (LAW_CASES, law_samples), each with its file's own check: the float64 referees are
held to the text.
Level B, a launch: raygen -> traverse -> intersection -> closest hit -> material / texture / pdf -> miss, one sample per pixel seeded
tea<64>(width * y + x, 0): this project's sample 0 under RTW_RNG_TEA_LCG and RTW_EST_REFERENCE. The reference's frame is the square
root of the sample (raygen.cu:151-155), so the oracle's and the kernels' radiance is square-rooted before the comparison.

Tolerance of level B. MEASURED_CONSTANT_SAMPLE is the largest relative difference per channel, |a - b| / max(|a|, |b|), between the
two builds of the reference over the samples of all level B cases whose per-pixel traversal counts agree between the builds - the
reference against itself under another, equally valid, fp32 evaluation. At depth 1 the counts cannot tell a decision taken otherwise
(every sample is one traversal, and a shadow probe is counted whether it is occluded or not), and over the cases used the differences
are bimodal: at most 6.0e-4 (cluttered_cornell; 1.1e-4 and less in the other cases), or 0.6 to 1 (one build's probe occluded). A
sample whose builds differ by more than DECISION = 1e-2 counts as a disagreement of the builds, like one whose counts differ, and not
towards the constant. DECISION is this file's addition to the rule - without it the constant would be 1 -, a hand-chosen value
between the two modes; test_ref_programs_cpu.py asserts that no sample of any case lies between TOLERANCE and DECISION, so the
constant does not depend on where in that gap it is put. TOLERANCE = K_FACTOR * MEASURED_CONSTANT_SAMPLE with the
project's K_FACTOR = 4 (law_common.K_FACTOR): the oracle has its own sincos, log and written-out fmaf. Cap: at most CAP = 1 % of a
case's samples may lie outside (each is printed with its pixel), and the summed radiance and shadow traversals agree with the
oracle's segments / shadow_rays within that share. Condition on the cases: the two builds disagree with each other (traversal
counts, or a channel beyond TOLERANCE) on at most BUILDS_CAP = 0.25 % of a case's samples.

Finding (DESIGN.md "Pinning"): that condition decides the depth. The reference restarts a scattered ray 1e-6 from a hit point that is
accurate to about 2e-5 in the 555-unit box (include/rtw.h, rtw_estimator), so whether a ray re-hits the surface it leaves hangs
on the last bits of the hit point; a contracted multiply-add in `origin + t * direction` decides it otherwise. The two builds of the
reference's own text disagree on 11.9 % of scene 0's samples at depth 2, 20 % at depth 3 and 26.7 % at depth 50 (64 x 64; fog scene:
3.5 %, 8.3 %, 11.0 %), and the oracle disagrees with either build by the same shares (12.9 %, 23.2 %, 30.5 %) - the reference
is no referee of itself beyond the first segment, on any scene with a surface to leave. Every level B case therefore runs at depth 1:
camera ray, traversal, intersection, closest hit, material, texture, light sample, shadow probe, miss. The deeper loop (depth cut,
roulette, throughput) stays with path_ref.py. Per-case shares at depth 1 (builds / oracle outside TOLERANCE), as
`python tests/golden/make_ref_programs.py` prints them, are in SHARES below.
"""
import ctypes as C
import functools
import os

import numpy as np

import law_common
from raytracing_weekend_amd import abi

REF_DIR = os.path.join(abi.REPO_DIR, "oracle", "_ref")
BUILDS = {"plain": os.path.join(REF_DIR, "libref_programs.so"), "fma": os.path.join(REF_DIR, "libref_programs_fma.so")}
GOLD = os.path.join(abi.REPO_DIR, "tests", "golden")
SIDE = 64
K_FACTOR = law_common.K_FACTOR
MEASURED_CONSTANT_SAMPLE = 5.9908e-4  # make_ref_programs.py: cluttered_cornell (cornell, checkered_cornell: 1.04e-4; the others below 6e-6)
TOLERANCE = K_FACTOR * MEASURED_CONSTANT_SAMPLE
DECISION = 1e-2  # a relative difference beyond this is another decision (a probe occluded or not, a checker's other colour), no rounding
CAP = 0.01
BUILDS_CAP = 0.0025
N_RAYS = 2000  # level A: geometry_ref's rays per scene


def have_live():
    return all(os.path.exists(p) for p in BUILDS.values())


@functools.lru_cache(maxsize=None)
def load(build):
    lib = C.CDLL(BUILDS[build])
    lib.ref_launch.restype = C.c_int
    lib.ref_launch.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.ref_launch_rows.restype = C.c_int
    lib.ref_launch_rows.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ref_intersect.restype = C.c_int
    lib.ref_intersect.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ref_texture.restype = C.c_int
    lib.ref_texture.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ref_camera.restype = C.c_int
    lib.ref_camera.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def launch(build, blob, width, height, depth):
    """One launch of the reference's programs: (frame (h, w, 4) float32, counts (h, w, 3) uint32: radiance traversals, shadow
    traversals, rnd calls of each pixel)."""
    frame, counts = np.zeros((height, width, 4), np.float32), np.zeros((height, width, 3), np.uint32)
    rc = load(build).ref_launch(blob, len(blob), width, height, depth, frame.ctypes.data, counts.ctypes.data)
    if rc:
        raise RuntimeError(f"ref_launch: {rc}")
    return frame, counts


def render(build):
    """`render(blob, params) -> (image, stats)` as law_common.observe takes it, by a launch of the reference's programs: the rows
    [row0, row1) of sample 0 under TEA+LCG, the LINEAR sample (what raygen.cu hands to its sqrtf), alpha 1; stats carries the
    summed radiance traversals as segments and the shadow traversals as shadow_rays."""
    def run(blob, p):
        assert (p.spp, p.sample_offset, p.rng_kind, p.estimator) == (1, 0, abi.RTW_RNG_TEA_LCG, abi.RTW_EST_REFERENCE) and p.row_stride <= 1
        rows = p.row1 - p.row0
        frame, linear = np.zeros((rows, p.width, 4), np.float32), np.zeros((rows, p.width, 3), np.float32)
        counts = np.zeros((rows, p.width, 3), np.uint32)
        rc = load(build).ref_launch_rows(blob, len(blob), p.width, p.height, p.row0, p.row1, p.max_depth, frame.ctypes.data, linear.ctypes.data,
                                         counts.ctypes.data)
        if rc:
            raise RuntimeError(f"ref_launch_rows: {rc}")
        assert np.array_equal(np.sqrt(linear), frame[..., :3])
        st = abi.Stats(segments=int(counts[..., 0].sum()), shadow_rays=int(counts[..., 1].sum()))
        return np.concatenate([linear, frame[..., 3:]], -1), st
    return run


# Level A through the float64 laws' own cases: each case's rays as one-ray cameras (radiance_ref.ray_blob), every key one launch
# index, so that the reference's closest-hit program, its material, pdf and miss callables produce the very samples the law
# describes. module name -> case names: shading_ref's mirror and glass directions on its INCIDENCES under the reference estimator
# (the transformed ones are defined for the corrected estimator only), lighting_ref's depth-1 light samples under it.
LAW_CASES = {
    "shading_ref": ("direction-mirror_above", "direction-mirror_above_long", "direction-glass_above", "direction-glass_below",
                    "direction-glass_below_flipped"),
    "lighting_ref": ("three_lights-d1", "nonwhite_pair-d1", "behind-d1", "probe_far_end-d1", "point00-d1"),
}


def law_module(name):
    import importlib
    return importlib.import_module(name)


def law_samples(build, module, name):
    """law_common.Observed of case `name` of a law module through the reference's programs: the first draw of TEA+LCG (keys from 0)."""
    c = law_module(module).case(name)
    assert law_common.REF in c.estimators
    return law_common.observe(render(build), c, abi.RTW_RNG_TEA_LCG, law_common.REF, law_common.SEEDS[0], 0)


def record_law(module, name):
    out = {}
    for build in BUILDS:
        ob = law_samples(build, module, name)
        out[f"samples_{build}"], out[f"counts_{build}"] = ob.samples, np.array([ob.segments, ob.shadow_rays], np.int64)
    return out


def law_fixture(module, name, build):
    fx = fixture("a", f"{module}_{name}")
    return law_common.Observed(fx[f"samples_{build}"], int(fx[f"counts_{build}"][0]), int(fx[f"counts_{build}"][1]))


def intersect(build, blob, rays, ray_time, gather_time):
    """The intersection programs on rays: dict t, prim, reported (accepted reports), normal, uv, point of the committed hit."""
    rays, rt, gt = (np.ascontiguousarray(a, np.float32) for a in (rays, ray_time, gather_time))
    n = len(rays)
    out, prim, rep = np.zeros((n, 11), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = load(build).ref_intersect(blob, len(blob), rays.ctypes.data, rt.ctypes.data, gt.ctypes.data, n, out.ctypes.data, prim.ctypes.data, rep.ctypes.data)
    if rc:
        raise RuntimeError(f"ref_intersect: {rc}")
    return {"t": out[:, 0].copy(), "prim": prim, "reported": rep, "normal": out[:, 1:4].copy(), "uv": out[:, 4:6].copy(), "point": out[:, 6:9].copy()}


def camera_rays(build, blob, width, height):
    """The camera callable of the blob's camera kind on the (s, t, seed) raygen.cu:129-139 hands it for every pixel of a frame:
    (origin, direction) (h * w, 3) float32 in stream-key order."""
    import camera_ref
    key = np.arange(width * height, dtype=np.uint64)
    seed = camera_ref.tea(64, key, np.zeros_like(key))
    seed, r0 = camera_ref.lcg(seed)
    seed, r1 = camera_ref.lcg(seed)
    x, y = (key % width).astype(np.float32), (key // width).astype(np.float32)
    s = ((x + r0.astype(np.float32)) / np.float32(width)).astype(np.float32)
    t = ((y + r1.astype(np.float32)) / np.float32(height)).astype(np.float32)
    seed = np.ascontiguousarray(seed, np.uint32)
    n = len(key)
    o, d, so = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    rc = load(build).ref_camera(blob, len(blob), s.ctypes.data, t.ctypes.data, seed.ctypes.data, n, o.ctypes.data, d.ctypes.data, so.ctypes.data)
    if rc:
        raise RuntimeError(f"ref_camera: {rc}")
    return o, d


# ---------------------------------------------------------------- the cases
def _without_images(blob):
    """The blob with every image texture replaced by a constant (tex2D's hardware filter is out of the referee's scope) and what
    fp32 itself cannot decide taken out."""
    parts = dict(abi.parse_scene(blob))
    texs = [abi.Texture.from_buffer_copy(bytes(t)) for t in parts["textures"]]
    for i, t in enumerate(texs):
        if t.type == abi.TEX_IMAGE:
            t.type, t.data = abi.TEX_CONSTANT, 0
            t.color[0], t.color[1], t.color[2] = 0.2 + 0.1 * (i % 5), 0.7 - 0.1 * (i % 4), 0.5
        if t.type == abi.TEX_NOISE:
            # 0.5 (1 + sin(..)) comes arbitrarily close to 0, where a relative difference means nothing: with the noise textures in,
            # the two builds differ by more than the tolerance on 2.7 % of the frame (largest difference below DECISION 3.6e-3)
            t.type, t.data = abi.TEX_CONSTANT, 0
            t.color[0], t.color[1], t.color[2] = 0.6, 0.5, 0.3 + 0.1 * (i % 4)
    # a checker's sign is sin(10 x) sin(10 - y) sin(10 z) (checkeredTexture.cu:9): on a rectangle in a coordinate plane through the
    # origin it hangs on the last bit of the hit point. Such rectangles take the first material without a checker instead.
    mats, prims = parts["materials"], [abi.Prim.from_buffer_copy(bytes(p)) for p in parts["prims"]]
    plain = [i for i, m in enumerate(mats) if m.type == abi.MAT_LAMBERTIAN and m.texture >= 0 and texs[m.texture].type == abi.TEX_CONSTANT][-1]
    for p in prims:
        if abi.PRIM_RECT_X <= p.type <= abi.PRIM_RECT_Z and p.p[4] == 0.0 and texs[mats[p.material].texture].type == abi.TEX_CHECKER:
            p.material = plain
    # a diffuse sphere or a diffuse face of a transformed box under a listed light: its probe starts 5e-5 from a hit point that is
    # 2e-5 to 1e-4 off the surface, and whether the surface shadows itself is a decision of the last bits (a quarter of such a
    # face's samples differ between the builds). The sphere is glass and the boxes are metal again, as in scene 0.
    glass = [i for i, m in enumerate(mats) if m.type == abi.MAT_DIELECTRIC][0]
    metal = [i for i, m in enumerate(mats) if m.type == abi.MAT_METAL][0]
    for p in prims:
        if p.type == abi.PRIM_SPHERE:
            p.material = glass
        elif p.xform != 0:
            p.material = metal
    parts["textures"], parts["prims"] = texs, prims
    return abi.assemble_scene(parts)


def _level_b():
    import oracle  # scene builders only (pure Python)
    w = h = SIDE
    return {
        "cornell": lambda: abi.build_scene(0, w, h),
        "cornell_environment": lambda: abi.build_scene(100, w, h),
        "cornell_orthographic": lambda: abi.build_scene(200, w, h),
        "fog": lambda: abi.build_scene(3, w, h),
        "cluttered_cornell": lambda: oracle.cluttered_cornell(w, h, n_extra=30, seed=8),
        # metal, glass, moving spheres, transforms, the sky and two lights
        "random21": lambda: oracle.random_scene(21, w, h, n_prims=40, motion=True, n_lights=2, sky=True),
        "random32": lambda: oracle.random_scene(32, w, h, n_prims=60, motion=True, n_lights=1),
        # a heavily edited scene (_without_images): oracle.textured_cornell with its noise and image textures replaced by constants, its
        # sphere glass and its transformed boxes metal again, no checker on a plane through the origin. What is left of the textures:
        # checkers of constants on the untransformed walls. Noise is held to the text in level A only (TEXTURES).
        "checkered_cornell": lambda: _without_images(oracle.textured_cornell(w, h)),
    }


LEVEL_B = _level_b()
DEPTH = 1  # the module docstring's finding: the only depth at which the reference agrees with itself
# case -> (share of samples on which the two builds disagree, share on which the oracle lies outside TOLERANCE), make_ref_programs.py
SHARES = {"cornell": (0.000000, 0.000000), "cornell_environment": (0.001221, 0.001221), "cornell_orthographic": (0.000000, 0.000000), "fog": (0.000000, 0.000000), "cluttered_cornell": (0.000977, 0.000977), "random21": (0.000000, 0.000000), "random32": (0.001221, 0.001221), "checkered_cornell": (0.000000, 0.000000)}


def _level_a():
    import geometry_ref as G
    return {k: G.SCENES[k] for k in ("scene0", "cluttered_cornell", "random19", "random16_motion")}


LEVEL_A = _level_a()


def fixture_path(level, name):
    return os.path.join(GOLD, "ref_programs", f"{level}_{name}.npz")


@functools.lru_cache(maxsize=None)
def fixture(level, name):
    z = np.load(fixture_path(level, name))
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    if "blob" in out:
        out["blob"] = out["blob"].tobytes()
    return out


def level_a_rays(blob):
    import geometry_ref as G
    rays, rt, gt = G.scene_rays(blob, G.RAY_SEED, N_RAYS)
    return rays, rt, gt


def record_level_b(name):
    """What the fixture of a level B case holds, from the live libraries."""
    blob = LEVEL_B[name]()
    out = {"blob": np.frombuffer(blob, np.uint8), "meta": np.array([SIDE, SIDE, DEPTH], np.int32)}
    for build in BUILDS:
        frame, counts = launch(build, blob, SIDE, SIDE, DEPTH)
        assert counts.max() < 65536 and np.all(frame[..., 3] == 1.0)
        out[f"frame_{build}"], out[f"counts_{build}"] = frame[..., :3].copy(), counts.astype(np.uint16)
    o, d = camera_rays("plain", blob, SIDE, SIDE)
    out["camera_origin"], out["camera_direction"] = o, d
    return out


TEXTURES = ("noise_scale4_near", "noise_scale005_far", "noise_scale4_far", "checker_constants")  # shading_ref's cases without an image


def texture_values(build, blob, tex, points):
    """The texture callable of texture `tex` of the blob at points (n, 3) (u = v = 0: neither noise nor a checker of constants reads them)."""
    p = np.ascontiguousarray(points, np.float32)
    assert np.array_equal(p.astype(np.float64), points), "a point is not exact in float32"
    uv, rgb = np.zeros((len(p), 2), np.float32), np.zeros((len(p), 3), np.float32)
    rc = load(build).ref_texture(blob, len(blob), tex, uv.ctypes.data, p.ctypes.data, len(p), rgb.ctypes.data)
    if rc:
        raise RuntimeError(f"ref_texture: {rc}")
    return rgb


def record_textures():
    """Level A, textures: the noise and checker callables at the points of shading_ref's own texture cases (texture 0 of each)."""
    import shading_ref
    out = {}
    for name in TEXTURES:
        c = shading_ref.case("texture-" + name)
        out[f"{name}_points"] = c.points
        for build in BUILDS:
            out[f"{name}_{build}"] = texture_values(build, c.blob, 0, c.points)
    return out


LENS_RADIUS = 25.0  # level A's camera with a lens: scene 0's perspective camera with this aperture radius


def lens_blob():
    """Scene 0 with a lens on its perspective camera (the reference never sets one: include/rtw.h, rtw_camera.lens_radius)."""
    import camera_ref
    blob = abi.build_scene(0, SIDE, SIDE)
    cam, kind = camera_ref.camera_of(blob)
    cam[21] = LENS_RADIUS
    return camera_ref._with_camera(blob, cam, kind)


def record_camera_lens():
    blob = lens_blob()
    out = {"blob": np.frombuffer(blob, np.uint8), "meta": np.array([SIDE, SIDE, DEPTH], np.int32)}
    for build in BUILDS:
        out[f"camera_origin_{build}"], out[f"camera_direction_{build}"] = camera_rays(build, blob, SIDE, SIDE)
    return out


def check_camera(name, blob, origin, direction, **wrong):
    """Level A, the camera callables: the reference's (origin, direction) of every pixel of a SIDE x SIDE frame's sample 0 against
    camera_ref.camera_rays at float64 on camera_ref.draws' uniforms, within K_FACTOR times the forward error bounds e_o, e_d that
    camera_rays itself states for an fp32 evaluation (camera_ref.fp32_ray_units; units of 2^-24). camera_ref's own checks read rays
    back through rendered pictures (the sky's colour, a wall's tiles); the reference's camera callables hand out the ray itself, so this
    comparison of rays is new - its bound is not: it is the one camera_ref states for every ray it predicts. `wrong`: camera_rays' negative controls."""
    import camera_ref
    cam, kind = camera_ref.camera_of(blob)
    frame = camera_ref.Frame(SIDE, SIDE, 0, SIDE, 0)
    d = camera_ref.draws(frame.keys(), 0, 0, abi.RTW_RNG_TEA_LCG, kind)
    o64, d64, e_o, e_d = camera_ref.camera_rays(cam, kind, frame, d, **wrong)
    err_o = np.abs(origin.reshape(SIDE, SIDE, 3).astype(np.float64) - o64).max(-1)
    err_d = np.abs(direction.reshape(SIDE, SIDE, 3).astype(np.float64) - d64).max(-1)
    unit_o, unit_d = camera_ref.fp32_ray_units(o64, d64, e_o, e_d)
    worst_o, worst_d = float((err_o / (law_common.U * unit_o)).max()), float((err_d / (law_common.U * unit_d)).max())
    fig = f"{name}: camera kind {kind}, lens {cam[21]:g}: origin off by {worst_o:.3f} units, direction by {worst_d:.3f} (K = {K_FACTOR:g})"
    assert worst_o <= K_FACTOR and worst_d <= K_FACTOR, fig
    return fig


def record_level_a(name):
    blob = LEVEL_A[name]()
    rays, rt, gt = level_a_rays(blob)
    out = {"blob": np.frombuffer(blob, np.uint8), "rays": rays, "ray_time": rt, "gather_time": gt}
    for build in BUILDS:
        for k, v in intersect(build, blob, rays, rt, gt).items():
            out[f"{k}_{build}"] = v
    return out


# ---------------------------------------------------------------- level B: the comparison
def relative(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def builds_disagree(fx):
    """(mask (h, w) of the samples on which the two builds disagree, the largest relative difference over those whose counts agree)."""
    counts_differ = (fx["counts_plain"][..., :2] != fx["counts_fma"][..., :2]).any(-1)
    rel = relative(fx["frame_plain"], fx["frame_fma"]).max(-1)
    decided = counts_differ | (rel > DECISION)
    constant = float(rel[~decided].max())
    return counts_differ | (rel > TOLERANCE), constant


def display(radiance):
    """Linear radiance of one sample (h, w, >= 3) -> what raygen.cu:151-155 stores."""
    return np.sqrt(np.asarray(radiance, np.float32)[..., :3])


def check_frame(name, fx, got, segments=None, shadow_rays=None, what="oracle"):
    """A frame `got` (h, w, 3), already square-rooted, against the fixture of level B case `name`: every channel within TOLERANCE
    of the reference's (no-contraction build) on all but CAP of the samples, the counts within that share. Returns the figures."""
    want = fx["frame_plain"]
    assert got.shape == want.shape, (got.shape, want.shape)
    rel = relative(got, want).max(-1)
    out = rel > TOLERANCE
    fig = f"{name} ({what}): {int(out.sum())} of {out.size} samples outside {TOLERANCE:.3g} ({100 * out.mean():.3f} %), largest inside {rel[~out].max():.3g}"
    for y, x in np.argwhere(out)[:64]:
        fig += f"\n  pixel ({x}, {y}): {got[y, x]} against the reference's {want[y, x]}"
    assert out.mean() <= CAP, fig
    for k, v, col in (("segments", segments, 0), ("shadow_rays", shadow_rays, 1)):
        if v is not None:
            ref = int(fx["counts_plain"][..., col].astype(np.int64).sum())
            fig += f"\n  {k} {int(v)}, the reference's traversals {ref}"
            assert abs(int(v) - ref) <= CAP * max(ref, out.size), fig
    return fig


def oracle_frame(blob, depth=DEPTH, sample=0):
    """The oracle's sample `sample` of every pixel of a SIDE x SIDE frame, TEA+LCG, the reference's estimator: (display frame, stats)."""
    import oracle
    p = abi.make_params(SIDE, SIDE, 1, depth, rng_kind=abi.RTW_RNG_TEA_LCG, estimator=abi.RTW_EST_REFERENCE, sample_offset=sample)
    img, st = oracle.render(blob, p, threads=4)
    return display(img), st
