"""Guide buffers (rtw_render_guides) and the guided denoiser (rtw_denoise_guided) on the GPU. The guide identities are exact
because the guides trace the beauty's own camera rays and read its hit records: an all-emitter scene's spp-1 beauty IS its
albedo guide, a primitive-coded emitter scene's beauty IS its prim guide."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guides_ref
import oracle
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


def _xf(x):
    m = np.array(x.m, np.float64).reshape(3, 4)
    inv = np.array(x.inv, np.float64).reshape(3, 4)
    return m, inv


@pytest.mark.parametrize("n_prims", [20, 48])  # candidate lists / tree
def test_normals_and_depth_against_the_geometry(gpu, n_prims):
    w, h = 96, 96
    blob = oracle.random_scene(11, w, h, n_prims=n_prims)
    gpu.upload_scene(blob)
    g = gpu.render_guides(abi.make_params(w, h, 1, 4))
    parts = abi.parse_scene(blob)
    org = np.array(parts["header"].camera.origin, np.float64)
    nrm, depth, prim = g["normal"][..., :3].astype(np.float64), g["depth"].astype(np.float64), g["prim"]
    assert (prim >= 0).sum() > 1000
    seen = set()
    for k in np.unique(prim[prim >= 0]):
        pr = parts["prims"][int(k)]
        sel = prim == k
        m, inv = _xf(parts["xforms"][pr.xform])
        if abi.PRIM_RECT_X <= pr.type <= abi.PRIM_RECT_Z:
            n = np.zeros(3)
            n[pr.type - abi.PRIM_RECT_X] = -1.0 if pr.flip else 1.0
            if pr.xform == 0:
                assert np.array_equal(nrm[sel], np.broadcast_to(n, nrm[sel].shape))
            else:
                nw = inv[:, :3].T @ n
                assert np.abs(nrm[sel] - nw / np.linalg.norm(nw)).max() < 1e-6
            seen.add(("rect", pr.xform != 0))
        elif pr.type == abi.PRIM_SPHERE:
            c, r = np.array(pr.p[:3], np.float64), float(pr.p[3])
            if pr.xform == 0:
                # the shading normal is (p - c) / r of the fp32 hit point p = o + t*d; t comes from fp32 quadratic roots with the
                # camera ~1000 units away, which puts p up to ~1e-2 off the surface (measured |n| - 1 up to 3.5e-4): the unit length
                # holds to 1e-3, the hit point itself (c + r*n, at the guide's depth from the camera) to 1e-5
                assert np.abs(np.linalg.norm(nrm[sel], axis=1) - 1.0).max() < 1e-3
                hit = c + r * nrm[sel]
                assert np.abs(np.linalg.norm(hit - org, axis=1) / depth[sel] - 1.0).max() < 1e-5
            else:
                # SURVEY Q13 (kept by the shading code): a transformed sphere's shading normal is (world point - object-space
                # centre) / r carried through the inverse transpose - no unit vector, and not recoverable without the exact
                # jittered ray: only checked to be finite and at a finite depth here
                assert np.isfinite(nrm[sel]).all() and np.isfinite(depth[sel]).all()
            seen.add(("sphere", pr.xform != 0))
    assert ("rect", False) in seen and ("sphere", False) in seen
    # misses
    assert np.all(np.isinf(depth[prim < 0])) and np.all(g["albedo"][prim < 0] == 0)


EMITTER_CASES = [
    # (scene seed, n_prims, motion, camera code, lens radius)
    (3, 20, False, 0, 0.0),
    (4, 20, True, 0, 8.0),
    (5, 48, True, 100, 0.0),
    (6, 48, False, 200, 0.0),
    (7, 48, True, 0, 8.0),
]


@pytest.mark.parametrize("seed,n_prims,motion,cam,lens", EMITTER_CASES)
@pytest.mark.parametrize("rng", [abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG])
def test_emitter_beauty_is_the_albedo_guide(gpu, seed, n_prims, motion, cam, lens, rng):
    """All-emitter scene, textures in [0, 1], sky off: the spp-1 beauty is L = 0 + Le * (1,1,1) for a front-face hit (the
    emitter ends the path, rtw_kernels.h shade_a), 0 on a back face or a miss - what the albedo guide holds, bit for bit."""
    w, h = 64, 48
    blob = oracle.random_scene(seed, w, h, n_prims=n_prims, motion=motion, textured=True)
    blob = guides_ref.with_camera(guides_ref.all_emitters(blob), cam, w, h, lens)
    gpu.upload_scene(blob)
    for off in (0, 37):
        p = abi.make_params(w, h, 1, 5, rng_kind=rng, sample_offset=off)
        img, _ = gpu.render(p)
        g = gpu.render_guides(p, which=("albedo", "prim"))
        assert (g["prim"] >= 0).sum() > 20  # (the orthographic view of the box sees a few primitives only)
        assert np.array_equal(img[..., :3], g["albedo"][..., :3])
        assert np.array_equal(g["albedo"][..., 3], (g["prim"] >= 0).astype(np.float32))


@pytest.mark.parametrize("n_prims", [20, 48])
def test_prim_identity(gpu, n_prims):
    w, h = 80, 60
    blob = oracle.random_scene(21, w, h, n_prims=n_prims, motion=True)
    n = len(abi.parse_scene(blob)["prims"])
    # colour of primitive i: ((i + 1) / 256, 0.5, 0.25), exact in float32
    cols = [((i + 1) / 256.0, 0.5, 0.25) for i in range(n)]
    gpu.upload_scene(guides_ref.all_emitters(blob, cols))
    for off in (0, 5, 113):
        p = abi.make_params(w, h, 1, 3, sample_offset=off)
        img, _ = gpu.render(p)
        prim = gpu.render_guides(p, which=("prim",))["prim"]
        lit = img[..., 1] != 0
        assert lit.sum() > 100
        assert np.array_equal(np.rint(img[..., 0][lit] * 256.0).astype(np.int32) - 1, prim[lit])
        assert np.all(prim[~lit] >= -1)
        assert np.all(img[..., :3][prim < 0] == 0)


@pytest.mark.parametrize("spp", [16, 40])
def test_means_are_contract_ordered_sums_of_single_samples(gpu, spp):
    w, h = 40, 24
    gpu.upload_scene(oracle.random_scene(31, w, h, n_prims=30, motion=True, textured=True))
    full = gpu.render_guides(abi.make_params(w, h, spp, 4, sample_offset=3))
    ones = [gpu.render_guides(abi.make_params(w, h, 1, 4, sample_offset=3 + s), which=("albedo", "normal")) for s in range(spp)]
    for k in ("albedo", "normal"):
        ref = guides_ref.contract_mean([o[k] for o in ones])
        assert np.array_equal(full[k][..., :3], ref[..., :3])
    first = gpu.render_guides(abi.make_params(w, h, 1, 4, sample_offset=3))
    assert np.array_equal(full["depth"], first["depth"]) and np.array_equal(full["prim"], first["prim"])


def test_row_shards_and_groups(gpu):
    w, h = 48, 30
    blob = oracle.random_scene(41, w, h, n_prims=40, textured=True)
    gpu.upload_scene(blob)
    full = gpu.render_guides(abi.make_params(w, h, 4, 4))
    shard = gpu.render_guides(abi.make_params(w, h, 4, 4, row0=5, row1=29, row_stride=3))
    for k in abi.GUIDES:
        assert np.array_equal(shard[k], full[k][5:29:3])
    grp = abi.Renderer([0, 0])
    try:
        grp.upload_scene(blob)
        st = abi.Stats()
        g2 = grp.render_guides(abi.make_params(w, h, 4, 4), stats=st)
        assert st.samples == st.segments == w * h * 4
    finally:
        grp.close()
    for k in abi.GUIDES:
        assert np.array_equal(g2[k], full[k])


def test_media_are_transparent_to_the_guides(gpu):
    w, h = 64, 48
    blob = oracle.random_scene(51, w, h, n_prims=30, volumes=True)
    parts = dict(abi.parse_scene(blob))
    vol = [pr for pr in parts["prims"] if pr.type in (abi.PRIM_VOLUME_BOX, abi.PRIM_VOLUME_SPHERE)]
    assert vol
    parts["prims"] = [pr for pr in parts["prims"] if pr.type not in (abi.PRIM_VOLUME_BOX, abi.PRIM_VOLUME_SPHERE)]
    p = abi.make_params(w, h, 4, 4)
    gpu.upload_scene(blob)
    a = gpu.render_guides(p)
    gpu.upload_scene(abi.assemble_scene(parts))
    b = gpu.render_guides(p)
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(a[k], b[k])


def _rect_scene(w, h, zs):
    """RECT_Z planes at the given depths in front of the Cornell camera, each larger than the view."""
    parts = dict(abi.parse_scene(oracle.random_scene(1, w, h, n_prims=2)))
    prims = []
    for z in zs:
        pr = abi.Prim(type=abi.PRIM_RECT_Z, material=0, xform=0, flip=0)
        for k, v in enumerate((-2000.0, 2000.0, -2000.0, 2000.0, z)):
            pr.p[k] = v
        prims.append(pr)
    parts.update(prims=prims, lights=[])
    return parts


def test_depth_of_an_orthographic_camera_is_the_plane_distance(gpu):
    w, h = 48, 32
    parts = _rect_scene(w, h, [300.0])
    blob = guides_ref.with_camera(abi.assemble_scene(parts), 200, w, h)
    cam = abi.parse_scene(blob)["header"].camera
    gpu.upload_scene(blob)
    g = gpu.render_guides(abi.make_params(w, h, 1, 2))
    wv = np.array(cam.w, np.float64)
    d = -wv / np.linalg.norm(wv)
    assert abs(d[2]) > 0.5  # the camera looks along z
    # ray origins lie on the image plane: origin = lower_left + s*horizontal + t*vertical + camera origin
    ll, hz, vt, o = (np.array(v, np.float64) for v in (cam.lower_left, cam.horizontal, cam.vertical, cam.origin))
    z0 = (ll + o)[2] + np.array([0, hz[2], vt[2], hz[2] + vt[2]])
    expect = (300.0 - z0) / d[2]
    assert g["prim"].min() == 0
    assert np.all(g["depth"] >= expect.min() * (1 - 1e-5)) and np.all(g["depth"] <= expect.max() * (1 + 1e-5))
    if np.ptp(expect) == 0:
        assert np.abs(g["depth"] / expect[0] - 1).max() < 1e-5


def test_depth_on_the_cornell_back_wall(gpu):
    w, h = 64, 64
    blob = abi.build_scene(0, w, h)
    parts = abi.parse_scene(blob)
    gpu.upload_scene(blob)
    g = gpu.render_guides(abi.make_params(w, h, 1, 2))
    # the back wall: the z-rectangle at the largest k
    back = max((i for i, pr in enumerate(parts["prims"]) if pr.type == abi.PRIM_RECT_Z and pr.xform == 0), key=lambda i: parts["prims"][i].p[4])
    kz = float(parts["prims"][back].p[4])
    cam = parts["header"].camera
    ll, hz, vt, o = (np.array(v, np.float64) for v in (cam.lower_left, cam.horizontal, cam.vertical, cam.origin))
    ys, xs = np.nonzero(g["prim"] == back)
    assert len(xs) > 200
    lo, hi = np.full(len(xs), np.inf), np.zeros(len(xs))
    for cx in (0, 1):
        for cy in (0, 1):
            d = ll + np.outer((xs + cx) / w, hz) + np.outer((ys + cy) / h, vt) - o
            dist = (kz - o[2]) / d[:, 2] * np.linalg.norm(d, axis=1)
            lo, hi = np.minimum(lo, dist), np.maximum(hi, dist)
    dep = g["depth"][ys, xs].astype(np.float64)
    assert np.all(dep >= lo * (1 - 1e-5)) and np.all(dep <= hi * (1 + 1e-5))


def test_guided_filter_with_constant_guides_is_rtw_denoise(gpu):
    rs = np.random.RandomState(3)
    img = rs.uniform(0, 1, (45, 61, 4)).astype(np.float32)
    for av, nv in ((0.0, 0.0), (0.4, -0.6)):
        got = gpu.denoise_guided(img, np.full_like(img, av), np.full_like(img, nv), 5, 0.5, 0.1, 0.2)
        assert np.array_equal(got, gpu.denoise(img, 5, 0.5))


def test_guided_filter_matches_the_restatement(gpu):
    rs = np.random.RandomState(4)
    img = rs.uniform(0, 1, (37, 53, 4)).astype(np.float32)
    alb = rs.uniform(0, 1, img.shape).astype(np.float32)
    nrm = rs.uniform(-1, 1, img.shape).astype(np.float32)
    for it, s, sa, sn in ((5, 0.5, 0.1, 0.25), (3, 0.3, 0.7, 0.05), (8, 1.0, 2.0, 1.0)):
        assert np.array_equal(gpu.denoise_guided(img, alb, nrm, it, s, sa, sn), guides_ref.atrous_guided(img, alb, nrm, it, s, sa, sn))


def test_guided_filter_keeps_edges(gpu):
    h, w, e = 48, 64, 32
    rs = np.random.RandomState(6)
    clean = np.zeros((h, w, 4), np.float32)
    clean[:, :e, :3], clean[:, e:, :3] = 0.25, 0.65
    clean[..., 3] = 1
    img = clean.copy()
    img[..., :3] += rs.normal(0, 0.08, (h, w, 3)).astype(np.float32)
    alb = np.zeros_like(clean)
    alb[:, :e, :3], alb[:, e:, :3] = 0.3, 0.8
    nrm = np.zeros_like(clean)
    nrm[:, :e, 0], nrm[:, e:, 2] = 1.0, 1.0
    cols = slice(e - 1, e + 1)
    err = lambda out: float(np.sqrt(np.mean((out[:, cols, :3] - clean[:, cols, :3]) ** 2)))
    guided, plain = gpu.denoise_guided(img, alb, nrm, 5, 0.5), gpu.denoise(img, 5, 0.5)
    assert err(guided) <= 0.5 * err(plain), (err(guided), err(plain))


# How much lower the guided filter's RMSE against a 1024-spp reference is than the colour-only filter's, with the default sigmas.
# Measured (scripts/guide_sweep.py; the renders are deterministic): scene 0 4.5 %, scene 2 1.8 %. The best sigmas of the sweep give
# less than the 10 % first estimated, so the bound is a strict "guided beats colour-only" with the measured margin, rounded down.
QUALITY_MARGIN = {0: 0.03, 2: 0.01}


@pytest.mark.parametrize("scene", [0, 2])
def test_guided_beats_colour_only_on_reference_scenes(gpu, scene):
    n = 256
    gpu.upload_scene(abi.build_scene(scene, n, n))
    p = abi.make_params(n, n, 8, 50)
    noisy, _ = gpu.render(p)
    ref, _ = gpu.render(abi.make_params(n, n, 1024, 50, seed=0x1234567))
    g = gpu.render_guides(p, which=("albedo", "normal"))
    enc, ref_enc = guides_ref.encode(noisy), guides_ref.encode(ref)
    rm = lambda a: float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref_enc[..., :3]) ** 2)))
    plain = rm(gpu.denoise(enc, 5, 0.5))
    guided = rm(gpu.denoise_guided(enc, g["albedo"], g["normal"], 5, 0.5))
    print(f"scene {scene}: noisy {rm(enc):.5f} colour-only {plain:.5f} guided {guided:.5f} ({1 - guided / plain:+.1%})")
    assert guided < (1.0 - QUALITY_MARGIN[scene]) * plain


def test_guide_errors(gpu):
    lib = abi.load_hip()
    r = abi.Renderer(0)
    try:
        p = abi.make_params(8, 8, 1, 2)
        buf = np.zeros(8 * 8 * 4, np.float32)
        g = abi.Guides(albedo=buf.ctypes.data)
        assert lib.rtw_render_guides(r.ctx, C.byref(p), C.byref(g), None) == -3  # no scene
        r.upload_scene(abi.build_scene(0, 8, 8))
        assert lib.rtw_render_guides(r.ctx, C.byref(p), C.byref(abi.Guides()), None) == -1  # no buffer
        bad = abi.make_params(8, 8, 0, 2)
        assert lib.rtw_render_guides(r.ctx, C.byref(bad), C.byref(g), None) == -1
        assert lib.rtw_denoise_guided(r.ctx, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 8, 8, 1, 0.5, 0.1, 0.1) == -1
    finally:
        r.close()


def _read_pfm(path):
    raw = open(path, "rb").read()
    parts = raw.split(b"\n", 3)
    w, h = (int(v) for v in parts[1].split())
    ch = 3 if parts[0] == b"PF" else 1
    return np.frombuffer(parts[3], "<f4").reshape((h, w, ch) if ch == 3 else (h, w))


def test_cli_writes_the_guides(gpu, tmp_path):
    cli = os.path.join(ROOT, "raytracing_weekend_amd", "host", "rtw_render")
    base = [cli, "-s", "0", "-ns", "4", "-dx", "64", "-dy", "48", "-d", "5"]
    plain = subprocess.run(base + ["-o", str(tmp_path / "a.pfm")], capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    prefix = str(tmp_path / "g")
    run = subprocess.run(base + ["-o", str(tmp_path / "b.pfm"), "-aov", prefix, "-guide_spp", "3"], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert open(tmp_path / "a.pfm", "rb").read() == open(tmp_path / "b.pfm", "rb").read()
    gpu.upload_scene(abi.build_scene(0, 64, 48))
    g = gpu.render_guides(abi.make_params(64, 48, 3, 5), which=("albedo", "normal", "depth"))
    assert np.array_equal(_read_pfm(prefix + "_albedo.pfm"), g["albedo"][..., :3])
    assert np.array_equal(_read_pfm(prefix + "_normal.pfm"), g["normal"][..., :3])
    assert np.array_equal(_read_pfm(prefix + "_depth.pfm"), g["depth"])
    den = subprocess.run(base + ["-o", str(tmp_path / "c.pfm"), "-denoise", "3", "-guided"], capture_output=True, timeout=120)
    assert den.returncode == 0, den.stderr
    assert _read_pfm(str(tmp_path / "c.pfm")).shape == (48, 64, 3)
