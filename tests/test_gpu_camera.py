"""The kernels' camera rays against tests/camera_ref.py (a float64 reading of the reference's camera, raygen and sampling programs
that shares nothing with the oracle or the kernels), then against the oracle's bits of the same samples, so that a failure says
which side moved. Every written-out copy of the camera is reached: rtw_render through k_path (perspective without a lens -
sky-pinhole-* and wall24-pinhole, camera_ref.lens_free_reference_camera -: the LDS frame and, under Philox, the reserve of rays
made ahead of time; a lens, the environment and the orthographic camera, the moving sphere: the other instantiation) and through
k_first (as uploaded, with the tree forced, with the tree outside LDS), rtw_render_guides, rtw_views and rtw_views_guides
(view_raygen<>), and rtw_radiance on the law's own rays (the header's "Hence"). One-sample frames of 24 x 16 over seven sample
offsets, row shards, the far corner of an 8K image, and one mean of 144 samples per camera kind; both generators."""
import numpy as np
import pytest

import camera_ref as L
import view_ref as V
import gpu_common
from gpu_common import UPLOADS_LDS as UPLOADS, gpu, same_bits  # noqa: F401
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu

WALL_CASES = [n for n in L.CASES if n.startswith("wall")]


def upload(gpu, monkeypatch, blob, how="as_uploaded", path=None):
    gpu_common.upload(gpu, monkeypatch, blob, how, knobs=gpu_common.UPLOAD_KNOBS + ("RTW_PATH",), env=None if path is None else {"RTW_PATH": path})


def all_runs(draws=(0, 1)):
    return [pytest.param(name, rng, draw, id=f"{name}-rng{rng}-draw{draw}") for name in L.CASES for rng in L.RNGS for draw in draws]


K_FIRST, K_PATH = (abi.Stats.KERNELS.index(k) for k in ("k_first", "k_path"))
# rtw_stats tells k_first from k_path, not one instantiation of k_path from another: which cases the scene preparation gives to the
# hot one is camera_ref.lens_free_reference_camera's reading of it, held here so that the set cannot empty unnoticed
HOT_CASES = [n for n in L.CASES if L.lens_free_reference_camera(n) and not n.startswith("wall300")]
assert set(HOT_CASES) == {"wall24-pinhole", "sky-pinhole-v", "sky-pinhole-w", "sky-pinhole-u"} and set(HOT_CASES) - {"wall24-pinhole"} <= set(L.MEAN_CASES)


def law_then_oracle(gpu, name, rng, draw, kernel, frames=None):
    """The float64 reference first, the oracle's bits second, on the same rendered frames; every render must have run `kernel`
    and not the other one."""
    got = {}

    def render(frame, sample, seed):
        img, st = gpu.render(frame.params(1, sample, seed, rng))
        launches = (st.kernel_launches[K_FIRST], st.kernel_launches[K_PATH])
        assert launches[kernel == K_PATH] > 0 and launches[kernel != K_PATH] == 0, f"{name} {tuple(frame)}: k_first, k_path launches {launches}"
        got[(frame, sample, seed)] = img
        return img
    print(L.check_run(name, rng, draw, render, frames=frames))
    for (frame, sample, seed), img in got.items():
        want = L.oracle_frame(name, frame, sample, seed, rng)
        assert same_bits(img, want), f"{name} {tuple(frame)} sample {sample}: {int((img != want).any(-1).sum())} samples differ from the oracle's"


# ---------------------------------------------------------------- rtw_render
@pytest.mark.parametrize("name,rng,draw", all_runs())
def test_render_k_path_matches_float64_reference_and_oracle(gpu, monkeypatch, name, rng, draw):
    """RTW_PATH=1: every frame and sample offset of the draw, the row shards and the far corner among them. k_path renders the
    scenes whose primitives fit its lists; the wall of 300 tiles goes through the tree and k_first whatever RTW_PATH says."""
    upload(gpu, monkeypatch, L.case(name).blob, path="1")
    law_then_oracle(gpu, name, rng, draw, K_FIRST if name.startswith("wall300") else K_PATH)


@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name,rng,draw", all_runs(draws=(0,)))
def test_render_k_first_matches_float64_reference_and_oracle(gpu, monkeypatch, name, rng, draw, how):
    """RTW_PATH=0: k_first with the list walk, the whole-wave tree walk and the tree outside LDS; the seven sample offsets and the
    interleaved shard."""
    upload(gpu, monkeypatch, L.case(name).blob, how, path="0")
    law_then_oracle(gpu, name, rng, draw, K_FIRST, frames=("full", "stride"))


@pytest.mark.parametrize("path", ["1", "0"])
@pytest.mark.parametrize("rng,seed", [(L.PHILOX, L.SEEDS[0]), (L.PHILOX, L.SEEDS[1]), (L.TEA_LCG, L.SEEDS[0])])
@pytest.mark.parametrize("name", L.MEAN_CASES)
def test_render_mean_of_144_samples(gpu, monkeypatch, name, rng, seed, path):
    """144 samples cross a block of 16 and a unit of 128. In sky-pinhole-* under Philox and RTW_PATH=1 a lane of k_path's hot
    instantiation makes the rays of its next samples ahead of time and takes them from its LDS reserve: a reserve that handed out
    another sample's ray would move the mean's three components. The other mean cases run the instantiation that makes each ray
    when the lane needs it."""
    upload(gpu, monkeypatch, L.case(name).blob, path=path)
    img, st = gpu.render(L.FULL.params(L.MEAN_SPP, 0, seed, rng))
    assert (st.kernel_launches[K_PATH] > 0) == (path == "1") and (st.kernel_launches[K_FIRST] > 0) == (path == "0")
    print(L.check_mean(name, seed, rng, img))
    assert same_bits(img, L.oracle_frame(name, L.FULL, 0, seed, rng, L.MEAN_SPP))


# ---------------------------------------------------------------- rtw_render_guides
@pytest.mark.parametrize("rng", L.RNGS)
@pytest.mark.parametrize("name", WALL_CASES)
def test_render_guides_prim_and_depth(gpu, monkeypatch, name, rng):
    """prim and depth of the samples the beauty renders: prim exact and depth within the tolerance against the law, and prim is
    the primitive the beauty's colour names, miss for miss."""
    c = L.case(name)
    upload(gpu, monkeypatch, c.blob)
    seed, todo = L.runs(rng, 0)
    results = {}
    for fname, sample in todo:
        frame = L.FRAMES[fname]
        p = frame.params(1, sample, seed, rng)
        g = gpu.render_guides(p, which=("depth", "prim"))
        e = L.expect(name, frame, sample, seed, rng)
        results.setdefault(fname, []).append(L.check_guides(c, e, g["prim"], g["depth"], f"{name} {fname} sample {sample}: "))
        print(results[fname][-1].fig)
        img, _ = gpu.render(p)
        named = c.colours[g["prim"]]
        assert np.array_equal(img[..., :3], named), f"{name} {fname} sample {sample}: {int((img[..., :3] != named).any(-1).sum())} guide primitives are not the beauty's"
    for fname, rs in results.items():
        print(L.pooled(rs, f"{name} {fname}: "))


# ---------------------------------------------------------------- rtw_views, rtw_views_guides: view_raygen<>
VIEW_SEEDS = (0x6314759, 12345, 0xfeedbeef, 0x6314759)  # the second perspective view shares view 0's seed
VIEW_SHUTTERS = ((0.25, 0.75), (0.3, 0.9), (0.5, 0.5), (0.6, 0.7))  # every view has its own time0 / time1


class ViewCase:
    """A view of an uploaded scene as camera_ref reads a case: the view's camera, type and times, the scene's primitives."""

    def __init__(self, kind, blob, cam, camera_type, wall=None):
        self.kind, self.blob = kind, blob
        self.cam, self.camera_type = np.asarray(cam, np.float64).astype(np.float32), camera_type
        if wall:
            self.colours = L.wall_colours(wall)

    def view(self, seed):
        return abi.make_view(self.cam, self.camera_type, seed)


def sphere_views():
    which = ("perspective", "environment", "orthographic", "perspective")
    out = []
    for w, shutter in zip(which, VIEW_SHUTTERS):
        kind, cam = L._sphere_camera(w, shutter)
        out.append(ViewCase("shutter", L._sphere_blob(), cam, kind))
    return out


def wall_views(wall):
    out = []
    for w in ("pinhole", "environment", "orthographic", "lens"):
        kind, cam = L._wall_camera(w)
        out.append(ViewCase("wall", L._wall_blob(wall), cam, kind, wall))
    return out


@pytest.mark.parametrize("rng", L.RNGS)
@pytest.mark.parametrize("scene", ["sphere", "wall300", "wall24"])
def test_views_match_float64_reference_and_oracle(gpu, monkeypatch, scene, rng):
    """One call with all three camera kinds as views of one scene, each with its own seed and its own time0 / time1: the key is
    the pixel within the view, the times are the view's."""
    cases = sphere_views() if scene == "sphere" else wall_views(scene)
    upload(gpu, monkeypatch, cases[0].blob)
    views = [c.view(s) for c, s in zip(cases, VIEW_SEEDS)]
    w, h = L.FULL.width, L.FULL.height
    results = {}
    for sample in L.SAMPLE_OFFSETS:
        frames = gpu.views(views, w, h, 1, 1, rng_kind=rng, sample_offset=sample)
        for v, (c, seed) in enumerate(zip(cases, VIEW_SEEDS)):
            r = L.check_expectation(c, L.expect_of(c, L.FULL, sample, seed, rng), frames[v], f"{scene} view {v} sample {sample}: ")
            print(r.fig)
            results.setdefault(v, []).append(r)
        want, _, _ = V.expect(cases[0].blob, views, abi.make_view_params(w, h, 1, 1, rng_kind=rng, sample_offset=sample))
        assert same_bits(frames, want), f"{scene} sample {sample}: {int((frames != want).any(-1).sum())} samples differ from the oracle's"
    for v, rs in results.items():
        print(L.pooled(rs, f"{scene} view {v}: "))
    if scene == "sphere":  # views 0 and 3 share a seed and a camera but not a shutter: the frames must differ
        assert not np.array_equal(frames[0], frames[3])


@pytest.mark.parametrize("rng", L.RNGS)
@pytest.mark.parametrize("wall", ["wall300", "wall24"])
def test_views_guides_prim_and_depth(gpu, monkeypatch, wall, rng):
    cases = wall_views(wall)
    upload(gpu, monkeypatch, cases[0].blob)
    views = [c.view(s) for c, s in zip(cases, VIEW_SEEDS)]
    w, h = L.FULL.width, L.FULL.height
    results = {}
    for sample in L.SAMPLE_OFFSETS:
        g = gpu.views_guides(views, w, h, spp=1, which=("depth", "prim"), rng_kind=rng, sample_offset=sample)
        frames = gpu.views(views, w, h, 1, 1, rng_kind=rng, sample_offset=sample)
        for v, (c, seed) in enumerate(zip(cases, VIEW_SEEDS)):
            e = L.expect_of(c, L.FULL, sample, seed, rng)
            results.setdefault(v, []).append(L.check_guides(c, e, g["prim"][v], g["depth"][v], f"{wall} view {v} sample {sample}: "))
            print(results[v][-1].fig)
            assert np.array_equal(frames[v][..., :3], c.colours[g["prim"][v]])
    for v, rs in results.items():
        print(L.pooled(rs, f"{wall} view {v}: "))


# ---------------------------------------------------------------- rtw_radiance: the header's "Hence" with the law's rays
@pytest.mark.parametrize("rng", L.RNGS)
@pytest.mark.parametrize("name", WALL_CASES + ["shutter-perspective"])
def test_radiance_on_the_laws_rays_is_the_renders_sample(gpu, monkeypatch, name, rng):
    """Ray i = the law's ray of pixel i of the 24 x 16 frame, rounded to float32, on key width * y + x = i: rtw_radiance returns
    what the law expects of the render's sample and, where the sample does not depend on the ray's last bits (a tile's colour, a
    hit's zero), the render's bits. The times are rtw_radiance's own draws for that key: a perspective path's, so the moving
    sphere is asked of the perspective camera only; the walls do not move and take every camera kind."""
    c = L.case(name)
    upload(gpu, monkeypatch, c.blob)
    seed = L.DRAWS[rng][0][0]
    results = []
    for sample in L.SAMPLE_OFFSETS:
        e = L.expect(name, L.FULL, sample, seed, rng)
        out = gpu.radiance(e["rays"].copy(), 1, 1, seed=seed, rng_kind=rng, sample_offset=sample, key_offset=0)
        assert np.array_equal(out[:, 3], np.ones(len(out), np.float32))
        out = out.reshape(L.FULL.height, L.FULL.width, 4)
        results.append(L.check_expectation(c, e, out, f"{name} sample {sample}: "))
        print(results[-1].fig)
        img, _ = gpu.render(L.FULL.params(1, sample, seed, rng))
        exact = e["well"] & ((e["prim"] >= 0) | (c.kind == "wall"))
        assert same_bits(out[exact], img[exact]), f"{name} sample {sample}: {int((out != img).any(-1)[exact].sum())} samples differ from the render's"
    print(L.pooled(results, f"{name}: "))
