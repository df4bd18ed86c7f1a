"""GPU suite of the views (include/rtw.h rtw_views / rtw_views_device). The referee is the contract itself: frame v is rtw_render's
frame of the scene with views[v] in its header, which the oracle renders as it stands (view_ref). Then odd shapes with the summation
units and offsets, the golden fixtures, independence of the call's other views, chunks and slab ranges, the torch path, every
refusal, groups, sessions, the older entry points afterwards, and the command-line turntable."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import geometry_ref as G
import gpu_common
import probe_ref as P
import radiance_ref as R
import view_ref as V
from gpu_common import (BOTH, GOLD, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render,  # noqa: F401
                        check_stream_order, golden, gpu, left_alone, same, sentinel_stats, upload)
from raytracing_weekend_amd import abi, bake
from raytracing_weekend_amd.torch_views import views_tensor, views_torch

pytestmark = pytest.mark.gpu
ROOT = abi.REPO_DIR
first_difference = functools.partial(gpu_common.first_difference, what="pixels (view, y, x)", axes=3)


def call(gpu, views, params, stats=None):
    return gpu.views(views, params.width, params.height, params.spp, params.max_depth, rng_kind=params.rng_kind,
                     sample_offset=params.sample_offset, estimator=params.estimator, stats=stats)


# ---------------------------------------------------------------- 1. every frame is the oracle's render of that camera, counts included
def check_main(gpu, name, rng_kind, estimator=0):
    blob, views, params, want, seg, shadow = V.case(name, rng_kind, estimator)
    st = abi.Stats()
    got = call(gpu, views, params, st)
    lit = [V.lit_fraction(f) for f in want]
    print(f"{name} rng {rng_kind} estimator {estimator}: segments {st.segments} (oracle {seg}), shadow rays {st.shadow_rays} ({shadow}), "
          f"non-zero fractions {lit}")
    # not black frames: tests/test_views_cpu.py holds the cameras to MIN_LIT under the reference estimator. Estimator 2 samples no
    # lights, and at 48 spp most of the box stays black in a render as well: there every view must still show something.
    assert min(lit) >= V.MIN_LIT if estimator == 0 else min(lit) > 0.0
    assert got.shape == (3, V.H, V.W, 4) and same(got, want), first_difference(got, want)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 3 * V.W * V.H * V.SPP)
    assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    assert (got[..., 3] == 1.0).all()


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", V.SCENES)
def test_every_frame_is_the_render_of_the_scene_with_that_camera(gpu, monkeypatch, name, how, rng_kind):
    upload(gpu, monkeypatch, R.scene(name), how)
    check_main(gpu, name, rng_kind)


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("estimator", [1, 2, 3])
def test_under_the_corrected_estimators_on_scene_0(gpu, monkeypatch, estimator, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    check_main(gpu, "scene0", rng_kind, estimator)


# ---------------------------------------------------------------- 2. odd shapes, units, tails, offsets
@pytest.mark.parametrize("spp", [1, 16, 17, 129, 272])
def test_odd_shapes_summation_units_and_sample_offsets(gpu, monkeypatch, spp):
    """Three views of 7 x 5: 35 pixels a frame, so the view boundaries fall inside a wave and neither the width nor the frame is a
    power of two or a multiple of 64. One sample; one full block; a block and a one-sample tail; a unit and a one-sample unit (the
    slab and the resolve); two units and a 16-sample tail. Offset 40 starts inside what would be a block of an offset-0 call."""
    name = "scene0"
    upload(gpu, monkeypatch, R.scene(name))
    views = list(V.cameras(name))
    for off, rng_kind in ((0, abi.RTW_RNG_PHILOX), (40, abi.RTW_RNG_TEA_LCG), (40, abi.RTW_RNG_PHILOX)):
        params = abi.make_view_params(7, 5, spp, 6, rng_kind=rng_kind, sample_offset=off)
        want, seg, shadow = V.expect(R.scene(name), views, params)
        st = abi.Stats()
        got = call(gpu, views, params, st)
        assert got.shape == (3, 5, 7, 4) and same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 3 * 35 * spp)
        assert max(V.lit_fraction(f) for f in want) > 0.5


# ---------------------------------------------------------------- 3. the golden fixtures
@pytest.mark.parametrize("fixture", ["cornell_200x200_16spp_d4_philox", "cornell_200x200_16spp_d4_lcg"])
def test_the_scenes_own_camera_gives_the_golden_frames(gpu, monkeypatch, fixture):
    z = np.load(os.path.join(GOLD, fixture + ".npz"))
    scene, w, h, spp, depth, rng, seed = (int(v) for v in z["meta"])
    assert (scene, w, h) == (0, 200, 200)
    blob = abi.build_scene(0, 200, 200)
    upload(gpu, monkeypatch, blob)
    view = abi.scene_view(blob, seed)
    st = abi.Stats()
    got = gpu.views([view, view], w, h, spp, depth, rng_kind=rng, stats=st)  # twice in one call
    for f in got:
        assert np.array_equal(f[..., :3].view(np.uint32), np.ascontiguousarray(z["rgb"][..., :3]).view(np.uint32)) and np.all(f[..., 3] == 1.0)
    assert (st.samples, st.segments, st.shadow_rays) == tuple(2 * int(v) for v in z["stats"])


# ---------------------------------------------------------------- 4. independence
def test_a_pixel_depends_on_its_view_its_place_and_the_params_alone(gpu, monkeypatch):
    name = "scene3"
    upload(gpu, monkeypatch, R.scene(name))
    a, b, c = V.cameras(name)
    for spp in (16, 144):
        alone = gpu.views([c], 7, 5, spp, 6)
        assert V.lit_fraction(alone[0]) > 0.5
        # the same record as view 40 of 41
        crowd = gpu.views([a, b] * 20 + [c], 7, 5, spp, 6)
        assert crowd.shape == (41, 5, 7, 4) and same(crowd[40:], alone)
        assert same(crowd[0], gpu.views([a], 7, 5, spp, 6)[0]) and same(crowd[39], gpu.views([b], 7, 5, spp, 6)[0])
        # and first of two, with a generator and an offset of its own
        p = dict(rng_kind=abi.RTW_RNG_TEA_LCG, sample_offset=24)
        assert same(gpu.views([c, a], 7, 5, spp, 6, **p)[:1], gpu.views([c], 7, 5, spp, 6, **p))
    # chunks of 50 pixels begin and end mid-row and mid-view
    views = [a, b, c]
    want16, want272 = gpu.views(views, 7, 5, 16, 6), gpu.views(views, 7, 5, 272, 6)
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "50")
    s0 = abi.Stats()
    assert same(gpu.views(views, 7, 5, 16, 6, stats=s0), want16) and same(gpu.views(views, 7, 5, 272, 6), want272)
    assert s0.samples == 3 * 35 * 16 and s0.segments > 0
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "1")
    assert same(gpu.views(views, 7, 5, 16, 6), want16)
    monkeypatch.delenv("RTW_RADIANCE_CHUNK")
    # a slab cap of 50 pixels' unit sums cuts the 105 pixels at spp 272 (3 units) into ranges 50, 50, 5: two of them split a view
    monkeypatch.setenv("RTW_RADIANCE_SLAB_BYTES", str(50 * 3 * 16))
    s1 = abi.Stats()
    assert same(gpu.views(views, 7, 5, 272, 6, stats=s1), want272)
    d_views = views_tensor(views, "cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        assert same(views_torch(gpu, d_views, 7, 5, 272, 6).cpu().numpy(), want272)
    monkeypatch.setenv("RTW_RADIANCE_SLAB_BYTES", "16")  # one pixel per range
    assert same(gpu.views(views, 7, 5, 272, 6), want272)
    monkeypatch.delenv("RTW_RADIANCE_SLAB_BYTES")
    s2 = abi.Stats()
    assert same(gpu.views(views, 7, 5, 272, 6, stats=s2), want272) and (s1.segments, s1.shadow_rays) == (s2.segments, s2.shadow_rays)


# ---------------------------------------------------------------- 5. the device path
def test_views_torch_equals_views_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    name = "random_volumes_motion"
    blob, views, params, want, seg, shadow = V.case(name, abi.RTW_RNG_PHILOX)
    upload(gpu, monkeypatch, blob)
    d_views = views_tensor(views, "cuda:0")
    assert tuple(d_views.shape) == (3, 28) and d_views.cpu().numpy().tobytes() == bytes(abi.view_array(views))
    st = abi.Stats()
    torch.cuda.synchronize()
    got = views_torch(gpu, d_views, V.W, V.H, V.SPP, V.DEPTH, stats=st)
    assert got.is_cuda and tuple(got.shape) == (3, V.H, V.W, 4) and same(got.cpu().numpy(), want)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 3 * V.W * V.H * V.SPP) and st.seconds > 0.0
    check_stream_order(lambda t: views_torch(gpu, t, V.W, V.H, V.SPP, V.DEPTH), d_views, lambda got: same(got.cpu().numpy(), want))
    assert tuple(views_torch(gpu, torch.zeros((0, 28), device="cuda:0"), 4, 3, 4, 4).shape) == (0, 3, 4, 4)
    for kw in (dict(width=0), dict(height=-1), dict(spp=0)):
        args = dict(width=V.W, height=V.H, spp=V.SPP, max_depth=V.DEPTH)
        args.update(kw)
        with pytest.raises(ValueError):
            views_torch(gpu, d_views, **args)


@pytest.mark.parametrize("rng_kind", BOTH)
def test_on_the_device_an_unknown_camera_type_is_a_perspective_camera(gpu, monkeypatch, rng_kind):
    """rtw_views_device does not read the records back: a type of 7 renders as type 0, lens draws included (the TEA+LCG stream shows
    them), and the reserved words are ignored. rtw_views, which can read them, refuses both."""
    name = "scene0"
    upload(gpu, monkeypatch, R.scene(name))
    a = V.cameras(name)[0]
    want = gpu.views([a], V.W, V.H, 32, 6, rng_kind=rng_kind)
    odd = abi.View.from_buffer_copy(bytes(a))
    odd.camera_type = 7
    odd.reserved[0], odd.reserved[1] = 5, 0xffffffff
    got = views_torch(gpu, views_tensor([odd], "cuda:0"), V.W, V.H, 32, 6, rng_kind=rng_kind)
    assert same(got.cpu().numpy(), want) and V.lit_fraction(want[0]) > 0.5
    neg = abi.View.from_buffer_copy(bytes(a))
    neg.camera_type = -1
    assert same(views_torch(gpu, views_tensor([neg], "cuda:0"), V.W, V.H, 32, 6, rng_kind=rng_kind).cpu().numpy(), want)


# ---------------------------------------------------------------- 6. refusals and side effects
def test_every_refusal_leaves_the_context_usable_and_writes_nothing(gpu, monkeypatch):
    name = "scene0"
    blob = R.scene(name)
    upload(gpu, monkeypatch, blob)
    views = abi.view_array(V.cameras(name))
    n, w, h, spp = 3, 7, 5, 16
    want = gpu.views(views, w, h, spp, 6)
    lib = gpu.lib
    out = np.full((n, h, w, 4), -7, np.float32)
    d_views = torch.cat([views_tensor(views, "cuda:0").ravel(), torch.zeros(8, device="cuda:0")])
    d_out = torch.full((n * h * w * 4 + 8,), -7.0, device="cuda:0")
    V_, O_, D_, DO_ = C.addressof(views), out.ctypes.data, d_views.data_ptr(), d_out.data_ptr()

    def vp(**kw):
        p = abi.make_view_params(w, h, spp, 6)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_views(fresh.ctx, V_, n, vp(), O_, None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_views_device(fresh.ctx, D_, n, vp(), DO_, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()

    def still_fine():
        assert same(gpu.views(views, w, h, spp, 6), want)
    bad_params = [None, vp(width=0), vp(width=-1), vp(height=0), vp(height=-5), vp(spp=0), vp(spp=-1), vp(max_depth=-1), vp(rng_kind=2), vp(rng_kind=-1),
                  vp(estimator=4), vp(estimator=-1), vp(sample_offset=-1), vp(sample_offset=2 ** 31 - spp), vp(spp=2 ** 31 - 1, sample_offset=1),
                  vp(reserved=1), vp(reserved=2 ** 31), vp(width=2 ** 16, height=2 ** 15), vp(width=2 ** 31 - 1, height=2 ** 31 - 1)]
    too_many = [(2 ** 31 - 1) // 35 + 1, 1 << 31, 1 << 40, 2 ** 64 - 1]  # n_views * width * height beyond 2^31 - 1, the last ones beyond 64 bits
    refusals = [(V_, n, p, O_) for p in bad_params] + [(V_, m, vp(), O_) for m in too_many] + [(None, n, vp(), O_), (V_, n, vp(), None)]
    for v_, m, p, o_ in refusals:
        st = sentinel_stats()
        assert lib.rtw_views(gpu.ctx, v_, m, p, o_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    # the host variant reads the records: a camera type outside 0..2 and a non-zero reserved word, in any view
    for field, value in (("camera_type", 3), ("camera_type", -1), ("camera_type", 7), ("reserved0", 1), ("reserved1", 2 ** 31)):
        bad = abi.view_array([abi.View.from_buffer_copy(bytes(v)) for v in views])
        if field == "camera_type":
            bad[2].camera_type = value
        else:
            bad[1].reserved[int(field[-1])] = value
        st = abi.Stats(segments=77, seconds=7.0)
        assert lib.rtw_views(gpu.ctx, C.addressof(bad), n, vp(), O_, C.byref(st)) == -1 and (st.segments, st.seconds) == (77, 7.0)
        assert b"view" in lib.rtw_last_error(gpu.ctx)
    still_fine()
    dev_refusals = [(D_, n, p, DO_) for p in bad_params] + [(D_, m, vp(), DO_) for m in too_many] + [
        (None, n, vp(), DO_), (D_, n, vp(), None), (D_ + 4, n, vp(), DO_), (D_ + 8, n, vp(), DO_), (D_, n, vp(), DO_ + 4), (D_, n, vp(), DO_ + 8)]
    for v_, m, p, o_ in dev_refusals:
        st = sentinel_stats()
        assert lib.rtw_views_device(gpu.ctx, v_, m, p, o_, None, C.byref(st)) == -1
        assert left_alone(st)
    still_fine()  # after a misaligned pointer as after any other refusal: the next call works
    torch.cuda.synchronize()
    assert (out == -7).all() and bool((d_out == -7).all().item())  # no refused call wrote anything
    # n_views = 0 is fine and launches nothing, whatever the pointers
    st = abi.Stats(segments=77)
    assert lib.rtw_views(gpu.ctx, None, 0, vp(), None, C.byref(st)) == 0 and (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
    assert lib.rtw_views(gpu.ctx, None, 0, vp(width=2 ** 31 - 1, height=2 ** 31 - 1), None, None) == 0
    assert lib.rtw_views_device(gpu.ctx, None, 0, vp(), None, None, None) == 0
    assert lib.rtw_views_device(gpu.ctx, D_ + 4, 0, vp(), DO_ + 4, None, None) == 0
    assert gpu.views([], w, h, spp, 6).shape == (0, h, w, 4)
    torch.cuda.synchronize()
    assert bool((d_out == -7).all().item())
    # from view 1 on, 16 bytes into the output: aligned enough, and nothing is written beside the frames
    assert lib.rtw_views_device(gpu.ctx, D_ + 112, n - 1, vp(), DO_ + 16, None, None) == 0
    assert same(d_out[4:4 + 4 * 35 * (n - 1)].cpu().numpy().reshape(n - 1, h, w, 4), want[1:])
    assert bool((d_out[:4] == -7).all().item()) and bool((d_out[4 + 4 * 35 * (n - 1):] == -7).all().item())
    # Python's own refusals
    for bad in (dict(width=0), dict(spp=0), dict(height=2.5)):
        args = dict(width=w, height=h, spp=spp, max_depth=6)
        args.update(bad)
        with pytest.raises(ValueError):
            gpu.views(views, **args)
    with pytest.raises(ValueError):
        gpu.views([None], w, h, spp, 6)
    with pytest.raises(ValueError):
        gpu.views(views, 2 ** 15, 2 ** 15, spp, 6)
    zero = gpu.views(views, w, h, spp, 0)  # max_depth = 0: black frames, alpha 1
    assert not zero[..., :3].any() and (zero[..., 3] == 1.0).all() and same(gpu.views(views, w, h, 200, 0), zero)


def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    name = "scene1"
    blob = R.scene(name)
    upload(gpu, monkeypatch, blob)
    views = abi.view_array(V.cameras(name))
    group = abi.Renderer([0, 0])  # a {0, 0} group
    try:
        out = np.zeros((3, 5, 7, 4), np.float32)
        p0 = abi.make_view_params(7, 5, 16, 6)
        assert group.lib.rtw_views(group.ctx, C.addressof(views), 3, C.byref(p0), out.ctypes.data, None) == -3 and not out.any()
        group.upload_scene(blob)
        for spp in (16, 144):
            s0, s1 = abi.Stats(), abi.Stats()
            want = gpu.views(views, 7, 5, spp, 6, stats=s0)
            assert same(group.views(views, 7, 5, spp, 6, stats=s1), want) and V.lit_fraction(want[0]) > 0.5
            assert (s1.segments, s1.shadow_rays) == (s0.segments, s0.shadow_rays)
            assert same(views_torch(group, views_tensor(views, "cuda:0"), 7, 5, spp, 6).cpu().numpy(), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    name = "scene0"
    upload(gpu, monkeypatch, R.scene(name))
    views = list(V.cameras(name))
    want = gpu.views(views, 7, 5, 16, 6)
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        assert same(gpu.views(views, 7, 5, 16, 6), want)
        assert same(views_torch(gpu, views_tensor(views, "cuda:0"), 7, 5, 16, 6).cpu().numpy(), want)
        gpu.views(views, 7, 5, 144, 4)  # the unit slab and the resolve
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    assert same(gpu.views(views, 7, 5, 16, 6), want)


def test_render_probe_sh_radiance_and_cast_are_what_they_were_before_views_calls(gpu, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for g in map(golden, GOLDEN_PAIR):
        blob, rng, seed = g.blob, g.rng, g.seed
        gpu.upload_scene(blob)
        rays, _, _ = G.scene_rays(blob, 5, 300)
        rays[:, 6], rays[:, 7] = 1e-6, 1e27
        rad = gpu.radiance(rays, 24, 6, rng_kind=rng)
        hits = gpu.cast(rays)
        probes = P.scene_probes(gpu.cast, blob, 300, tmax=100.0)
        sh = gpu.probe_sh(probes, 160, 3, rng_kind=rng)
        views = bake.orbit_views(blob, 3, seed=seed) + bake.cube_views((278, 278, 278))
        a = gpu.views(views, 16, 12, 24, 6, rng_kind=rng)
        b = gpu.views(views, 16, 12, 160, 3, rng_kind=rng, estimator=1)  # the slab the other resolves read as well
        assert np.isfinite(a).all() and np.isfinite(b).all() and a[..., :3].sum() > 0 and b[..., :3].sum() > 0
        check_golden_render(gpu, g)
        assert same(gpu.radiance(rays, 24, 6, rng_kind=rng), rad) and same(gpu.probe_sh(probes, 160, 3, rng_kind=rng), sh)
        assert same(gpu.views(views, 16, 12, 24, 6, rng_kind=rng), a)
        again = gpu.cast(rays)
        assert all(np.array_equal(hits[k].view(np.uint32), again[k].view(np.uint32)) for k in hits)


# ---------------------------------------------------------------- 7. the command line
def test_cli_orbit_writes_the_turntable_of_renderer_views(gpu, monkeypatch, tmp_path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cli = os.path.join(ROOT, "raytracing_weekend_amd", "host", "rtw_render")
    assert os.path.exists(cli), "build() has not produced the CLI"
    w, h, spp, depth, seed = 48, 32, 16, 6, 99
    base = [cli, "-s", "0", "-dx", str(w), "-dy", str(h), "-ns", str(spp), "-d", str(depth), "-seed", str(seed)]
    plain = subprocess.run(base + ["-o", str(tmp_path / "p.pfm")], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    orbit = subprocess.run(base + ["-orbit", "3", "-o", str(tmp_path / "t.pfm")], capture_output=True, text=True, timeout=120)
    assert orbit.returncode == 0, orbit.stderr
    files = sorted(f for f in os.listdir(tmp_path) if f.startswith("t"))
    assert files == ["t_000.pfm", "t_001.pfm", "t_002.pfm"]
    assert open(tmp_path / "t_000.pfm", "rb").read() == open(tmp_path / "p.pfm", "rb").read()  # byte for byte

    def frames_of(scene, stem):
        blob = abi.build_scene(scene, w, h)
        gpu.upload_scene(blob)
        frames = gpu.views(bake.orbit_views(blob, 3, seed=seed), w, h, spp, depth)  # -seed applies to every view
        for k in range(3):
            raw = open(tmp_path / f"{stem}_{k:03d}.pfm", "rb").read()
            assert raw.startswith(b"PF\n") and len(raw) > w * h * 12
            body = np.frombuffer(raw[len(raw) - w * h * 12:], "<f4").reshape(h, w, 3)
            assert same(np.ascontiguousarray(body), np.ascontiguousarray(frames[k][..., :3])), (scene, k)
        return frames
    frames = frames_of(0, "t")
    assert V.lit_fraction(frames[0]) > 0.5
    assert not same(frames[0], gpu.views(bake.orbit_views(abi.build_scene(0, w, h), 1), w, h, spp, depth)[0])  # (the seed is not the default)
    # the Cornell box's frame stands ten units in front of a camera 800 units away from the box, so its turned views look past the
    # box; scene 1's stands among the spheres, under a sky: a turntable whose every frame shows the scene
    orbit1 = subprocess.run(base[:1] + ["-s", "1"] + base[3:] + ["-orbit", "3", "-o", str(tmp_path / "u.pfm")], capture_output=True, text=True, timeout=120)
    assert orbit1.returncode == 0, orbit1.stderr
    frames = frames_of(1, "u")
    assert min(V.lit_fraction(f) for f in frames) > 0.5
    assert not same(frames[0], frames[1]) and not same(frames[1], frames[2]) and not same(frames[0], frames[2])
    # refused before anything is rendered: no views, no file name to number, a flag the turntable does not combine with
    for bad in (["-orbit", "0", "-o", str(tmp_path / "x.pfm")], ["-orbit", "3"], ["-orbit", "2", "-denoise", "2", "-o", str(tmp_path / "x.pfm")]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "ERROR" in r.stderr
    assert not any(f.startswith("x") for f in os.listdir(tmp_path))
