"""GPU suite of the view guides (include/rtw.h rtw_views_guides / rtw_denoise_views and their device variants). The referees are the
contract itself and existing code: the guides of view v are rtw_render_guides' of the scene with views[v] in its header, frame v of
the denoiser is rtw_denoise_guided of frame v alone (view_guides_ref). Then the summation boundaries and offsets, independence of
the call's other views, chunks and requested buffers, the torch path, an identity that does not lean on k_guides, every refusal,
groups, sessions, the older entry points afterwards, and the command line."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import guides_ref
import oracle
import radiance_ref as R
import view_guides_ref as VG
import view_ref as V
from gpu_common import (BOTH, KNOBS, UPLOADS, check_golden_render, check_stream_order,  # noqa: F401
                        golden, gpu, left_alone, sentinel_stats, to_numpy, upload)
from raytracing_weekend_amd import abi, bake
from raytracing_weekend_amd.torch_views import denoise_views_torch, views_guides_torch, views_tensor

pytestmark = pytest.mark.gpu

ROOT = abi.REPO_DIR
same = VG.same


def all_same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), f"{k}: {int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words differ"
    return True


# ---------------------------------------------------------------- 1. every view's guides are rtw_render_guides' with that camera
@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", V.SCENES)
def test_every_views_guides_are_render_guides_of_the_scene_with_that_camera(gpu, monkeypatch, name, how, rng_kind):
    blob, views = R.scene(name), list(VG.cameras(name))
    upload(gpu, monkeypatch, blob, how)
    want = VG.referee_guides(gpu, blob, views, VG.W, VG.H, VG.SPP, rng_kind)
    hits = VG.hit_fractions(want["prim"])
    print(f"{name} {how} rng {rng_kind}: referee (hit fraction, distinct primitives) per view {hits}")
    # not empty guides: asserted on the referee's output, never on the code under test
    assert all(f >= VG.MIN_HIT and k >= 2 for f, k in hits), hits
    assert not same(want["albedo"][0], want["albedo"][1]) and not same(want["albedo"][1], want["albedo"][2])
    st = abi.Stats(shadow_rays=77, algorithmic_bytes=77)
    got = gpu.views_guides(views, VG.W, VG.H, VG.SPP, rng_kind=rng_kind, stats=st)
    assert got["albedo"].shape == (3, VG.H, VG.W, 4) and got["depth"].shape == (3, VG.H, VG.W) and got["prim"].dtype == np.int32
    assert all_same(got, want)
    assert st.samples == st.segments == 3 * VG.W * VG.H * VG.SPP and st.seconds > 0.0
    assert st.shadow_rays == 0 and st.algorithmic_bytes == 0 and not any(st.kernel_seconds) and not any(st.kernel_launches)
    assert np.array_equal(got["albedo"][..., 3], got["normal"][..., 3]) and np.all(np.isinf(got["depth"][got["prim"] < 0]))


# ---------------------------------------------------------------- 2. the summation boundaries and sample offsets
@pytest.mark.parametrize("spp", [1, 16, 17, 129, 272])
def test_odd_shapes_summation_units_and_sample_offsets(gpu, monkeypatch, spp):
    """Three views of 7 x 5: 35 pixels a frame, so the view boundaries fall inside a wave. One sample; one full block; a block and a
    one-sample tail; a unit and a one-sample unit; two units and a 16-sample tail. Offset 40 starts inside what would be a block of
    an offset-0 call; depth and prim then come from sample 40."""
    name = "random_volumes_motion"  # motion, media to skip, a view with times of its own
    blob, views = R.scene(name), list(VG.cameras(name))
    upload(gpu, monkeypatch, blob)
    for off, rng_kind in ((0, abi.RTW_RNG_PHILOX), (40, abi.RTW_RNG_TEA_LCG), (40, abi.RTW_RNG_PHILOX)):
        want = VG.referee_guides(gpu, blob, views, 7, 5, spp, rng_kind, sample_offset=off)
        assert max(f for f, _ in VG.hit_fractions(want["prim"])) >= 0.5
        got = gpu.views_guides(views, 7, 5, spp, rng_kind=rng_kind, sample_offset=off)
        assert got["albedo"].shape == (3, 5, 7, 4) and all_same(got, want)
    first = VG.referee_guides(gpu, blob, views, 7, 5, 1, sample_offset=40, which=("depth", "prim"))
    assert same(got["depth"], first["depth"]) and same(got["prim"], first["prim"])


# ---------------------------------------------------------------- 3. independence
def test_a_pixel_depends_on_its_view_its_place_and_the_params_alone(gpu, monkeypatch):
    name = "scene3"
    upload(gpu, monkeypatch, R.scene(name))
    a, b, c = VG.cameras(name)
    for spp in (16, 144):
        alone = gpu.views_guides([c], 7, 5, spp)
        assert (alone["prim"] >= 0).mean() > 0.5
        crowd = gpu.views_guides([a, b] * 20 + [c], 7, 5, spp)  # the same record as view 40 of 41
        assert crowd["albedo"].shape == (41, 5, 7, 4) and all_same({k: v[40:] for k, v in crowd.items()}, alone)
        assert all_same({k: v[:1] for k, v in crowd.items()}, gpu.views_guides([a], 7, 5, spp))
        assert all_same({k: v[39:40] for k, v in crowd.items()}, gpu.views_guides([b], 7, 5, spp))
        p = dict(rng_kind=abi.RTW_RNG_TEA_LCG, sample_offset=24)
        assert all_same({k: v[:1] for k, v in gpu.views_guides([c, a], 7, 5, spp, **p).items()}, gpu.views_guides([c], 7, 5, spp, **p))
    views = [a, b, c]
    want = gpu.views_guides(views, 7, 5, 16)
    # any subset of the four buffers: a NULL pointer does not change the others
    for r in range(1, 5):
        for which in itertools.combinations(abi.GUIDES, r):
            got = gpu.views_guides(views, 7, 5, 16, which=which)
            assert all_same(got, {k: want[k] for k in which})
    # chunks of 50 pixels begin and end mid-row and mid-view; chunks of one pixel
    for chunk in ("50", "1"):
        monkeypatch.setenv("RTW_RADIANCE_CHUNK", chunk)
        st = abi.Stats()
        assert all_same(gpu.views_guides(views, 7, 5, 16, stats=st), want)
        assert st.samples == st.segments == 3 * 35 * 16 and st.seconds > 0.0
        assert all_same(gpu.views_guides(views, 7, 5, 16, which=("normal", "prim")), {k: want[k] for k in ("normal", "prim")})
    monkeypatch.delenv("RTW_RADIANCE_CHUNK")
    assert all_same(gpu.views_guides(views, 7, 5, 16), want)


# ---------------------------------------------------------------- 4. the device path
def test_views_guides_torch_equals_views_guides_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    name = "random_volumes_motion"
    blob, views = R.scene(name), list(VG.cameras(name))
    upload(gpu, monkeypatch, blob)
    want = VG.referee_guides(gpu, blob, views, VG.W, VG.H, VG.SPP)
    d_views = views_tensor(views, "cuda:0")
    st = abi.Stats()
    torch.cuda.synchronize()
    got = views_guides_torch(gpu, d_views, VG.W, VG.H, VG.SPP, stats=st)
    assert all(t.is_cuda for t in got.values()) and got["prim"].dtype == torch.int32 and tuple(got["depth"].shape) == (3, VG.H, VG.W)
    assert all_same({k: t.cpu().numpy() for k, t in got.items()}, want)
    assert st.samples == st.segments == 3 * VG.W * VG.H * VG.SPP and st.seconds > 0.0 and st.shadow_rays == 0
    check_stream_order(lambda t: views_guides_torch(gpu, t, VG.W, VG.H, VG.SPP), d_views, lambda got: all_same(to_numpy(got), want),
                       default=(lambda t: views_guides_torch(gpu, t, VG.W, VG.H, VG.SPP, which=("albedo", "prim")),
                                lambda got: all_same(to_numpy(got), {k: want[k] for k in ("albedo", "prim")})))
    empty = views_guides_torch(gpu, torch.zeros((0, 28), device="cuda:0"), 4, 3, 4)
    assert tuple(empty["albedo"].shape) == (0, 3, 4, 4) and tuple(empty["prim"].shape) == (0, 3, 4)
    for kw in (dict(width=0), dict(height=-1), dict(spp=0), dict(which=()), dict(which=("beauty",))):
        args = dict(width=VG.W, height=VG.H, spp=VG.SPP)
        args.update(kw)
        with pytest.raises(ValueError):
            views_guides_torch(gpu, d_views, **args)


@pytest.mark.parametrize("rng_kind", BOTH)
def test_on_the_device_an_unknown_camera_type_is_a_perspective_camera(gpu, monkeypatch, rng_kind):
    """rtw_views_guides_device does not read the records back: a type of 7 or -1 gives type 0's guides, lens draws included (the
    TEA+LCG stream shows them), and the reserved words are ignored. rtw_views_guides, which can read them, refuses both."""
    name = "scene0"
    upload(gpu, monkeypatch, R.scene(name))
    a = VG.cameras(name)[0]
    want = gpu.views_guides([a], VG.W, VG.H, 32, rng_kind=rng_kind)
    assert (want["prim"] >= 0).mean() >= VG.MIN_HIT
    for camera_type in (7, -1):
        odd = abi.View.from_buffer_copy(bytes(a))
        odd.camera_type = camera_type
        odd.reserved[0], odd.reserved[1] = 5, 0xffffffff
        got = views_guides_torch(gpu, views_tensor([odd], "cuda:0"), VG.W, VG.H, 32, rng_kind=rng_kind)
        assert all_same({k: t.cpu().numpy() for k, t in got.items()}, want)
        with pytest.raises(RuntimeError):
            gpu.views_guides([odd], VG.W, VG.H, 32, rng_kind=rng_kind)


# ---------------------------------------------------------------- 5. an identity that does not lean on k_guides
def emitter_views(blob, w, h, seeds):
    out = []
    for (cam, lens), seed in zip(((0, 0.0), (0, 8.0), (100, 0.0), (200, 0.0)), seeds):
        out.append(abi.scene_view(guides_ref.with_camera(blob, cam, w, h, lens), seed))
    out[1].camera.time0, out[1].camera.time1 = 0.0, 1.0  # a view with times of its own
    return out


@pytest.mark.parametrize("seed,n_prims,motion", [(3, 20, False), (5, 48, True)])
@pytest.mark.parametrize("rng", BOTH)
def test_emitter_views_are_the_albedo_guides(gpu, monkeypatch, seed, n_prims, motion, rng):
    """All-emitter scene, textures in [0, 1], sky off: a 1-spp frame of rtw_views is Le for a front-face hit and 0 on a back face or
    a miss - what the albedo guide of rtw_views_guides holds for the same views, bit for bit (spp 1 and depth 5, as
    test_gpu_guides.py::test_emitter_beauty_is_the_albedo_guide takes them for one frame)."""
    w, h = 64, 48
    blob = guides_ref.all_emitters(oracle.random_scene(seed, w, h, n_prims=n_prims, motion=motion, textured=True))
    upload(gpu, monkeypatch, blob)
    views = emitter_views(blob, w, h, (11, 12, 13, 14))
    for off in (0, 37):
        frames = gpu.views(views, w, h, 1, 5, rng_kind=rng, sample_offset=off)
        g = gpu.views_guides(views, w, h, 1, which=("albedo", "prim"), rng_kind=rng, sample_offset=off)
        assert all((p >= 0).sum() > 20 for p in g["prim"])
        assert same(frames[..., :3], g["albedo"][..., :3])
        assert np.array_equal(g["albedo"][..., 3], (g["prim"] >= 0).astype(np.float32))


def test_emitters_that_encode_their_index_decode_to_the_prim_guide(gpu, monkeypatch):
    w, h = 80, 60
    blob = oracle.random_scene(21, w, h, n_prims=48, motion=True)
    n = len(abi.parse_scene(blob)["prims"])
    cols = [((i + 1) / 256.0, 0.5, 0.25) for i in range(n)]  # colour of primitive i, exact in float32
    blob = guides_ref.all_emitters(blob, cols)
    upload(gpu, monkeypatch, blob)
    views = emitter_views(blob, w, h, (1, 2, 3, 4))
    for off in (0, 113):
        frames = gpu.views(views, w, h, 1, 3, sample_offset=off)
        prim = gpu.views_guides(views, w, h, 1, which=("prim",), sample_offset=off)["prim"]
        lit = frames[..., 1] != 0
        assert lit[0].sum() > 100 and all(m.sum() > 20 for m in lit)  # (the orthographic view of the box sees a few primitives only)
        assert np.array_equal(np.rint(frames[..., 0][lit] * 256.0).astype(np.int32) - 1, prim[lit])
        assert np.all(prim[~lit] >= -1) and np.all(frames[..., :3][prim < 0] == 0)


# ---------------------------------------------------------------- 6. the denoiser
@pytest.fixture(scope="module")
def three_frames():
    return VG.distinct_frames(3, VG.H, VG.W)


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_denoise_views_is_denoise_guided_of_every_frame_alone(gpu, three_frames, iterations):
    """Three 24 x 16 frames of different content: a tap that reads a neighbouring view changes bits at the frame borders. At 5
    iterations the hole size of 16 exceeds the 16 rows: the smallest shape at which the per-frame clamp can go wrong."""
    frames, alb, nrm = three_frames
    want = VG.referee_denoise(gpu, frames, alb, nrm, iterations)
    stacked = gpu.denoise_guided(frames.reshape(-1, VG.W, 4), alb.reshape(-1, VG.W, 4), nrm.reshape(-1, VG.W, 4), iterations=iterations).reshape(frames.shape)
    assert not same(stacked, want)  # (one tall image is another filter: the comparison can tell)
    got = gpu.denoise_views(frames, alb, nrm, iterations=iterations)
    assert same(got, want) and np.array_equal(got[..., 3], frames[..., 3])
    sig = dict(sigma=0.3, sigma_albedo=0.2, sigma_normal=0.7)
    assert same(gpu.denoise_views(frames, alb, nrm, iterations=iterations, **sig), VG.referee_denoise(gpu, frames, alb, nrm, iterations, **sig))
    # the device entry, on a side stream and on the default stream
    d = [torch.from_numpy(x).to("cuda:0") for x in (frames, alb, nrm)]
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        late = [torch.zeros_like(t) for t in d]
        for t, s in zip(late, d):
            t.copy_(s, non_blocking=True)
        out = denoise_views_torch(gpu, *late, iterations=iterations)
    assert out.is_cuda and same(out.cpu().numpy(), want)
    torch.cuda.synchronize()
    assert same(denoise_views_torch(gpu, *d, iterations=iterations).cpu().numpy(), want)
    assert all(same(t.cpu().numpy(), x) for t, x in zip(d, (frames, alb, nrm)))  # the inputs are read only
    # one frame is rtw_denoise_guided itself; odd shapes; 41 frames
    assert same(gpu.denoise_views(frames[1:2], alb[1:2], nrm[1:2], iterations=iterations)[0], want[1])
    f, a, n = VG.distinct_frames(41, 5, 7, seed=9)
    assert same(gpu.denoise_views(f, a, n, iterations=iterations), VG.referee_denoise(gpu, f, a, n, iterations))


def test_with_constant_guides_denoise_views_is_denoise_of_every_frame(gpu, three_frames):
    frames = three_frames[0]
    flat = np.full_like(frames, 0.5)
    want = np.stack([gpu.denoise(f, iterations=4, sigma=0.5) for f in frames])
    assert same(gpu.denoise_views(frames, flat, flat, iterations=4, sigma=0.5), want)


def test_denoise_views_of_rendered_views_with_their_guides(gpu, monkeypatch):
    name = "scene0"
    blob, views = R.scene(name), list(VG.cameras(name))
    upload(gpu, monkeypatch, blob)
    frames = guides_ref.encode(gpu.views(views, VG.W, VG.H, 8, 6))
    g = gpu.views_guides(views, VG.W, VG.H, 8, which=("albedo", "normal"))
    want = VG.referee_denoise(gpu, frames, g["albedo"], g["normal"], 5)
    got = gpu.denoise_views(frames, g["albedo"], g["normal"])
    assert same(got, want) and not same(got, frames) and np.isfinite(got).all()


# ---------------------------------------------------------------- 7. refusals and side effects
def test_every_refusal_of_views_guides_leaves_the_context_usable_and_writes_nothing(gpu, monkeypatch):
    name = "scene0"
    blob = R.scene(name)
    upload(gpu, monkeypatch, blob)
    views = abi.view_array(VG.cameras(name))
    n, w, h, spp = 3, 7, 5, 16
    npix = n * h * w
    want = gpu.views_guides(views, w, h, spp)
    lib = gpu.lib
    host = {"albedo": np.full((npix, 4), -7, np.float32), "normal": np.full((npix, 4), -7, np.float32), "depth": np.full(npix, -7, np.float32),
            "prim": np.full(npix, -7, np.int32)}
    d_views = torch.cat([views_tensor(views, "cuda:0").ravel(), torch.zeros(8, device="cuda:0")])
    dev = {"albedo": torch.full((npix * 4 + 8,), -7.0, device="cuda:0"), "normal": torch.full((npix * 4 + 8,), -7.0, device="cuda:0"),
           "depth": torch.full((npix + 8,), -7.0, device="cuda:0"), "prim": torch.full((npix + 8,), -7, dtype=torch.int32, device="cuda:0")}
    V_, D_ = C.addressof(views), d_views.data_ptr()

    def guides(ptrs, **shift):
        return C.byref(abi.Guides(**{k: ptrs[k] + shift.get(k, 0) for k in ptrs}))
    H_ = {k: v.ctypes.data for k, v in host.items()}
    P_ = {k: v.data_ptr() for k, v in dev.items()}

    def vp(**kw):
        p = abi.make_view_params(w, h, spp, 6)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_views_guides(fresh.ctx, V_, n, vp(), guides(H_), None) == -3  # RTW_ERR_NO_SCENE
        assert lib.rtw_views_guides_device(fresh.ctx, D_, n, vp(), guides(P_), None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()

    def still_fine():
        assert all_same(gpu.views_guides(views, w, h, spp), want)
    bad_params = [None, vp(width=0), vp(width=-1), vp(height=0), vp(height=-5), vp(spp=0), vp(spp=-1), vp(max_depth=-1), vp(rng_kind=2), vp(rng_kind=-1),
                  vp(estimator=4), vp(estimator=-1), vp(sample_offset=-1), vp(sample_offset=2 ** 31 - spp), vp(spp=2 ** 31 - 1, sample_offset=1),
                  vp(reserved=1), vp(reserved=2 ** 31), vp(width=2 ** 16, height=2 ** 15), vp(width=2 ** 31 - 1, height=2 ** 31 - 1)]
    too_many = [(2 ** 31 - 1) // 35 + 1, 1 << 31, 1 << 40, 2 ** 64 - 1]
    no_buffer = C.byref(abi.Guides())
    refusals = ([(V_, n, p, guides(H_)) for p in bad_params] + [(V_, m, vp(), guides(H_)) for m in too_many] +
                [(None, n, vp(), guides(H_)), (V_, n, vp(), None), (V_, n, vp(), no_buffer)])
    for v_, m, p, g_ in refusals:
        st = sentinel_stats()
        assert lib.rtw_views_guides(gpu.ctx, v_, m, p, g_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    for field, value in (("camera_type", 3), ("camera_type", -1), ("camera_type", 7), ("reserved0", 1), ("reserved1", 2 ** 31)):
        bad = abi.view_array([abi.View.from_buffer_copy(bytes(v)) for v in views])
        if field == "camera_type":
            bad[2].camera_type = value
        else:
            bad[1].reserved[int(field[-1])] = value
        st = abi.Stats(segments=77, seconds=7.0)
        assert lib.rtw_views_guides(gpu.ctx, C.addressof(bad), n, vp(), guides(H_), C.byref(st)) == -1 and (st.segments, st.seconds) == (77, 7.0)
        assert b"view" in lib.rtw_last_error(gpu.ctx)
    still_fine()
    misaligned = [guides(P_, albedo=4), guides(P_, albedo=8), guides(P_, normal=4), guides(P_, normal=8), guides(P_, depth=1), guides(P_, depth=2),
                  guides(P_, prim=2), guides(P_, prim=3), guides({"depth": P_["depth"] + 1})]
    dev_refusals = ([(D_, n, p, guides(P_)) for p in bad_params] + [(D_, m, vp(), guides(P_)) for m in too_many] +
                    [(None, n, vp(), guides(P_)), (D_, n, vp(), None), (D_, n, vp(), no_buffer), (D_ + 4, n, vp(), guides(P_)), (D_ + 8, n, vp(), guides(P_))] +
                    [(D_, n, vp(), g_) for g_ in misaligned])
    for v_, m, p, g_ in dev_refusals:
        st = sentinel_stats()
        assert lib.rtw_views_guides_device(gpu.ctx, v_, m, p, g_, None, C.byref(st)) == -1
        assert left_alone(st)
    still_fine()
    torch.cuda.synchronize()
    assert all((v == -7).all() for v in host.values()) and all(bool((t == -7).all().item()) for t in dev.values())  # no refused call wrote anything
    # n_views = 0 is fine and launches nothing, whatever the pointers
    st = abi.Stats(segments=77)
    assert lib.rtw_views_guides(gpu.ctx, None, 0, vp(), guides(H_), C.byref(st)) == 0 and (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
    assert lib.rtw_views_guides(gpu.ctx, None, 0, vp(width=2 ** 31 - 1, height=2 ** 31 - 1), guides(H_), None) == 0
    assert lib.rtw_views_guides_device(gpu.ctx, None, 0, vp(), guides(P_), None, None) == 0
    assert lib.rtw_views_guides_device(gpu.ctx, D_ + 4, 0, vp(), guides(P_, albedo=4, depth=1), None, None) == 0
    empty = gpu.views_guides([], w, h, spp)
    assert empty["albedo"].shape == (0, h, w, 4) and empty["prim"].shape == (0, h, w)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all().item()) for t in dev.values())
    # from view 1 on, 16 (4) bytes into the buffers: aligned enough, and nothing is written beside the guides
    st = abi.Stats()
    assert lib.rtw_views_guides_device(gpu.ctx, D_ + 112, n - 1, vp(), guides(P_, albedo=16, normal=16, depth=4, prim=4), None, C.byref(st)) == 0
    assert st.samples == st.segments == (n - 1) * 35 * spp
    m = 35 * (n - 1)
    for k, width in (("albedo", 4), ("normal", 4), ("depth", 1), ("prim", 1)):
        t = dev[k]
        assert same(t[width:width + width * m].cpu().numpy().reshape(want[k][1:].shape), want[k][1:])
        assert bool((t[:width] == -7).all().item()) and bool((t[width + width * m:] == -7).all().item())


def test_every_refusal_of_denoise_views_writes_nothing(gpu, three_frames):
    frames, alb, nrm = three_frames
    n, h, w = frames.shape[:3]
    lib = gpu.lib
    want = gpu.denoise_views(frames, alb, nrm, iterations=2)
    out = np.full_like(frames, -7)
    I_, A_, N_, O_ = frames.ctypes.data, alb.ctypes.data, nrm.ctypes.data, out.ctypes.data
    d = [torch.cat([torch.from_numpy(x).to("cuda:0").ravel(), torch.zeros(8, device="cuda:0")]) for x in (frames, alb, nrm)]
    d_out = torch.full((frames.size + 8,), -7.0, device="cuda:0")
    DI_, DA_, DN_, DO_ = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_out.data_ptr()
    ok = dict(n=n, w=w, h=h, it=2, s=0.5, sa=0.4, sn=0.5)
    bad_args = [dict(w=0), dict(w=-1), dict(h=0), dict(h=-3), dict(it=0), dict(it=9), dict(it=-1), dict(s=0.0), dict(s=-1.0), dict(s=float("nan")),
                dict(sa=0.0), dict(sa=-0.5), dict(sa=1e-30), dict(sn=0.0), dict(sn=float("nan")), dict(sn=1e-30), dict(n=(2 ** 31 - 1) // (w * h) + 1),
                dict(n=1 << 40), dict(n=2 ** 64 - 1), dict(w=2 ** 16, h=2 ** 15), dict(n=1, w=2 ** 15, h=2 ** 14)]

    def host(i=I_, a=A_, nn=N_, o=O_, **kw):
        k = dict(ok, **kw)
        return lib.rtw_denoise_views(gpu.ctx, i, a, nn, o, k["n"], k["w"], k["h"], k["it"], k["s"], k["sa"], k["sn"])

    def device(i=DI_, a=DA_, nn=DN_, o=DO_, **kw):
        k = dict(ok, **kw)
        return lib.rtw_denoise_views_device(gpu.ctx, i, a, nn, o, k["n"], k["w"], k["h"], k["it"], k["s"], k["sa"], k["sn"], None)
    for kw in bad_args:
        assert host(**kw) == -1 and lib.rtw_last_error(gpu.ctx) and device(**kw) == -1, kw
    for kw in (dict(i=None), dict(a=None), dict(nn=None), dict(o=None), dict(o=I_), dict(o=A_), dict(o=N_), dict(o=I_ + 16), dict(i=O_ + 16 * (w * h))):
        assert host(**kw) == -1, kw
    for kw in (dict(i=None), dict(a=None), dict(nn=None), dict(o=None), dict(o=DI_), dict(o=DA_), dict(o=DN_), dict(o=DA_ + 16), dict(i=DI_ + 4),
               dict(a=DA_ + 8), dict(nn=DN_ + 4), dict(o=DO_ + 4), dict(o=DO_ + 8)):
        assert device(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == -7).all() and bool((d_out == -7).all().item())
    # n_views = 0 is fine, whatever the pointers
    assert host(n=0) == 0 and host(i=None, a=None, nn=None, o=None, n=0) == 0 and device(n=0) == 0 and device(i=None, o=DO_ + 4, n=0) == 0
    assert gpu.denoise_views(frames[:0], alb[:0], nrm[:0]).shape == (0, h, w, 4)
    torch.cuda.synchronize()
    assert (out == -7).all() and bool((d_out == -7).all().item())
    # the context stays usable; 16 bytes into the output is aligned enough, and nothing is written beside the frames
    assert device(o=DO_ + 16) == 0
    assert same(d_out[4:4 + frames.size].cpu().numpy().reshape(frames.shape), want)
    assert bool((d_out[:4] == -7).all().item()) and bool((d_out[4 + frames.size:] == -7).all().item())
    assert host() == 0 and same(out, want)
    # a context without a scene denoises as well
    fresh = abi.Renderer(0)
    try:
        assert same(fresh.denoise_views(frames, alb, nrm, iterations=2), want)
    finally:
        fresh.close()


def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch, three_frames):
    name = "scene1"
    blob = R.scene(name)
    upload(gpu, monkeypatch, blob)
    views = abi.view_array(VG.cameras(name))
    frames, alb, nrm = three_frames
    group = abi.Renderer([0, 0])  # a {0, 0} group
    try:
        out = np.zeros((3 * 5 * 7, 4), np.float32)
        p0 = abi.make_view_params(7, 5, 16, 6)
        g0 = abi.Guides(albedo=out.ctypes.data)
        assert group.lib.rtw_views_guides(group.ctx, C.addressof(views), 3, C.byref(p0), C.byref(g0), None) == -3 and not out.any()
        group.upload_scene(blob)
        for spp in (16, 144):
            want = gpu.views_guides(views, 7, 5, spp)
            assert (want["prim"][0] >= 0).mean() > 0.5
            assert all_same(group.views_guides(views, 7, 5, spp), want)
            got = views_guides_torch(group, views_tensor(views, "cuda:0"), 7, 5, spp)
            assert all_same({k: t.cpu().numpy() for k, t in got.items()}, want)
        want = gpu.denoise_views(frames, alb, nrm, iterations=3)
        assert same(group.denoise_views(frames, alb, nrm, iterations=3), want)
        d = [torch.from_numpy(x).to("cuda:0") for x in (frames, alb, nrm)]
        assert same(denoise_views_torch(group, *d, iterations=3).cpu().numpy(), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch, three_frames):
    name = "scene0"
    upload(gpu, monkeypatch, R.scene(name))
    views = list(VG.cameras(name))
    frames, alb, nrm = three_frames
    want = gpu.views_guides(views, 7, 5, 16)
    want_dn = gpu.denoise_views(frames, alb, nrm, iterations=3)
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        assert all_same(gpu.views_guides(views, 7, 5, 16), want)
        got = views_guides_torch(gpu, views_tensor(views, "cuda:0"), 7, 5, 16)
        assert all_same({k: t.cpu().numpy() for k, t in got.items()}, want)
        assert same(gpu.denoise_views(frames, alb, nrm, iterations=3), want_dn)
        gpu.views_guides(views, 7, 5, 144)
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    assert all_same(gpu.views_guides(views, 7, 5, 16), want)


def test_render_and_views_are_what_they_were_before_the_new_calls(gpu, monkeypatch, three_frames):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    frames, alb, nrm = three_frames
    gold = golden("cornell_200x200_16spp_d4_philox")
    blob, w, h, rng, seed = gold.blob, gold.w, gold.h, gold.rng, gold.seed
    gpu.upload_scene(blob)
    views = bake.orbit_views(blob, 3, seed=seed) + bake.cube_views((278, 278, 278))
    before = gpu.views(views, 16, 12, 24, 6, rng_kind=rng)
    guides_before = gpu.render_guides(abi.make_params(w, h, 4, 0, seed=seed))
    g = gpu.views_guides(views, 16, 12, 24, rng_kind=rng)
    gpu.views_guides(views, 16, 12, 160, which=("depth",))
    gpu.denoise_views(frames, alb, nrm)
    assert (g["prim"] >= 0).any() and np.isfinite(g["albedo"]).all()
    check_golden_render(gpu, gold)
    assert same(gpu.views(views, 16, 12, 24, 6, rng_kind=rng), before)
    assert all_same(gpu.render_guides(abi.make_params(w, h, 4, 0, seed=seed)), guides_before)


# ---------------------------------------------------------------- 8. the command line
def read_pfm(path, w, h, channels):
    raw = open(path, "rb").read()
    assert raw.startswith(b"PF\n" if channels == 3 else b"Pf\n") and len(raw) > w * h * 4 * channels
    body = np.frombuffer(raw[len(raw) - w * h * 4 * channels:], "<f4")
    return np.ascontiguousarray(body.reshape((h, w, 3) if channels == 3 else (h, w)))


def test_cli_orbit_writes_the_guides_and_the_denoised_frames_of_the_renderer(gpu, monkeypatch, tmp_path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cli = os.path.join(ROOT, "raytracing_weekend_amd", "host", "rtw_render")
    assert os.path.exists(cli), "build() has not produced the CLI"
    w, h, spp, depth, seed = 48, 32, 16, 6, 99
    base = [cli, "-s", "1", "-dx", str(w), "-dy", str(h), "-ns", str(spp), "-d", str(depth), "-seed", str(seed)]
    blob = abi.build_scene(1, w, h)
    gpu.upload_scene(blob)
    views = bake.orbit_views(blob, 3, seed=seed)  # -seed applies to every view
    frames = gpu.views(views, w, h, spp, depth)
    # -aov: the guides of -guide_spp samples, the frames untouched
    r = subprocess.run(base + ["-orbit", "3", "-aov", str(tmp_path / "g"), "-guide_spp", "8", "-o", str(tmp_path / "t.pfm")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == sorted([f"t_{k:03d}.pfm" for k in range(3)] + [f"g_{k:03d}_{n}.pfm" for k in range(3) for n in ("albedo", "normal", "depth")])
    want = gpu.views_guides(views, w, h, 8, which=("albedo", "normal", "depth"))
    assert min(float(np.isfinite(d).mean()) for d in want["depth"]) > 0.5  # every frame of this turntable shows the scene
    for k in range(3):
        assert same(read_pfm(tmp_path / f"t_{k:03d}.pfm", w, h, 3), frames[k][..., :3])
        assert same(read_pfm(tmp_path / f"g_{k:03d}_albedo.pfm", w, h, 3), want["albedo"][k][..., :3])
        assert same(read_pfm(tmp_path / f"g_{k:03d}_normal.pfm", w, h, 3), want["normal"][k][..., :3])
        assert same(read_pfm(tmp_path / f"g_{k:03d}_depth.pfm", w, h, 1), want["depth"][k])
    # -denoise K -guided: every view through rtw_denoise_views, display encoding in, linear values out; the guides of min(Ns, 16) samples
    r = subprocess.run(base + ["-orbit", "3", "-denoise", "3", "-guided", "-o", str(tmp_path / "d.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = gpu.views_guides(views, w, h, 16, which=("albedo", "normal"))
    filtered = gpu.denoise_views(guides_ref.encode(frames), g["albedo"], g["normal"], iterations=3)
    for k in range(3):
        got = read_pfm(tmp_path / f"d_{k:03d}.pfm", w, h, 3)
        assert same(got, filtered[k][..., :3] * filtered[k][..., :3]) and not same(got, frames[k][..., :3])
    # still refused before anything is rendered: the unguided denoiser does not combine with the turntable
    r = subprocess.run(base + ["-orbit", "2", "-denoise", "2", "-o", str(tmp_path / "x.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ERROR" in r.stderr and not any(f.startswith("x") for f in os.listdir(tmp_path))
