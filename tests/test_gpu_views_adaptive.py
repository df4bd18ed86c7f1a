"""GPU suite of the adaptive views (include/rtw.h rtw_views_adaptive / rtw_views_adaptive_device). The referee is the contract
itself: the three outputs of view v are rtw_render_adaptive's for the scene with views[v]'s camera in its header, in bits, stats
summed. Then every pixel against rtw_views at its own count and the decisions against view_adaptive_ref.reference, odd shapes and
schedules, the threshold's extremes, independence of the call's other views, batches and slab ranges, the torch path, every refusal,
groups, sessions, the older entry points afterwards, and the command-line turntable.

The threshold of the main cases is the rehearsal's (tests/test_views_adaptive_cpu.py): the median of the positive finite errors at
32 spp over the three views, here taken from the call itself with threshold +inf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import probe_ref as P
import radiance_ref as R
import view_adaptive_ref as VA
import view_ref as V
from gpu_common import (BOTH, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render, check_stream_order,  # noqa: F401
                        golden, gpu, left_alone, same3, same_words as same, sentinel_stats, upload)
from raytracing_weekend_amd import abi, bake
from raytracing_weekend_amd.torch_views import views_adaptive_torch, views_tensor

pytestmark = pytest.mark.gpu

ROOT = abi.REPO_DIR
W, H, CAP, MIN_SPP, DEPTH = 24, 16, 256, 32, 8  # the rehearsed inputs


def describe(got, want):
    bad = np.argwhere((got[1] != want[1]) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(-1) | (got[2].view(np.uint32) != want[2].view(np.uint32)))
    if not len(bad):
        return ""
    i = tuple(bad[0])
    return f"{len(bad)} pixels differ, first (view, y, x) = {i}: n {got[1][i]} != {want[1][i]}, err {got[2][i]!r} != {want[2][i]!r}, {got[0][i]} != {want[0][i]}"


def median_threshold(gpu, views, w, h, depth, min_spp=MIN_SPP, **kw):
    """the median of the positive finite errors at min_spp over the call's pixels (threshold +inf: everything stops there)"""
    _, n, err = gpu.views_adaptive(views, w, h, max(min_spp, 64), depth, np.inf, min_spp=min_spp, dilate=0, **kw)
    assert (n[np.isfinite(err)] == min_spp).all()
    e = err[np.isfinite(err) & (err > 0)]
    return float(np.float32(np.median(e.astype(np.float64))))


def per_view(gpu, blob, views, w, h, cap, depth, threshold, min_spp, step_spp, dilate, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0):
    """The contract: rtw_render_adaptive of the scene with each view's camera in its header; ((frames, spp, err), samples, segments,
    shadow rays). It uploads: the caller uploads `blob` again afterwards."""
    out = (np.empty((len(views), h, w, 4), np.float32), np.empty((len(views), h, w), np.int32), np.empty((len(views), h, w), np.float32))
    tot = [0, 0, 0]
    for i, v in enumerate(views):
        gpu.upload_scene(V.view_blob(blob, v))
        p = abi.make_params(w, h, cap, depth, seed=v.seed, rng_kind=rng_kind, sample_offset=sample_offset, estimator=estimator)
        out[0][i], out[1][i], out[2][i], st = gpu.render_adaptive(p, threshold, min_spp=min_spp, step_spp=step_spp, dilate=dilate)
        tot = [tot[0] + st.samples, tot[1] + st.segments, tot[2] + st.shadow_rays]
    return out, tuple(tot)


# ---------------------------------------------------------------- 1. every view is rtw_render_adaptive of the scene with that camera
def check_equivalence(gpu, name, rng_kind, estimator=0):
    blob, views = R.scene(name), list(V.cameras(name))
    kw = dict(rng_kind=rng_kind, estimator=estimator)
    T = median_threshold(gpu, views, W, H, DEPTH, **kw)
    for dilate in (0, 1):
        st = abi.Stats()
        got = gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP, dilate=dilate, stats=st, **kw)
        want, tot = per_view(gpu, blob, views, W, H, CAP, DEPTH, T, MIN_SPP, 0, dilate, **kw)
        gpu.upload_scene(blob)
        print(f"{name} rng {rng_kind} estimator {estimator} dilate {dilate} T {T:.6g}: n_p {[VA.histogram(n) for n in got[1]]}, "
              f"samples {st.samples}, segments {st.segments} (renders {tot[1]}), shadow rays {st.shadow_rays} ({tot[2]})")
        assert got[0].shape == (3, H, W, 4) and got[1].shape == (3, H, W) and got[2].shape == (3, H, W)
        assert same3(got, want), describe(got, want)
        assert (st.samples, st.segments, st.shadow_rays) == tot and st.samples == int(got[1].astype(np.int64).sum())
        assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
        assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
        assert (got[0][..., 3] == 1.0).all() and set(np.unique(got[1])) <= {32, 48, 80, 128, 192, 256}
        assert len(np.unique(got[1])) >= 2  # (not one count for the whole call)


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", V.SCENES)
def test_every_view_is_render_adaptive_of_the_scene_with_that_camera(gpu, monkeypatch, name, how, rng_kind):
    upload(gpu, monkeypatch, R.scene(name), how)
    check_equivalence(gpu, name, rng_kind)


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("estimator", [1, 2, 3])
def test_under_the_corrected_estimators_on_scene_0(gpu, monkeypatch, estimator, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    check_equivalence(gpu, "scene0", rng_kind, estimator)


# ---------------------------------------------------------------- 2. every pixel is rtw_views at its own count; the decisions
def blocks_of(gpu, views, w, h, cap, depth, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0):
    """S[b, v, y, x, 3] from 16-spp rtw_views calls at sample offsets 16 b (mean x 16 is exact)"""
    S = np.empty((cap // 16, len(views), h, w, 3), np.float32)
    for b in range(cap // 16):
        S[b] = gpu.views(views, w, h, 16, depth, rng_kind=rng_kind, sample_offset=sample_offset + 16 * b)[..., :3] * np.float32(16)
    return S


def check_pixels_equal_views_at_their_count(gpu, views, got, w, h, depth, **kw):
    for n in np.unique(got[1]):
        m = got[1] == n
        frames = gpu.views(views, w, h, int(n), depth, **kw)
        assert same(got[0][m], frames[m]), (int(n), int(m.sum()))


@pytest.mark.parametrize("rng_kind", BOTH)
def test_every_pixel_equals_views_at_its_count_and_the_decisions_are_the_referees(gpu, monkeypatch, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    views = list(V.cameras("scene0"))
    T = median_threshold(gpu, views, W, H, DEPTH, rng_kind=rng_kind)
    S = blocks_of(gpu, views, W, H, CAP, DEPTH, rng_kind)
    tie = VA.near_ties(S, T, MIN_SPP, 0, CAP)
    assert tie.mean() <= 0.02
    for dilate in (0, 1):
        got = gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP, dilate=dilate, rng_kind=rng_kind)
        check_pixels_equal_views_at_their_count(gpu, views, got, W, H, DEPTH, rng_kind=rng_kind)
        rimg, rn, rerr = VA.reference(S, T, MIN_SPP, 0, CAP, dilate)
        ok = ~(VA.spread(tie) if dilate else tie)
        print(f"rng {rng_kind} dilate {dilate}: n_p {[VA.histogram(n) for n in got[1]]}; {int((~ok).sum())} pixels excluded as ties")
        assert np.array_equal(got[1][ok], rn[ok]), int(np.count_nonzero(got[1][ok] != rn[ok]))
        assert same(got[0][ok], rimg[ok]) and same(got[2][ok], rerr[ok])
        for v in range(3):
            assert len(VA.histogram(got[1][v])) >= 2, (dilate, v)
    assert np.count_nonzero(gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP, dilate=0, rng_kind=rng_kind)[1] != got[1]) >= 1


# ---------------------------------------------------------------- 3. shapes, schedules, extremes
@pytest.mark.parametrize("sample_offset", [0, 16])
def test_three_views_of_7x5_under_a_schedule_that_crosses_a_unit(gpu, monkeypatch, sample_offset):
    """35 pixels a view: a decision wave spans two views, and neither the width nor the frame is a power of two. Checkpoints
    32 80 128 176 224 272: the passes end on, and cross, the 128-sample unit; 272 = two units and a 16-sample tail."""
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    views = list(V.cameras("scene0"))
    w, h, cap, step, depth = 7, 5, 272, 48, 6
    for rng_kind in BOTH:
        kw = dict(rng_kind=rng_kind, sample_offset=sample_offset)
        T = median_threshold(gpu, views, w, h, depth, **kw)
        for dilate in (0, 1):
            st = abi.Stats()
            got = gpu.views_adaptive(views, w, h, cap, depth, T, min_spp=32, step_spp=step, dilate=dilate, stats=st, **kw)
            want, tot = per_view(gpu, blob, views, w, h, cap, depth, T, 32, step, dilate, **kw)
            gpu.upload_scene(blob)
            print(f"7x5 offset {sample_offset} rng {rng_kind} dilate {dilate}: {VA.histogram(got[1])}")
            assert same3(got, want), describe(got, want)
            assert (st.samples, st.segments, st.shadow_rays) == tot
            assert set(np.unique(got[1])) <= {32, 80, 128, 176, 224, 272} and len(np.unique(got[1])) >= 2
            check_pixels_equal_views_at_their_count(gpu, views, got, w, h, depth, **kw)


def test_single_pixel_and_single_column_views(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    views = list(V.cameras("scene0"))
    for w, h, vs in ((1, 1, views[:1]), (1, 1, views), (1, 9, views[:1]), (9, 1, views[1:]), (1, 9, views)):
        for dilate in (0, 1):
            T = median_threshold(gpu, vs, w, h, DEPTH)
            got = gpu.views_adaptive(vs, w, h, 128, DEPTH, T, min_spp=32, dilate=dilate)
            want, _ = per_view(gpu, blob, vs, w, h, 128, DEPTH, T, 32, 0, dilate)
            gpu.upload_scene(blob)
            assert got[0].shape == (len(vs), h, w, 4) and same3(got, want), (w, h, len(vs), dilate, describe(got, want))


def test_threshold_extremes_and_depth_zero(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    views = list(V.cameras("scene0"))
    for dilate in (0, 1):
        # threshold 0: nothing stops early; the frames are rtw_views' at the cap
        st = abi.Stats()
        img, n, err = gpu.views_adaptive(views, W, H, CAP, DEPTH, 0.0, min_spp=MIN_SPP, dilate=dilate, stats=st)
        s0 = abi.Stats()
        assert (n == CAP).all() and same(img, gpu.views(views, W, H, CAP, DEPTH, stats=s0))
        assert (st.samples, st.segments, st.shadow_rays) == (s0.samples, s0.segments, s0.shadow_rays)
        # threshold +inf: everything with a finite err stops at min_spp
        img, n, err = gpu.views_adaptive(views, W, H, CAP, DEPTH, np.inf, min_spp=MIN_SPP, dilate=dilate)
        assert np.isfinite(err).all() and (n == MIN_SPP).all() and same(img, gpu.views(views, W, H, MIN_SPP, DEPTH))
        # max_depth 0: no segment, black frames, err 0
        st = abi.Stats()
        img, n, err = gpu.views_adaptive(views, W, H, CAP, 0, 0.02, min_spp=MIN_SPP, dilate=dilate, stats=st)
        assert not img[..., :3].any() and (img[..., 3] == 1.0).all() and (n == MIN_SPP).all() and not err.any()
        assert (st.samples, st.segments, st.shadow_rays) == (3 * W * H * MIN_SPP, 0, 0)
        img, n, err = gpu.views_adaptive(views, W, H, 64, 0, 0.0, min_spp=MIN_SPP, dilate=dilate)
        assert not img[..., :3].any() and (n == 64).all() and not err.any()


# ---------------------------------------------------------------- 4. independence
def away_view(seed=7):
    """an orthographic view in front of the Cornell box that looks away from it: every sample leaves at once, black frames, err 0"""
    return abi.make_view(V.orthographic_camera((139, 139, -400), (139, 139, -401), (0, 1, 0), 540.0, 540.0), abi.RTW_CAM_ORTHOGRAPHIC, seed)


def test_a_view_does_not_depend_on_the_views_around_it(gpu, monkeypatch):
    """The same record alone and as the 40th of 41 views under dilate = 1, between a view of seed 1 (noisy: other samples) and a view
    that sees nothing (all of it stops at min_spp): neither may move one of its pixels."""
    upload(gpu, monkeypatch, R.scene("scene0"))
    a, b, c = V.cameras("scene0")
    T = median_threshold(gpu, [a, b, c], W, H, DEPTH)
    for me in (a, b, c):
        alone = gpu.views_adaptive([me], W, H, CAP, DEPTH, T, min_spp=MIN_SPP, dilate=1)
        before = abi.make_view(a.camera, a.camera_type, 1)
        crowd = [a, b, c] * 13 + [me, away_view()]
        crowd[38] = before
        assert len(crowd) == 41
        big = gpu.views_adaptive(crowd, W, H, CAP, DEPTH, T, min_spp=MIN_SPP, dilate=1)
        assert same3(tuple(x[39:40] for x in big), alone), describe(tuple(x[39:40] for x in big), alone)
        assert not big[0][40][..., :3].any() and (big[1][40] == MIN_SPP).all() and not big[2][40].any()
        assert len(np.unique(alone[1])) >= 2 and not same(big[0][38], big[0][0])
        # and in another order: the view first, the black one before the noisy one
        other = gpu.views_adaptive([me, away_view(), before], W, H, CAP, DEPTH, T, min_spp=MIN_SPP, dilate=1)
        assert same3(tuple(x[0:1] for x in other), alone) and same3(tuple(x[2:3] for x in other), tuple(x[38:39] for x in big))


def test_batches_slab_ranges_and_lds_change_no_bit(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    views = list(V.cameras("scene0")) * 2 + [away_view()]
    w, h, cap, depth = 7, 5, 128, 6
    T = median_threshold(gpu, views, w, h, depth)
    d_views = views_tensor(views, "cuda:0")
    for dilate in (0, 1):
        s0 = abi.Stats()
        whole = gpu.views_adaptive(views, w, h, cap, depth, T, min_spp=32, dilate=dilate, stats=s0)
        assert len(np.unique(whole[1])) >= 2
        variants = ({"RTW_RADIANCE_CHUNK": "50"},  # one view (35 pixels) per batch
                    {"RTW_RADIANCE_CHUNK": "1"},   # below a frame: still one whole view per batch
                    {"RTW_RADIANCE_CHUNK": "80"},  # two views per batch, the last batch one view
                    {"RTW_RADIANCE_SLAB_BYTES": str(40 * 2 * 16)},  # 40 positions of the first pass's two blocks: ranges that end inside a view
                    {"RTW_RADIANCE_CHUNK": "80", "RTW_RADIANCE_SLAB_BYTES": "16"})  # one list position per range
        for env in variants:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            s1 = abi.Stats()
            got = gpu.views_adaptive(views, w, h, cap, depth, T, min_spp=32, dilate=dilate, stats=s1)
            assert same3(got, whole), (env, describe(got, whole))
            assert (s1.samples, s1.segments, s1.shadow_rays) == (s0.samples, s0.segments, s0.shadow_rays)
            if "RTW_RADIANCE_CHUNK" not in env:
                t = views_adaptive_torch(gpu, d_views, w, h, cap, depth, T, min_spp=32, dilate=dilate)
                assert same3(tuple(x.cpu().numpy() for x in t), whole), env
            for k in env:
                monkeypatch.delenv(k)
    for lds in ("0", "48"):  # read at upload
        monkeypatch.setenv("RTW_LDS_KB", lds)
        monkeypatch.setenv("RTW_BRUTE_MAX", "0")
        gpu.upload_scene(blob)
        assert same3(gpu.views_adaptive(views, w, h, cap, depth, T, min_spp=32, dilate=1), whole), lds
    upload(gpu, monkeypatch, blob)


# ---------------------------------------------------------------- 5. the device path
def test_views_adaptive_torch_equals_the_host_path_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    views = list(V.cameras("scene0"))
    T = median_threshold(gpu, views, W, H, DEPTH)
    d_views = views_tensor(views, "cuda:0")
    kw = dict(min_spp=MIN_SPP, dilate=1)
    s0, st = abi.Stats(), abi.Stats()
    want = gpu.views_adaptive(views, W, H, CAP, DEPTH, T, stats=s0, **kw)
    got = views_adaptive_torch(gpu, d_views, W, H, CAP, DEPTH, T, stats=st, **kw)
    assert all(t.is_cuda for t in got) and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    assert tuple(got[0].shape) == (3, H, W, 4) and tuple(got[1].shape) == (3, H, W) and tuple(got[2].shape) == (3, H, W)
    assert same3(tuple(t.cpu().numpy() for t in got), want)
    assert (st.segments, st.shadow_rays, st.samples) == (s0.segments, s0.shadow_rays, s0.samples) and st.seconds > 0.0
    check_stream_order(lambda t: views_adaptive_torch(gpu, t, W, H, CAP, DEPTH, T, **kw), d_views,
                       lambda got: same3(tuple(t.cpu().numpy() for t in got), want))
    empty = views_adaptive_torch(gpu, torch.zeros((0, 28), device="cuda:0"), 8, 4, 64, 4, T)
    assert [tuple(t.shape) for t in empty] == [(0, 4, 8, 4), (0, 4, 8), (0, 4, 8)]
    with pytest.raises(ValueError):
        views_adaptive_torch(gpu, d_views, W, H, 0, DEPTH, T)


# ---------------------------------------------------------------- 6. refusals
def test_every_refusal_leaves_the_context_usable_and_writes_nothing(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    views = list(V.cameras("scene0"))
    arr = abi.view_array(views)
    T = 0.02
    want = gpu.views_adaptive(views, 8, 4, 64, DEPTH, T, min_spp=MIN_SPP)
    lib, n, npix = gpu.lib, 3, 3 * 8 * 4
    out, spp, err = np.full((npix, 4), -7, np.float32), np.full(npix, -7, np.int32), np.full(npix, -7, np.float32)
    d_views = torch.cat([views_tensor(views, "cuda:0").reshape(-1), torch.zeros(28, device="cuda:0")])
    d_out = torch.full((npix * 4 + 8,), -7.0, device="cuda:0")
    d_spp = torch.full((npix + 8,), -7, dtype=torch.int32, device="cuda:0")
    d_err = torch.full((npix + 8,), -7.0, device="cuda:0")
    V_, O_, S_, E_ = C.cast(arr, C.c_void_p), out.ctypes.data, spp.ctypes.data, err.ctypes.data
    D_, DO_, DS_, DE_ = d_views.data_ptr(), d_out.data_ptr(), d_spp.data_ptr(), d_err.data_ptr()

    def vp(**kw):
        p = abi.make_view_params(8, 4, 64, DEPTH)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def ad(min_spp=MIN_SPP, step_spp=0, threshold=T, dilate=1):
        return C.byref(abi.Adaptive(min_spp, step_spp, threshold, dilate))
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_views_adaptive(fresh.ctx, V_, n, vp(), ad(), O_, S_, E_, None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_views_adaptive_device(fresh.ctx, D_, n, vp(), ad(), DO_, DS_, DE_, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()

    def still_fine():
        assert same3(gpu.views_adaptive(views, 8, 4, 64, DEPTH, T, min_spp=MIN_SPP), want)
    # rtw_views' refusals, then the adaptive ones: the cap (params->spp), min_spp, step_spp, the threshold, dilate, a NULL ad
    bad = [(None, ad()), (vp(width=0), ad()), (vp(height=-4), ad()), (vp(spp=0), ad()), (vp(spp=-16), ad()), (vp(max_depth=-1), ad()),
           (vp(rng_kind=2), ad()), (vp(rng_kind=-1), ad()), (vp(estimator=4), ad()), (vp(estimator=-1), ad()), (vp(sample_offset=-1), ad()),
           (vp(sample_offset=2 ** 31 - 64), ad()), (vp(reserved=1), ad()),
           (vp(), None), (vp(spp=72), ad()), (vp(spp=16), ad(16)), (vp(), ad(16)), (vp(), ad(40)), (vp(), ad(80)), (vp(), ad(0)),
           (vp(), ad(step_spp=-16)), (vp(), ad(step_spp=8)), (vp(), ad(threshold=-0.5)), (vp(), ad(threshold=float("nan"))),
           (vp(), ad(dilate=2)), (vp(), ad(dilate=-1))]
    host = [(V_, n, p, a, O_) for p, a in bad] + [(V_, 1 << 31, vp(), ad(), O_), (V_, 1 << 26, vp(), ad(), O_), (None, n, vp(), ad(), O_),
                                                  (V_, n, vp(), ad(), None)]
    for v_, m, p, a, o_ in host:
        st = sentinel_stats()
        assert lib.rtw_views_adaptive(gpu.ctx, v_, m, p, a, o_, S_, E_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    # the host entry reads the records
    for field, value in (("camera_type", 3), ("camera_type", -1), ("reserved", (C.c_uint32 * 2)(0, 1))):
        rec = abi.view_array([abi.make_view(v.camera, v.camera_type, v.seed) for v in views])
        setattr(rec[1], field, value)
        st = abi.Stats(segments=77)
        assert lib.rtw_views_adaptive(gpu.ctx, C.cast(rec, C.c_void_p), n, vp(), ad(), O_, S_, E_, C.byref(st)) == -1 and st.segments == 77
    still_fine()
    dev = [(D_, n, p, a, DO_, DS_, DE_) for p, a in bad] + [
        (D_, 1 << 31, vp(), ad(), DO_, DS_, DE_), (None, n, vp(), ad(), DO_, DS_, DE_), (D_, n, vp(), ad(), None, DS_, DE_),
        (D_ + 4, n, vp(), ad(), DO_, DS_, DE_), (D_ + 8, n, vp(), ad(), DO_, DS_, DE_), (D_, n, vp(), ad(), DO_ + 4, DS_, DE_),
        (D_, n, vp(), ad(), DO_ + 8, DS_, DE_), (D_, n, vp(), ad(), DO_, DS_ + 2, DE_), (D_, n, vp(), ad(), DO_, DS_, DE_ + 1),
        (D_, n, vp(), ad(), DO_, DS_ + 1, None)]
    for v_, m, p, a, o_, s_, e_ in dev:
        st = sentinel_stats()
        assert lib.rtw_views_adaptive_device(gpu.ctx, v_, m, p, a, o_, s_, e_, None, C.byref(st)) == -1
        assert left_alone(st)
    still_fine()  # after a misaligned pointer as after any other refusal: the next call works
    torch.cuda.synchronize()
    assert (out == -7).all() and (spp == -7).all() and (err == -7).all()  # no refused call wrote anything
    assert bool((d_out == -7).all().item()) and bool((d_spp == -7).all().item()) and bool((d_err == -7).all().item())
    # n_views = 0 is fine and launches nothing, whatever the pointers
    st = abi.Stats(segments=77)
    assert lib.rtw_views_adaptive(gpu.ctx, None, 0, vp(), ad(), None, None, None, C.byref(st)) == 0
    assert (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
    assert lib.rtw_views_adaptive_device(gpu.ctx, None, 0, vp(), ad(), None, None, None, None, None) == 0
    assert lib.rtw_views_adaptive_device(gpu.ctx, D_ + 4, 0, vp(), ad(), DO_ + 4, DS_ + 1, DE_ + 1, None, None) == 0
    empty = gpu.views_adaptive([], 8, 4, 64, 4, T)
    assert [a.shape for a in empty] == [(0, 4, 8, 4), (0, 4, 8), (0, 4, 8)]
    # spp_out and error_out may be NULL; from view 1 on the pointers are aligned enough
    assert lib.rtw_views_adaptive(gpu.ctx, V_, n, vp(), ad(), O_, None, None, None) == 0
    assert same(out.reshape(3, 4, 8, 4), want[0]) and (spp == -7).all() and (err == -7).all()
    assert lib.rtw_views_adaptive_device(gpu.ctx, D_ + 112, n - 1, vp(), ad(), DO_ + 16, DS_ + 4, None, None, None) == 0
    assert same(d_out[4:4 + 4 * 64].cpu().numpy().reshape(2, 4, 8, 4), want[0][1:]) and np.array_equal(d_spp[1:65].cpu().numpy().reshape(2, 4, 8), want[1][1:])
    assert bool((d_err == -7).all().item())


# ---------------------------------------------------------------- 7. neighbours
def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    views = list(V.cameras("scene0"))
    T = median_threshold(gpu, views, W, H, DEPTH)
    group = abi.Renderer([0, 0])
    try:
        with pytest.raises(RuntimeError):
            group.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP)  # no scene yet
        group.upload_scene(blob)
        s0, s1 = abi.Stats(), abi.Stats()
        want = gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP, stats=s0)
        assert same3(group.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP, stats=s1), want)
        assert (s1.samples, s1.segments, s1.shadow_rays) == (s0.samples, s0.segments, s0.shadow_rays)
        got = views_adaptive_torch(group, views_tensor(views, "cuda:0"), W, H, CAP, DEPTH, T, min_spp=MIN_SPP)
        assert same3(tuple(t.cpu().numpy() for t in got), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    views = list(V.cameras("scene0"))
    T = median_threshold(gpu, views, W, H, DEPTH)
    want = gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP)
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        assert same3(gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP), want)
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    assert same3(gpu.views_adaptive(views, W, H, CAP, DEPTH, T, min_spp=MIN_SPP), want)


def test_views_probe_adaptive_and_render_are_what_they_were_before_adaptive_views(gpu, monkeypatch):
    """The slab, the staging and the per-entry state are shared: the older entry points before and after adaptive view calls."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for g in map(golden, GOLDEN_PAIR):
        blob, rng, seed = g.blob, g.rng, g.seed
        gpu.upload_scene(blob)
        views = bake.orbit_views(blob, 2, seed=seed)
        probes = P.scene_probes(gpu.cast, blob, 300, tmax=100.0)
        frames = gpu.views(views, 20, 12, 160, 4, rng_kind=rng)
        pa = gpu.probe_adaptive(probes, 192, 4, 0.02, min_spp=32, rng_kind=rng)
        for dilate in (0, 1):
            out, n_p, err = gpu.views_adaptive(views, 20, 12, 192, 4, 0.02, min_spp=32, dilate=dilate, rng_kind=rng)
            assert np.isfinite(out).all() and set(np.unique(n_p)) <= {32, 48, 80, 128, 192} and (err >= 0).all()
        check_golden_render(gpu, g)
        assert same(gpu.views(views, 20, 12, 160, 4, rng_kind=rng), frames)
        got = gpu.probe_adaptive(probes, 192, 4, 0.02, min_spp=32, rng_kind=rng)
        assert same(got[0], pa[0]) and np.array_equal(got[1], pa[1]) and same(got[2], pa[2])


# ---------------------------------------------------------------- 8. the command line
def test_cli_orbit_adaptive_writes_what_renderer_views_adaptive_returns(gpu, monkeypatch, tmp_path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    cli = os.path.join(ROOT, "raytracing_weekend_amd", "host", "rtw_render")
    assert os.path.exists(cli), "build() has not produced the CLI"
    w, h, cap, T = 48, 32, 256, float(np.float32(0.02))
    r = subprocess.run([cli, "-s", "1", "-dx", str(w), "-dy", str(h), "-ns", str(cap), "-orbit", "3", "-adaptive", repr(T), "-aov", str(tmp_path / "P"),
                        "-o", str(tmp_path / "t.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blob = abi.build_scene(1, w, h)
    gpu.upload_scene(blob)
    # the CLI's defaults: depth 20, min_spp 64, the default schedule, dilate 1, the default seed for every view
    frames, n_p, err = gpu.views_adaptive(bake.orbit_views(blob, 3), w, h, cap, 20, T, min_spp=64, dilate=1)
    assert len(np.unique(n_p)) >= 2

    def tail(path, floats):
        raw = open(path, "rb").read()
        return np.frombuffer(raw[len(raw) - 4 * floats:], "<f4")
    for k in range(3):
        assert same(tail(tmp_path / f"t_{k:03d}.pfm", w * h * 3).reshape(h, w, 3), np.ascontiguousarray(frames[k][..., :3])), k
        assert open(tmp_path / f"P_{k:03d}_spp.pfm", "rb").read().startswith(b"Pf\n")
        assert same(tail(tmp_path / f"P_{k:03d}_spp.pfm", w * h).reshape(h, w), n_p[k].astype(np.float32)), k
        assert same(tail(tmp_path / f"P_{k:03d}_error.pfm", w * h).reshape(h, w), err[k]), k
        for g in ("albedo", "normal", "depth"):
            assert os.path.exists(tmp_path / f"P_{k:03d}_{g}.pfm")
    # with the guided denoiser the adaptive frames are the ones that are filtered
    d = subprocess.run([cli, "-s", "1", "-dx", str(w), "-dy", str(h), "-ns", str(cap), "-orbit", "2", "-adaptive", repr(T), "-denoise", "2", "-guided",
                        "-o", str(tmp_path / "d.pfm")], capture_output=True, text=True, timeout=120)
    assert d.returncode == 0, d.stderr
    views = bake.orbit_views(blob, 2)
    frames = gpu.views_adaptive(views, w, h, cap, 20, T, min_spp=64, dilate=1)[0]
    guides = gpu.views_guides(views, w, h, 16, which=("albedo", "normal"))
    enc = frames.copy()
    rgb = enc[..., :3]
    rgb[~(rgb == rgb) | (rgb < 0)] = 0
    enc[..., :3] = np.sqrt(np.minimum(rgb, np.float32(1)))
    flt = gpu.denoise_views(enc, guides["albedo"], guides["normal"], iterations=2, sigma=0.5)
    for k in range(2):
        assert same(tail(tmp_path / f"d_{k:03d}.pfm", w * h * 3).reshape(h, w, 3), np.ascontiguousarray(flt[k][..., :3] * flt[k][..., :3])), k
