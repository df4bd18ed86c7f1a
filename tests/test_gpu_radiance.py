"""GPU suite of the radiance queries (include/rtw.h rtw_radiance / rtw_radiance_device): every pixel and both counts against the
oracle's bits (radiance_ref.py: the ray as the camera of a one-pixel render), the summation order and sample offsets, independence
of the batch, the chunking and the slab, keys that wrap, the first segment's interval, the torch path, every refusal, groups,
sessions and rtw_render afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import geometry_ref as G
import radiance_ref as R
import gpu_common
from gpu_common import (BOTH, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render, check_stream_order, golden, gpu, left_alone, same,  # noqa: F401
                        sentinel_stats, upload)
from raytracing_weekend_amd import abi
from raytracing_weekend_amd.torch_radiance import radiance_torch

pytestmark = pytest.mark.gpu
first_difference = functools.partial(gpu_common.first_difference, what="rays")


# ---------------------------------------------------------------- 1. the oracle's bits
def check_case(gpu, name, rng_kind, estimator=0):
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind, estimator)
    st = abi.Stats()
    got = gpu.radiance(rays, R.SPP, R.DEPTH, rng_kind=rng_kind, estimator=estimator, key_offset=R.KEY, stats=st)
    print(f"{name} rng {rng_kind} estimator {estimator}: segments {st.segments} (oracle {seg}), shadow rays {st.shadow_rays} ({shadow}), "
          f"{int((want[:, :3].sum(1) > 0).sum())} of {R.N} rays see light")
    assert got.shape == (R.N, 4) and same(got, want), first_difference(got, want)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, R.N * R.SPP)
    assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    assert (want[:, :3].sum(1) > 0).sum() >= R.N // 4 and seg > R.N * R.SPP


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", R.SCENES)
def test_every_pixel_and_both_counts_are_the_oracles(gpu, monkeypatch, name, how, rng_kind):
    upload(gpu, monkeypatch, R.scene(name), how)
    check_case(gpu, name, rng_kind)


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("estimator", [1, 2, 3])
@pytest.mark.parametrize("how", list(UPLOADS))
def test_the_corrected_estimators_on_scene_0(gpu, monkeypatch, how, estimator, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"), how)
    check_case(gpu, "scene0", rng_kind, estimator)


# ---------------------------------------------------------------- 2. summation order and offsets
def lit_ray():
    """A scene-0 ray that sees light."""
    blob, o, ll, _, want, _, _ = R.case("scene0", abi.RTW_RNG_PHILOX)
    i = int(np.argmax(want[:, :3].sum(1)))
    return blob, o[i:i + 1], ll[i:i + 1]


def test_units_tails_and_sample_offsets(gpu, monkeypatch):
    blob, o1, ll1 = lit_ray()
    upload(gpu, monkeypatch, blob)
    o, ll = np.repeat(o1, 80, 0), np.repeat(ll1, 80, 0)
    rays = R.make_rays(o, ll)
    for spp, off in ((272, 0), (16, 16)):  # two units and a 16-sample tail; one block that starts at sample 16
        want, seg, shadow = R.expect(blob, o, ll, spp, 6, sample_offset=off, key_offset=9)
        st = abi.Stats()
        got = gpu.radiance(rays, spp, 6, sample_offset=off, key_offset=9, stats=st)
        assert same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 80 * spp)
        assert len(np.unique(got.view(np.uint32), axis=0)) > 40 and got[:, :3].sum() > 0  # one ray, eighty streams
    # the same samples reached two ways: samples 16 ... 31 are the second block of a 32-spp call
    first = gpu.radiance(rays[:1], 16, 6, key_offset=9)
    second = gpu.radiance(rays[:1], 16, 6, key_offset=9, sample_offset=16)
    both = gpu.radiance(rays[:1], 32, 6, key_offset=9)
    assert same(((first[:, :3] * np.float32(16) + second[:, :3] * np.float32(16)) / np.float32(32)), both[:, :3])
    o3, ll3 = R.pairs(blob, R.N)
    o3, ll3 = o3[:3], ll3[:3]
    for spp in (1, 129):
        want, seg, shadow = R.expect(blob, o3, ll3, spp, 8, rng_kind=abi.RTW_RNG_TEA_LCG, key_offset=1000)
        st = abi.Stats()
        got = gpu.radiance(R.make_rays(o3, ll3), spp, 8, rng_kind=abi.RTW_RNG_TEA_LCG, key_offset=1000, stats=st)
        assert same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 3 * spp)


# ---------------------------------------------------------------- 3. independence at scale
def test_a_ray_does_not_depend_on_its_batch(gpu, monkeypatch):
    """n = 2^19 + 3 rays: more units than the device holds lanes, so the queue hands out jobs to the end. 257 scattered rays equal
    one-ray calls with their own keys; at spp 144 the same through the unit slab and the resolve."""
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    n = (1 << 19) + 3
    rays, _, _ = G.scene_rays(blob, 7, n)
    rays[:, 6], rays[:, 7] = 1e-6, 1e27
    ends = np.array([0, 1, 63, 64, n - 2, n - 1])
    pick = np.concatenate([ends, np.setdiff1d(np.random.default_rng(3).choice(n, 300, replace=False), ends)[:251]])
    assert len(np.unique(pick)) == 257
    for spp in (16, 144):
        st = abi.Stats()
        big = gpu.radiance(rays, spp, 4, key_offset=0, stats=st)
        assert st.samples == n * spp and st.segments >= st.samples and (big[:, 3] == 1.0).all()
        assert (big[:, :3].sum(1) > 0).mean() > 0.2
        for j in pick:
            one = gpu.radiance(rays[j:j + 1], spp, 4, key_offset=int(j))
            assert same(one, big[j:j + 1]), (spp, j, one, big[j])
    d_big = radiance_torch(gpu, torch.from_numpy(rays).cuda(), 144, 4)
    assert same(d_big.cpu().numpy(), big)


def test_chunks_and_slab_ranges_do_not_change_the_bits(gpu, monkeypatch):
    blob = R.scene("scene1")
    upload(gpu, monkeypatch, blob)
    rays, _, _ = G.scene_rays(blob, 11, 5003)
    rays[:, 6], rays[:, 7] = 1e-6, 1e27
    for spp in (8, 144):
        for k in ("RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES"):
            monkeypatch.delenv(k, raising=False)
        s0, s1, s2 = abi.Stats(), abi.Stats(), abi.Stats()
        whole = gpu.radiance(rays, spp, 6, key_offset=123, stats=s0)
        monkeypatch.setenv("RTW_RADIANCE_CHUNK", "1000")
        assert same(gpu.radiance(rays, spp, 6, key_offset=123, stats=s1), whole)
        monkeypatch.delenv("RTW_RADIANCE_CHUNK")
        monkeypatch.setenv("RTW_RADIANCE_SLAB_BYTES", str(700 * 2 * 16))  # 700 rays of two units: eight ranges at spp 144
        assert same(gpu.radiance(rays, spp, 6, key_offset=123, stats=s2), whole)
        d = radiance_torch(gpu, torch.from_numpy(rays).cuda(), spp, 6, key_offset=123)
        assert same(d.cpu().numpy(), whole)
        for s in (s1, s2):
            assert (s.segments, s.shadow_rays, s.samples) == (s0.segments, s0.shadow_rays, s0.samples)
        assert (whole[:, :3].sum(1) > 0).mean() > 0.5


@pytest.mark.parametrize("rng_kind", BOTH)
def test_keys_wrap_modulo_2_to_the_32(gpu, monkeypatch, rng_kind):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    _, o, ll, _, lit, _, _ = R.case("scene0", abi.RTW_RNG_PHILOX)
    idx = np.argsort(-lit[:, :3].sum(1))[:8]
    o, ll = o[idx], ll[idx]
    k0 = 2 ** 32 - 3
    want, _, _ = R.expect(blob, o, ll, 16, 6, rng_kind=rng_kind, key_offset=k0)
    rays = R.make_rays(o, ll)
    got = gpu.radiance(rays, 16, 6, rng_kind=rng_kind, key_offset=k0)
    assert same(got, want), first_difference(got, want)
    assert same(gpu.radiance(rays[3:], 16, 6, rng_kind=rng_kind, key_offset=0), got[3:]) and got[:, :3].sum() > 0
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "2")  # a chunk that starts before the wrap and one that starts on it
    assert same(gpu.radiance(rays, 16, 6, rng_kind=rng_kind, key_offset=k0), want)


# ---------------------------------------------------------------- 4. the first segment's interval
def test_the_interval_bounds_the_first_segment_only(gpu, monkeypatch):
    blob, o, ll, rays, want, seg, _ = R.case("scene0", abi.RTW_RNG_PHILOX)
    upload(gpu, monkeypatch, blob)
    hits = gpu.cast(rays, want=("t", "prim"))
    hit = hits["prim"] >= 0
    assert hit.sum() >= R.N // 4
    short = rays[hit].copy()
    short[:, 7] = hits["t"][hit] * np.float32(0.5)  # tmax below the first hit: scene 0 has no sky, a miss is black
    st = abi.Stats()
    got = gpu.radiance(short, R.SPP, R.DEPTH, stats=st)
    assert same(got, np.tile(np.array([0, 0, 0, 1], np.float32), (len(short), 1)))
    assert (st.segments, st.shadow_rays, st.samples) == (len(short) * R.SPP, 0, len(short) * R.SPP)
    # tmin beyond the first hit: the path starts behind it, and goes on with the estimator's own start distance
    far = rays[hit].copy()
    far[:, 6] = hits["t"][hit] * np.float32(1.0001)
    assert not same(gpu.radiance(far, R.SPP, R.DEPTH, key_offset=R.KEY), want[hit])
    st0 = abi.Stats(segments=5)
    zero = gpu.radiance(rays, R.SPP, 0, stats=st0)
    assert same(zero, np.tile(np.array([0, 0, 0, 1], np.float32), (R.N, 1)))
    assert (st0.segments, st0.shadow_rays, st0.samples) == (0, 0, R.N * R.SPP)
    assert same(gpu.radiance(rays, 200, 0), zero)


# ---------------------------------------------------------------- 5. the device path
def test_radiance_torch_equals_radiance_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    blob, o, ll, rays, want, seg, shadow = R.case("random_volumes_motion", abi.RTW_RNG_PHILOX)
    upload(gpu, monkeypatch, blob)
    kw = dict(key_offset=R.KEY)
    d_rays = torch.from_numpy(rays).cuda()
    st = abi.Stats()
    got = radiance_torch(gpu, d_rays, R.SPP, R.DEPTH, stats=st, **kw)
    assert got.is_cuda and tuple(got.shape) == (R.N, 4) and same(got.cpu().numpy(), want)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, R.N * R.SPP) and st.seconds > 0.0
    check_stream_order(lambda t: radiance_torch(gpu, t, R.SPP, R.DEPTH, **kw), d_rays, lambda got: same(got.cpu().numpy(), want))
    assert tuple(radiance_torch(gpu, torch.zeros((0, 8), device="cuda:0"), 4, 4).shape) == (0, 4)
    with pytest.raises(ValueError):
        radiance_torch(gpu, d_rays, 0, R.DEPTH)


def test_every_refusal_leaves_the_context_usable(gpu, monkeypatch):
    blob, o, ll, rays, want, _, _ = R.case("scene0", abi.RTW_RNG_PHILOX)
    lib, n = gpu.lib, R.N
    out = np.full((n, 4), -7, np.float32)
    d_rays = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(8, np.float32)])).cuda()
    d_out = torch.full((n * 4 + 8,), -7.0, device="cuda:0")
    R_, O_, D_, DO_ = rays.ctypes.data, out.ctypes.data, d_rays.data_ptr(), d_out.data_ptr()

    def rp(**kw):
        p = abi.make_radiance_params(R.SPP, R.DEPTH, key_offset=R.KEY)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_radiance(fresh.ctx, R_, n, rp(), O_, None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_radiance_device(fresh.ctx, D_, n, rp(), DO_, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()
    upload(gpu, monkeypatch, blob)

    def still_fine():
        assert same(gpu.radiance(rays, R.SPP, R.DEPTH, key_offset=R.KEY), want)
    bad_params = [None, rp(spp=0), rp(spp=-1), rp(max_depth=-1), rp(rng_kind=2), rp(rng_kind=-1), rp(estimator=4), rp(estimator=-1),
                  rp(sample_offset=-1), rp(sample_offset=2 ** 31 - R.SPP), rp(spp=2 ** 31 - 1, sample_offset=1), rp(reserved=1)]
    refusals = [(R_, n, p, O_) for p in bad_params] + [(R_, 1 << 31, rp(), O_), (None, n, rp(), O_), (R_, n, rp(), None)]
    for r_, m, p, o_ in refusals:
        st = sentinel_stats()
        assert lib.rtw_radiance(gpu.ctx, r_, m, p, o_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    still_fine()
    dev_refusals = [(D_, n, p, DO_) for p in bad_params] + [(D_, 1 << 31, rp(), DO_), (None, n, rp(), DO_), (D_, n, rp(), None),
                                                            (D_ + 4, n, rp(), DO_), (D_ + 8, n, rp(), DO_), (D_, n, rp(), DO_ + 4), (D_, n, rp(), DO_ + 8)]
    for r_, m, p, o_ in dev_refusals:
        st = sentinel_stats()
        assert lib.rtw_radiance_device(gpu.ctx, r_, m, p, o_, None, C.byref(st)) == -1
        assert left_alone(st)
        still_fine()  # after a misaligned pointer as after any other refusal: the next call works
    torch.cuda.synchronize()
    assert (out == -7).all() and bool((d_out == -7).all().item())  # no refused call wrote anything
    # n = 0 is fine and launches nothing, whatever the pointers
    st = abi.Stats(segments=77)
    assert lib.rtw_radiance(gpu.ctx, None, 0, rp(), None, C.byref(st)) == 0 and (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
    assert lib.rtw_radiance_device(gpu.ctx, None, 0, rp(), None, None, None) == 0
    assert lib.rtw_radiance_device(gpu.ctx, D_ + 4, 0, rp(), DO_ + 4, None, None) == 0
    assert gpu.radiance(np.zeros((0, 8), np.float32), 4, 4).shape == (0, 4)
    assert lib.rtw_radiance_device(gpu.ctx, D_ + 32, n - 1, rp(key_offset=R.KEY + 1), DO_ + 16, None, None) == 0  # from ray 1 on: aligned enough
    assert same(d_out[4:4 + 4 * (n - 1)].cpu().numpy().reshape(-1, 4), want[1:])


# ---------------------------------------------------------------- 6. neighbours
def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    blob, o, ll, rays, want, seg, shadow = R.case("scene1", abi.RTW_RNG_PHILOX)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    group = abi.Renderer([0, 0])
    try:
        out = np.zeros((R.N, 4), np.float32)
        rp = abi.make_radiance_params(R.SPP, R.DEPTH)
        assert group.lib.rtw_radiance(group.ctx, rays.ctypes.data, R.N, C.byref(rp), out.ctypes.data, None) == -3
        group.upload_scene(blob)
        st = abi.Stats()
        assert same(group.radiance(rays, R.SPP, R.DEPTH, key_offset=R.KEY, stats=st), want)
        assert (st.segments, st.shadow_rays) == (seg, shadow)
        assert same(radiance_torch(group, torch.from_numpy(rays).cuda(), R.SPP, R.DEPTH, key_offset=R.KEY).cpu().numpy(), want)
        assert same(group.radiance(rays, 144, 4, key_offset=R.KEY)[:, 3], np.ones(R.N, np.float32))
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    blob, o, ll, rays, want, _, _ = R.case("scene0", abi.RTW_RNG_PHILOX)
    upload(gpu, monkeypatch, blob)
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        assert same(gpu.radiance(rays, R.SPP, R.DEPTH, key_offset=R.KEY), want)
        assert same(radiance_torch(gpu, torch.from_numpy(rays).cuda(), R.SPP, R.DEPTH, key_offset=R.KEY).cpu().numpy(), want)
        gpu.radiance(rays, 144, 4)  # the unit slab and the resolve
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    assert same(gpu.radiance(rays, R.SPP, R.DEPTH, key_offset=R.KEY), want)


def test_rtw_render_after_radiance_calls_still_matches_its_golden_fixture(gpu, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for g in map(golden, GOLDEN_PAIR):
        blob, rng, seed = g.blob, g.rng, g.seed
        gpu.upload_scene(blob)
        o, ll = R.pairs(blob, 300)
        rays = R.make_rays(o, ll)
        a = gpu.radiance(rays, 24, 6, rng_kind=rng)
        b = gpu.radiance(rays, 160, 3, rng_kind=rng, estimator=1)
        assert np.isfinite(a).all() and np.isfinite(b).all() and a[:, :3].sum() > 0
        check_golden_render(gpu, g)
        assert same(gpu.radiance(rays, 24, 6, rng_kind=rng), a)
